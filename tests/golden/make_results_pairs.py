#!/usr/bin/env python3
"""Cut fixtures out of the ONE piece of golden data the reference holds for this path — the `.hdr` + `.png` pairs that
`Camera::WriteColorAttachment` (reference Source/Camera.cpp:279-331, `LinearToSRGB` :206-221) wrote from the same
`colorAttachment` into the reference's Results/ directory.

They cannot pin the hot path (the scene files that produced them are absent), but they DO pin the output stage
 and exercise the image readers (f3): the .hdr holds the linear floats (as RGBE), the .png what
the reference's NaN scrub + sRGB + clamp + 8-bit truncation made of them.

Writes tests/golden/results_pairs.npz — DATA only (pixel bytes, encoded scanline bytes, sizes, checksums):
  pairs            names of the pairs
  crop_xy          (n_crops, 3): pair index, x0, y0 of each 128x128 crop
  crop_rgbe        (n_crops, 128, 128, 4) u8: RGBE bytes as stored in the .hdr
  crop_png         (n_crops, 128, 128, 3) u8: the PNG's pixels at the same place
  rle_rows         (n_rows, 2): pair index, row — whole scanlines kept with their ENCODED bytes
  rle_row_rgbe     (n_rows, W, 4) u8: the scanline's RGBE pixels
  rle_row_bytes    object-free: concatenated encoded bytes + offsets (stb_image_write's per-component RLE)
  hdr_header       the file header bytes (identical for the four files)
  file_sha256      sha256 of every .hdr file (so a full-file re-encode can be checked where the reference is present)
  png_crc32        zlib.crc32 of Pillow's decode of EVERY Results/*.png (full image), with the sizes

and tests/golden/results_cuts.npz — smaller WHOLE files cut out of them, so that the file-level tests need no Results/:
  band_rows        (n_pairs, 2): pair index, first row of a BAND_ROWS-row band of full scanlines (the brightest one)
  band_hdr_bytes   the band's encoded scanlines as the reference wrote them (+ band_hdr_offsets): with the header's
                   "-Y 720" replaced by "-Y BAND_ROWS" they are a complete .hdr file
  band_png         (n_pairs, BAND_ROWS, W, 3) u8: the reference PNG's pixels of the band
  png_cut_names    PNGs cut to their first png_cut_rows rows (cut_png below): the reference's own deflate bits up to the
  png_cut_bytes    cut, so stb's filter choices and fixed-Huffman coding are what the reader decodes (+ png_cut_offsets);
  png_cut_crc32    zlib.crc32 of Pillow's decode of each cut file, png_cut_size its (H, W, C)
Usage: python tests/golden/make_results_pairs.py <reference Results/ directory>   (never runs on the GPU box)
"""
import glob
import hashlib
import io
import os
import struct
import sys
import zlib

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
CROP = 128
BAND_ROWS = 8
# (file, rows): together the cuts hold rows of all five PNG filter types and every kind of deflate symbol
PNG_CUTS = [("bathroom2_20260324_0706_spp500-depth50_4421.03s.png", 72), ("cornell-box_20250327_0231_spp100-depth100_335.31s.png", 20),
            ("veach-mis_20250328_0423_spp12000-depth100_11320.95s.png", 16)]


def parse_hdr(data):
    """Radiance RGBE with per-component RLE scanlines -> (header bytes, (H, W, 4) u8, [(start, end) of each scanline])."""
    pos = data.index(b"\n\n") + 2
    end = data.index(b"\n", pos)
    dims = data[pos:end].split()
    assert dims[0] == b"-Y" and dims[2] == b"+X", dims
    h, w = int(dims[1]), int(dims[3])
    pos = end + 1
    header = data[:pos]
    px = np.zeros((h, w, 4), dtype=np.uint8)
    spans = []
    for y in range(h):
        start = pos
        assert data[pos] == 2 and data[pos + 1] == 2 and (data[pos + 2] << 8 | data[pos + 3]) == w, (y, data[pos:pos + 4])
        pos += 4
        for c in range(4):
            x = 0
            while x < w:
                n = data[pos]
                if n > 128:  # run
                    n -= 128
                    px[y, x:x + n, c] = data[pos + 1]
                    pos += 2
                else:        # literal dump
                    px[y, x:x + n, c] = np.frombuffer(data, dtype=np.uint8, count=n, offset=pos + 1)
                    pos += 1 + n
                x += n
            assert x == w
        spans.append((start, pos))
    assert pos == len(data), (pos, len(data))
    return header, px, spans


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class _BitReader:
    def __init__(self, data, pos):
        self.data, self.pos = data, pos  # in bits

    def bits(self, n):  # value stored LSB first (extra bits)
        v = 0
        for i in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def code(self, n):  # Huffman code, MSB first
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1)
            self.pos += 1
        return v

    def litlen(self):  # fixed Huffman literal / length symbol
        v = self.code(7)
        if v <= 0b0010111:
            return 256 + v
        v = (v << 1) | self.code(1)
        if 0b00110000 <= v <= 0b10111111:
            return v - 0b00110000
        if 0b11000000 <= v <= 0b11000111:
            return 280 + v - 0b11000000
        v = (v << 1) | self.code(1)
        return 144 + v - 0b110010000


class _BitWriter:
    def __init__(self, bits=()):
        self.out = list(bits)

    def bits(self, v, n):
        self.out += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):
        self.out += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def litlen(self, s):
        if s < 144:
            self.code(0b00110000 + s, 8)
        elif s < 256:
            self.code(0b110010000 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0b11000000 + s - 280, 8)

    def match(self, length, dist):
        i = max(k for k in range(29) if LEN_BASE[k] <= length)
        self.litlen(257 + i)
        self.bits(length - LEN_BASE[i], LEN_EXTRA[i])
        j = max(k for k in range(30) if DIST_BASE[k] <= dist)
        self.code(j, 5)
        self.bits(dist - DIST_BASE[j], DIST_EXTRA[j])

    def tobytes(self):
        b = self.out + [0] * (-len(self.out) % 8)
        return bytes(sum(b[k + i] << i for i in range(8)) for k in range(0, len(b), 8))


def _chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload))


def cut_png(png, rows):
    """The first `rows` rows of an 8-bit RGB PNG whose IDAT is ONE fixed-Huffman deflate block (stb_image_write's
    encoder), as a PNG that keeps the encoder's own bits: the symbols before the cut are copied verbatim, the one that
    straddles it is re-coded shorter, then end-of-block, the Adler-32 of the kept bytes and an IHDR with the new height."""
    pos, chunks = 8, []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        chunks.append((png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]))
        pos += 12 + n
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    ihdr, z = chunks[0][1], chunks[1][1]
    w, h, depth, ctype = struct.unpack(">IIBB", ihdr[:10])
    assert depth == 8 and ctype == 2 and rows <= h
    want = rows * (1 + 3 * w)
    r = _BitReader(z, 16)
    assert r.bits(1) == 1 and r.bits(2) == 1  # BFINAL, fixed Huffman
    out = bytearray()
    while len(out) < want:
        start = r.pos
        s = r.litlen()
        assert s != 256, "the block ends before the cut"
        if s < 256:
            out.append(s)
            length, dist = 1, None
        else:
            length = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
            j = r.code(5)
            dist = DIST_BASE[j] + r.bits(DIST_EXTRA[j])
            for _ in range(length):
                out.append(out[-dist])
    keep = want - (len(out) - length)  # bytes the last symbol must still produce
    head = _BitReader(z, 16)
    wr = _BitWriter(head.bits(1) for _ in range(start - 16))
    if keep == length:
        wr.out += [head.bits(1) for _ in range(r.pos - start)]
    elif keep >= 3:
        wr.match(keep, dist)
    else:
        for b in out[want - keep:want]:
            wr.litlen(b)
    wr.litlen(256)
    data = bytes(out[:want])
    newz = z[:2] + wr.tobytes() + struct.pack(">I", zlib.adler32(data))
    assert zlib.decompress(newz) == data
    return png[:8] + _chunk(b"IHDR", struct.pack(">II", w, rows) + ihdr[8:]) + _chunk(b"IDAT", newz) + _chunk(b"IEND", b"")


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_results_pairs.py <reference Results/ directory>")
    results = sys.argv[1]
    hdrs = sorted(glob.glob(os.path.join(results, "*.hdr")))
    pairs, crop_xy, crop_rgbe, crop_png, rle_rows, rle_row_rgbe, blobs, sha = [], [], [], [], [], [], [], []
    header0 = None
    for k, hp in enumerate(hdrs):
        pp = hp[:-4] + ".png"
        data = open(hp, "rb").read()
        header, px, spans = parse_hdr(data)
        header0 = header0 or header
        assert header == header0
        png = np.asarray(Image.open(pp).convert("RGB"))
        assert png.shape[:2] == px.shape[:2]
        h, w = px.shape[:2]
        pairs.append(os.path.basename(hp)[:-4])
        sha.append(hashlib.sha256(data).hexdigest())
        # crops: the brightest 128x128 block (window / lamp: clamped values, large exponents), the darkest, one in between
        e = px[..., 3].astype(np.int32)
        blocks = [(int(e[y:y + CROP, x:x + CROP].sum()), x, y) for y in range(0, h - CROP + 1, CROP) for x in range(0, w - CROP + 1, CROP)]
        blocks.sort()
        for _, x, y in (blocks[0], blocks[len(blocks) // 2], blocks[-1]):
            crop_xy.append((k, x, y))
            crop_rgbe.append(px[y:y + CROP, x:x + CROP].copy())
            crop_png.append(png[y:y + CROP, x:x + CROP].copy())
        for y in (0, h // 3, h // 2, h - 1):
            rle_rows.append((k, y))
            rle_row_rgbe.append(px[y].copy())
            blobs.append(data[spans[y][0]:spans[y][1]])
    offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    png_names, png_crc, png_size = [], [], []
    for pp in sorted(glob.glob(os.path.join(results, "*.png"))):
        a = np.asarray(Image.open(pp))
        png_names.append(os.path.basename(pp))
        png_crc.append(zlib.crc32(np.ascontiguousarray(a).tobytes()))
        png_size.append(a.shape if a.ndim == 3 else a.shape + (1,))
    out = os.path.join(HERE, "results_pairs.npz")
    np.savez_compressed(out, pairs=np.array(pairs), crop_xy=np.array(crop_xy, dtype=np.int32),
                        crop_rgbe=np.array(crop_rgbe), crop_png=np.array(crop_png),
                        rle_rows=np.array(rle_rows, dtype=np.int32), rle_row_rgbe=np.array(rle_row_rgbe),
                        rle_row_bytes=np.frombuffer(b"".join(blobs), dtype=np.uint8), rle_row_offsets=offs,
                        hdr_header=np.frombuffer(header0, dtype=np.uint8), file_sha256=np.array(sha),
                        png_names=np.array(png_names), png_crc32=np.array(png_crc, dtype=np.uint32), png_size=np.array(png_size, dtype=np.int32))
    print(out, os.path.getsize(out), "bytes;", len(crop_xy), "crops,", len(rle_rows), "scanlines,", len(png_names), "png checksums")

    band_rows, band_blobs, band_png = [], [], []
    for k, hp in enumerate(hdrs):
        _, px, spans = parse_hdr(open(hp, "rb").read())
        e = px[..., 3].astype(np.int64).sum(1)
        y0 = int(np.argmax(np.convolve(e, np.ones(BAND_ROWS, np.int64), "valid")))  # the brightest band: the widest brackets
        band_rows.append((k, y0))
        band_blobs.append(open(hp, "rb").read()[spans[y0][0]:spans[y0 + BAND_ROWS - 1][1]])
        band_png.append(np.asarray(Image.open(hp[:-4] + ".png").convert("RGB"))[y0:y0 + BAND_ROWS])
    cuts, cut_crc, cut_size = [], [], []
    for name, rows in PNG_CUTS:
        full = open(os.path.join(results, name), "rb").read()
        cut = cut_png(full, rows)
        a = np.asarray(Image.open(io.BytesIO(cut)))
        assert np.array_equal(a, np.asarray(Image.open(io.BytesIO(full)))[:rows])
        cuts.append(cut)
        cut_crc.append(zlib.crc32(np.ascontiguousarray(a).tobytes()))
        cut_size.append(a.shape)
    out = os.path.join(HERE, "results_cuts.npz")
    np.savez_compressed(out, band_rows=np.array(band_rows, dtype=np.int32),
                        band_hdr_bytes=np.frombuffer(b"".join(band_blobs), dtype=np.uint8),
                        band_hdr_offsets=np.cumsum([0] + [len(b) for b in band_blobs]).astype(np.int64), band_png=np.array(band_png),
                        png_cut_names=np.array([n for n, _ in PNG_CUTS]), png_cut_rows=np.array([r for _, r in PNG_CUTS], dtype=np.int32),
                        png_cut_bytes=np.frombuffer(b"".join(cuts), dtype=np.uint8),
                        png_cut_offsets=np.cumsum([0] + [len(c) for c in cuts]).astype(np.int64),
                        png_cut_crc32=np.array(cut_crc, dtype=np.uint32), png_cut_size=np.array(cut_size, dtype=np.int32))
    print(out, os.path.getsize(out), "bytes;", len(band_rows), "bands of", BAND_ROWS, "rows,", len(cuts), "cut PNGs")


if __name__ == "__main__":
    main()
