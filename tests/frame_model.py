"""numpy float64 references for the full-frame tests (tests/test_gpu_full_frame.py): the owned-item order of an
accumulator, active-pixel patterns and the states that select them, and the resolve / sRGB byte arithmetic of
k_resolve and k_tonemap (pooraytracer_amd/csrc/prt_kernels.hip).  The ownership rule itself is
pooraytracer_amd.distributed.tile_owner_map; the adaptive rule is tests/adaptive_model.py."""
import numpy as np

SEGMENT = 256  # owned items per segment of the adaptive select (PRT_BLOCK)
KNEE = 0.0031308  # LinearToSRGB's switch from the linear to the power segment
SV_MAX = 0.9999  # the clamp before * 255: byte 255 is never written
NEAR = 1e-9  # |sv * 255 - integer| below this: the device's pow may round the other way


def _tile(tile):
    return max(8, (tile + 7) // 8 * 8)


def owned_items(width, height, tile=32, rank=0, nranks=1):
    """Pixel index j*W+i of every owned item of a rank, in item order (tile_pixel in prt_device.h: the rank's tile slots
    in order, 8x8 blocks row by row inside a tile, pixels row by row inside a block); -1 for an item whose pixel lies
    outside the frame (the right and bottom partial tiles).  Its length is the rank's items_per_chunk."""
    t = _tile(tile)
    tiles_x, tiles_y = (width + t - 1) // t, (height + t - 1) // t
    k = np.arange(rank, tiles_x * tiles_y, nranks, dtype=np.int64)  # tile slots of this rank
    ty, kx = k // tiles_x, k % tiles_x
    tx = (kx + 3 * ty) % tiles_x
    w = np.arange(t * t, dtype=np.int64)
    blk, lane = w // 64, w % 64
    bpr = t // 8
    ox, oy = (blk % bpr) * 8 + lane % 8, (blk // bpr) * 8 + lane // 8
    px = (tx[:, None] * t + ox[None, :]).reshape(-1)
    py = (ty[:, None] * t + oy[None, :]).reshape(-1)
    return np.where((px < width) & (py < height), py * width + px, -1)


def patterns(items, seed=0):
    """The active-pixel patterns of the select test, as sorted pixel-index arrays: name -> pixels.  `items` is
    owned_items(); every pattern is a subset of the owned pixels."""
    rng = np.random.default_rng(seed)
    valid = items >= 0
    owned = items[valid]
    seg = np.arange(items.size) // SEGMENT
    pos = np.arange(items.size) % SEGMENT
    last_in_seg = (pos == SEGMENT - 1) | (np.arange(items.size) == items.size - 1)
    out = {
        "all": owned,
        "none": owned[:0],
        "last_item": owned[-1:],
        "segment_first": items[valid & (pos == 0)],
        "segment_last": items[valid & last_in_seg],
        "alternate_segments": items[valid & (seg % 2 == 0)],
        "all_but_one": np.delete(owned, owned.size // 2),
        "random_half": owned[rng.random(owned.size) < 0.5],
        "random_sparse": owned[rng.random(owned.size) < 0.003],
    }
    return {k: np.sort(v) for k, v in out.items()}


def select_state(width, height, owned, active, samples=16, batch=8, seed=0):
    """An adaptive state in which exactly the pixels `active` are active at n = samples (below min_spp): count = samples
    there, 0 or samples - batch on the other owned pixels, 0 off the rank.  Active pixels have zero sums and moments, the
    others random nonzero ones.  owned: (H, W) bool.  Returns the state dict (no fingerprint)."""
    rng = np.random.default_rng(seed)
    P = width * height
    own = np.asarray(owned, bool).reshape(-1)
    counts = np.where(own & (rng.random(P) < 0.5), samples - batch, 0).astype(np.uint32)
    counts[active] = samples
    sums = rng.uniform(0.5, 2.0, (P, 3))
    moments = rng.uniform(0.5, 2.0, P)
    sums[active] = 0.0
    moments[active] = 0.0
    return {"sums": sums.reshape(height, width, 3), "moments": moments.reshape(height, width),
            "counts": counts.reshape(height, width), "samples": samples}


def load_accepts(st, owned, batch, max_spp):
    """prt_accum_import_adaptive's checks of a state (include/prt.h): samples a multiple of batch and <= max_spp; every
    count <= samples, a multiple of batch and 0 off the rank's pixels; every moment finite and >= 0."""
    n = int(st["samples"])
    c = np.asarray(st["counts"]).reshape(-1).astype(np.int64)
    m = np.asarray(st["moments"]).reshape(-1)
    own = np.asarray(owned, bool).reshape(-1)
    return bool(n % batch == 0 and n <= max_spp and (c <= n).all() and (c % batch == 0).all() and not (c[~own] != 0).any()
                and np.isfinite(m).all() and (m >= 0).all())


def resolve64(sums, n):
    """k_resolve's fp64 frame of a plain accumulator: sums / n, zeros when n = 0."""
    sums = np.asarray(sums, np.float64)
    if n == 0:
        return np.zeros_like(sums)
    with np.errstate(all="ignore"):
        return sums / np.float64(n)


def resolve_counts64(sums, counts):
    """k_resolve's fp64 frame of an adaptive accumulator: each pixel's sums / its count, 0 where the count is 0."""
    sums = np.asarray(sums, np.float64)
    c = np.asarray(counts).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        return np.where(c > 0, sums / np.where(c > 0, c, 1.0), 0.0)


def srgb_sv255(x):
    """srgb8_of's value before truncation, in float64, of float32 inputs x: NaN -> 0, 12.92 v up to the knee and
    1.055 v^(1/2.4) - 0.055 above, clamped to [0, 0.9999], times 255."""
    v = np.asarray(x, np.float32).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    with np.errstate(all="ignore"):
        sv = np.where(v <= KNEE, 12.92 * v, 1.055 * np.power(np.maximum(v, 0.0), 1.0 / 2.4) - 0.055)
    sv = np.where(sv < 0.0, 0.0, np.where(sv > SV_MAX, SV_MAX, sv))
    return sv * 255.0


def srgb8(x):
    """The bytes k_tonemap writes for float32 inputs x, and a mask of the ones on the power segment within NEAR of a byte
    boundary (where the device's pow, a few ulps from numpy's, may land on the other side; the linear segment and the
    clamps are exact in both)."""
    s = srgb_sv255(x)
    v = np.asarray(x, np.float32).astype(np.float64)
    return s.astype(np.uint8), (v > KNEE) & (np.abs(s - np.rint(s)) <= NEAR)


def byte_boundaries():
    """The linear value at which byte b begins, b = 1 .. 254, in float64: the inverse of LinearToSRGB at b / 255
    (the linear segment below the knee's byte, the power segment above)."""
    b = np.arange(1, 255, dtype=np.float64)
    sv = b / 255.0
    lin = sv / 12.92
    pw = ((sv + 0.055) / 1.055) ** 2.4
    return np.where(lin <= KNEE, lin, pw)


def float32_neighbours(v, k=3):
    """The float32 values within k ulps of float32(v), for every v: (len(v), 2k + 1) float32."""
    f = np.asarray(v, np.float64).astype(np.float32)
    out = [f]
    lo, hi = f.copy(), f.copy()
    with np.errstate(over="ignore"):
        for _ in range(k):
            lo = np.nextafter(lo, np.float32(-np.inf))
            hi = np.nextafter(hi, np.float32(np.inf))
            out = [lo] + out + [hi]
    return np.stack(out, axis=1)


def edge_values():
    """float32 inputs where the resolve and the sRGB bytes go wrong first: NaN, +-Inf, +-0, negatives, fp32 subnormals,
    FLT_MAX and its neighbours, the knee +- 8 ulps, and every byte boundary +- 3 ulps; also ((b/255 + 0.055)/1.055)^2.4
    +- 3 ulps for every b = 0 .. 255, the power segment's inverse, which below the knee lies inside a byte."""
    f32 = np.finfo(np.float32)
    fixed = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1e-30, -0.5, -1.0, -3e38, 1e-45, 1.4e-45, 1e-40, 1.1754942e-38,
                      f32.tiny, f32.max, 1.0, 0.9999, 1e30], np.float32)
    knee = float32_neighbours([KNEE], 8).reshape(-1)
    b = np.arange(256, dtype=np.float64)
    formula = float32_neighbours(((b / 255.0 + 0.055) / 1.055) ** 2.4, 3).reshape(-1)
    bounds = float32_neighbours(byte_boundaries(), 3).reshape(-1)
    big = float32_neighbours([f32.max], 2).reshape(-1)
    return np.concatenate([fixed, knee, formula, bounds, big])


def edge_values64():
    """float64 resolve results around the fp32 limits: subnormal results, results above FLT_MAX (some round to FLT_MAX,
    the rest to +inf) and their negatives."""
    fmax = float(np.finfo(np.float32).max)
    half_ulp = 2.0 ** 103  # half an fp32 ulp at FLT_MAX: the float64 rounding boundary to +inf
    v = np.array([1e-39, 1e-42, 1e-45, 7e-46, 1.5e-45, 2.2e-44, 1e-300, fmax, fmax + half_ulp * 0.999, fmax + half_ulp,
                  fmax + half_ulp * 1.001, 1e39, 1e300, np.finfo(np.float64).max])
    return np.concatenate([v, -v])
