"""The reference helpers of the full-frame GPU tests (tests/frame_model.py) without a GPU: the sRGB byte model against
exact decimal arithmetic at every byte boundary, the owned-item order against tile_pixel and the ownership map, and the
select patterns and states against the checks of prt_accum_import_adaptive and the activity rule of adaptive_model."""
from decimal import Decimal, getcontext

import numpy as np
import pytest

from pooraytracer_amd import distributed
from tests import adaptive_model as AM
from tests import frame_model as F

FRAMES = [(1024, 1024, 32, 0, 1), (1031, 777, 24, 0, 1), (1031, 777, 24, 0, 3), (1031, 777, 24, 1, 3), (1031, 777, 24, 2, 3)]


def exact_sv255(x):
    """srgb8_of's sv * 255 for one float32, in 60-digit decimal arithmetic on the device's double constants."""
    getcontext().prec = 60
    v = float(np.float32(x))
    if v != v:
        v = 0.0
    if v <= F.KNEE:
        sv = Decimal(12.92) * Decimal(v)
    else:
        sv = Decimal(1.055) * Decimal(v) ** Decimal(1.0 / 2.4) - Decimal(0.055)
    sv = min(max(sv, Decimal(0)), Decimal(F.SV_MAX))
    return sv * 255


def test_srgb_byte_model_reproduces_every_byte_boundary():
    """Bytes 0..254 each begin at their boundary: on the float32 values within 3 ulps of it the model writes b - 1 below
    and b from there on, as exact arithmetic does.  Byte 255 is never written (the 0.9999 clamp)."""
    bounds = F.byte_boundaries()
    assert bounds.size == 254 and (np.diff(bounds) > 0).all()
    near_seen = 0
    for b, v in zip(range(1, 255), bounds):
        xs = F.float32_neighbours([v], 3)[0]
        got, near = F.srgb8(xs)
        exact = [exact_sv255(x) for x in xs]
        want = np.array([int(e) for e in exact], np.uint8)
        ok = (got == want) | near
        assert ok.all(), (b, xs.tolist(), got.tolist(), want.tolist())
        near_seen += int(near.sum())
        assert set(want.tolist()) == {b - 1, b}, (b, want.tolist())  # the boundary lies inside the +-3-ulp window
        assert (np.diff(want.astype(int)) >= 0).all()
    assert near_seen == 0, near_seen
    # below byte 1 everything is 0; the top of the range is 254
    got, _ = F.srgb8(np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, bounds[0] * 0.999, 1.0, 2.0, 3.4e38, np.inf],
                              np.float32))
    assert got.tolist() == [0, 0, 0, 0, 0, 0, 0, 254, 254, 254, 254]
    allb, _ = F.srgb8(np.linspace(0.0, 1.0, 1 << 20, dtype=np.float32))
    assert set(np.unique(allb).tolist()) == set(range(255))


def test_srgb_byte_model_matches_exact_arithmetic_on_the_edge_values():
    xs = F.edge_values()
    got, near = F.srgb8(xs)
    want = np.array([int(exact_sv255(x)) for x in xs], np.uint8)
    assert ((got == want) | near).all(), np.flatnonzero((got != want) & ~near)[:10].tolist()
    assert np.isnan(xs).any() and np.isinf(xs).any() and (np.signbit(xs) & (xs == 0)).any()
    sub = (xs != 0) & (np.abs(xs) < np.finfo(np.float32).tiny)
    assert sub.any()


def test_resolve_models():
    s = np.array([[1.0, -2.0, np.inf], [np.nan, 3.0, 6.0]])
    assert F.resolve64(s, 0).tobytes() == np.zeros_like(s).tobytes()
    assert np.array_equal(F.resolve64(s, 3), s / 3.0, equal_nan=True)
    c = np.array([0, 8])
    r = F.resolve_counts64(s, c)
    assert r[0].tobytes() == np.zeros(3).tobytes() and np.array_equal(r[1], s[1] / 8.0, equal_nan=True)
    v = F.edge_values64()
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    assert np.isinf(f).any() and (np.abs(f) == np.finfo(np.float32).max).any()
    assert ((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).any() and ((f == 0) & (v != 0)).any()


def _tile_pixel(width, height, tile, rank, nranks, oi):
    """tile_pixel of prt_device.h for one item, line by line (scramble off)."""
    t = max(8, (tile + 7) // 8 * 8)
    tiles_x, tiles_y = (width + t - 1) // t, (height + t - 1) // t
    ot, w = oi // (t * t), oi % (t * t)
    k = rank + ot * nranks
    if k >= tiles_x * tiles_y:
        return None
    ty, kx = k // tiles_x, k % tiles_x
    tx = (kx + 3 * ty) % tiles_x
    bpr = t // 8
    blk, lane = w // 64, w % 64
    by, bx = blk // bpr, blk % bpr
    px, py = tx * t + bx * 8 + lane % 8, ty * t + by * 8 + lane // 8
    return py * width + px if (px < width and py < height) else -1


@pytest.mark.parametrize("w,h,tile,rank,nranks", [(53, 41, 24, 0, 1), (53, 41, 16, 1, 3), (40, 40, 8, 2, 3)])
def test_owned_items_is_tile_pixel(w, h, tile, rank, nranks):
    items = F.owned_items(w, h, tile, rank, nranks)
    want = [_tile_pixel(w, h, tile, rank, nranks, i) for i in range(items.size)]
    assert None not in want and _tile_pixel(w, h, tile, rank, nranks, items.size + tile * tile) is None
    assert items.tolist() == want


@pytest.mark.parametrize("w,h,tile,rank,nranks", FRAMES)
def test_patterns_and_states_are_accepted_and_select_exactly_the_pattern(w, h, tile, rank, nranks):
    items = F.owned_items(w, h, tile, rank, nranks)
    own = distributed.owned_mask(w, h, tile, rank, nranks)
    valid = items[items >= 0]
    assert np.unique(valid).size == valid.size and np.array_equal(np.sort(valid), np.flatnonzero(own.reshape(-1)))
    n_seg = (items.size + F.SEGMENT - 1) // F.SEGMENT
    if (w, h) == (1024, 1024):
        assert items.size == 1 << 20 and n_seg == 4096  # 4 segments per scan thread
    else:
        assert (items < 0).any()  # partial tiles on the right and bottom edges
    pats = F.patterns(items)
    assert len(pats) == 9 and pats["none"].size == 0 and pats["all"].size == own.sum()
    assert pats["last_item"].tolist() == [valid[-1]] and pats["all_but_one"].size == own.sum() - 1
    assert 0 < pats["random_sparse"].size < pats["random_half"].size < own.sum()
    for name, p in pats.items():
        assert np.isin(p, valid).all() and np.unique(p).size == p.size, name
        st = F.select_state(w, h, own, p)
        assert F.load_accepts(st, own, batch=8, max_spp=128), name
        act = AM.active(st, 16, 64, 128, 8, 0.05, 0.0)
        assert np.array_equal(np.flatnonzero(act.reshape(-1)), p), name
        off = np.setdiff1d(np.flatnonzero(own.reshape(-1)), p)
        assert (st["sums"].reshape(-1, 3)[off] != 0).all() and (st["moments"].reshape(-1)[off] != 0).all()
        assert not st["sums"].reshape(-1, 3)[p].any() and not st["moments"].reshape(-1)[p].any()
    # a state that load() refuses is recognised as such
    st = F.select_state(w, h, own, pats["all"])
    bad = dict(st, counts=st["counts"] + np.uint32(4) * (st["counts"] > 0))
    assert not F.load_accepts(bad, own, 8, 128)
    if nranks > 1:
        bad = dict(st, counts=np.where(own, st["counts"], 8).astype(np.uint32))
        assert not F.load_accepts(bad, own, 8, 128)
