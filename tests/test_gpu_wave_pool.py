"""GPU tests (-m gpu) of the wave-local work pool (WavePool, csrc/prt_wave.h) through every entry that deals its items
through it: closest-hit, any-hit, surface and multi-hit (k = 3) batches in fp64 and fp32 (chunks of PRT_K1_CHUNK = 1024
rays), closest-point, signed-distance and winding-number batches (chunks of PRT_K6_CHUNK = PRT_K8_CHUNK = 256 queries).

What a record holds is tested elsewhere; the subject here is that a batch of n items is dealt completely, once, and to
nothing else.  Per entry one reference batch of N = 65537 random items on the tiny Cornell box is computed once: 257
blocks' worth of lanes but only 65 chunks of rays, so most waves find the counter past n on their first fetch.  Then,
for n around a wave, around one chunk, past two chunks and N itself, the first n items are run into a buffer prefilled with
a sentinel byte, 64 guard records behind the n-th:

  - records [0, n) are the reference's first n, byte for byte (a record is a pure function of its item, so an item that was
    dealt twice or never, or whose index was off by one, shows as a sentinel or as another item's record);
  - the guard is untouched (nothing at or past index n was dealt);
  - with count_work on, the ray entries' rays_closest / rays_shadow counter equals n: every item was dealt exactly once.

Both instantiations of every kernel run (count_work off and on), each against a reference of its own.  Every input is a
valid batch."""
import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes

pytestmark = pytest.mark.gpu

F64, F32 = _abi.PRECISION_F64, _abi.PRECISION_F32
N = 65537
GUARD = 64       # records behind the n-th
SENTINEL = 0xAA  # no record of these batches consists of this byte alone (see record_bytes)
K = 3            # records per ray of the multi-hit entry

# entry -> (input kind, bytes per item written, the counter that counts its items or None, chunk size)
ENTRIES = {
    "closest": ("rays", _abi.HIT_DTYPE.itemsize, "rays_closest", 1024),
    "any": ("rays", 1, "rays_shadow", 1024),
    "surface": ("rays", _abi.SURFACE_DTYPE.itemsize, "rays_closest", 1024),
    "multi": ("rays", K * _abi.HIT_DTYPE.itemsize, "rays_closest", 1024),
    "closest_point": ("points", _abi.CLOSEST_POINT_DTYPE.itemsize, None, 256),
    "signed_distance": ("points", _abi.SIGNED_DISTANCE_DTYPE.itemsize, None, 256),
    "winding_number": ("points", 8, None, 256),
}
CASES = [(e, p) for e in ("closest", "any", "surface", "multi") for p in (F64, F32)] + \
        [(e, F64) for e in ("closest_point", "signed_distance", "winding_number")]


def sizes(chunk):
    return (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 63, N)


def launch(sc, entry, precision, d_in, n, d_out, count):
    if entry == "closest":
        sc.trace_closest_device(d_in, n, d_out, count_work=count, precision=precision)
    elif entry == "any":
        sc.trace_occluded_device(d_in, n, d_out, count_work=count, precision=precision)
    elif entry == "surface":
        sc.trace_surface_device(d_in, n, d_out, count_work=count, precision=precision)
    elif entry == "multi":
        sc.trace_multi_device(d_in, n, K, d_out, None, count_work=count, precision=precision)
    elif entry == "closest_point":
        sc.closest_point_device(d_in, n, d_out, count_work=count)
    elif entry == "signed_distance":
        sc.signed_distance_device(d_in, n, d_out, count_work=count)
    else:
        sc.winding_number_device(d_in, n, d_out, beta=2.0, count_work=count)


@pytest.fixture(scope="module")
def world(gpu):
    """The scene and the two input batches on the device, made once."""
    import torch
    data = scenes.tiny_scene()
    sc = api.Scene(data)
    sc.signed_queries = True   # (switches distance queries on)
    sc.winding_queries = True
    sc.upload(gpu)
    rays = scenes.random_rays(N, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), seed=20261)
    q = np.zeros(N, dtype=_abi.POINT_QUERY_DTYPE)
    q["p"] = np.random.default_rng(20262).uniform(-1.2, 1.2, (N, 3))
    q["max_dist"] = np.inf
    dev = {kind: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
           for kind, a in (("rays", rays), ("points", q))}
    yield sc, dev
    sc.close()


def record_bytes(sc, dev, entry, precision, n, count):
    """The first n items of the entry's batch into a sentinel-filled buffer of n + GUARD records: (records, guard) as bytes."""
    import torch
    kind, per, _, _ = ENTRIES[entry]
    d_out = torch.full(((n + GUARD) * per,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 32 == 0
    launch(sc, entry, precision, dev[kind].data_ptr(), n, d_out.data_ptr(), count)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return out[:n * per], out[n * per:]


@pytest.mark.parametrize("count", [False, True], ids=["plain", "counting"])
@pytest.mark.parametrize("entry,precision", CASES, ids=[f"{e}-{'f32' if p == F32 else 'f64'}" for e, p in CASES])
def test_first_n_items_are_dealt_once_and_nothing_else(world, entry, precision, count):
    sc, dev = world
    _, per, counter, chunk = ENTRIES[entry]
    ref, guard = record_bytes(sc, dev, entry, precision, N, count)
    assert np.all(guard == SENTINEL), (entry, "reference")
    rec = ref.reshape(N, per)
    # every reference record was written: none is still the sentinel from end to end (a hit record's prim / a one-byte
    # answer of 0 or 1 / a finite winding number cannot be 0xAA.. bytes)
    assert not np.any(np.all(rec == SENTINEL, axis=1)), entry
    if count and counter:
        assert sc.counters()[counter] == N, (entry, sc.counters())
    for n in sizes(chunk):
        got, guard = record_bytes(sc, dev, entry, precision, n, count)
        differ = np.flatnonzero(np.any(got.reshape(n, per) != rec[:n], axis=1))
        print(f"{entry} precision {precision} count {int(count)} n {n}: {differ.size} records differ from the reference, "
              f"{int(np.count_nonzero(guard != SENTINEL))} guard bytes written")
        assert differ.size == 0, (entry, n, differ[:8])
        assert np.all(guard == SENTINEL), (entry, n)
        if count and counter:
            c = sc.counters()
            other = "rays_shadow" if counter == "rays_closest" else "rays_closest"
            assert c[counter] == n and c[other] == 0, (entry, n, c)
