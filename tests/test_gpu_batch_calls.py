"""GPU tests (-m gpu) of the host side of the batched queries: the ten device entry points (prt_trace_closest_device,
prt_trace_{closest_device_prec, closest_sorted, occluded, occluded_sorted, surface, surface_sorted, multi, multi_sorted}_device,
prt_closest_point_device) and the five host-buffer ones (prt_trace_closest / occluded / surface / multi, prt_closest_point)
share one call frame in prt_api.cpp.  What the kernels compute is tested elsewhere; here the scene is one quad and the
batches are tiny, and the subject is what the frame does around the launch: every refusal's code and text, the state a
refusal leaves behind, the counters, the timed region, and the sort scratch between calls on two streams.

The refusal texts below are written out, not derived: they were recorded from the library as it was before the call frame
was folded, and the folded frame has to reproduce them byte for byte."""

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes

pytestmark = pytest.mark.gpu

F64, F32 = _abi.PRECISION_F64, _abi.PRECISION_F32
K1_CHUNK = 1024  # PRT_K1_CHUNK (prt_kernels.hip): rays a wave's pool takes per refill
SIZES = (0, 1, 65, K1_CHUNK + 1)  # empty; one lane; one over a wave; one over the chunk (a second refill, a ragged tail)
OUT_DTYPE = {"hit": _abi.HIT_DTYPE, "occ": np.dtype(np.uint8), "surf": _abi.SURFACE_DTYPE, "multi": _abi.HIT_DTYPE,
             "cp": _abi.CLOSEST_POINT_DTYPE}
K = 2  # records per ray of the multi-hit calls

# name -> (what it writes, its host-buffer form or None, takes a precision, sorts)
DEVICE = {
    "prt_trace_closest_device": ("hit", "prt_trace_closest", False, False),
    "prt_trace_closest_device_prec": ("hit", "prt_trace_closest", True, False),
    "prt_trace_closest_sorted_device": ("hit", None, True, True),
    "prt_trace_occluded_device": ("occ", "prt_trace_occluded", True, False),
    "prt_trace_occluded_sorted_device": ("occ", None, True, True),
    "prt_trace_surface_device": ("surf", "prt_trace_surface", True, False),
    "prt_trace_surface_sorted_device": ("surf", None, True, True),
    "prt_trace_multi_device": ("multi", "prt_trace_multi", True, False),
    "prt_trace_multi_sorted_device": ("multi", None, True, True),
    "prt_closest_point_device": ("cp", "prt_closest_point", False, False),
}
HOST = {"prt_trace_closest": "hit", "prt_trace_occluded": "occ", "prt_trace_surface": "surf", "prt_trace_multi": "multi",
        "prt_closest_point": "cp"}

# (entry point, fault) -> the message; every refusal returns PRT_E_INVALID.  Faults: a null input (n = 1), a null output
# (n = 1), the output 8 bytes past a 32-byte boundary, precision 7, k = 0, k = PRT_MULTI_HIT_MAX + 1, n = 2^32 (with valid
# one-element buffers: refused before anything is dereferenced), distance queries switched off.
REFUSALS = {
    ("prt_trace_closest_device", "null input"): "prt_trace_closest_device: null buffer",
    ("prt_trace_closest_device", "null output"): "prt_trace_closest_device: null buffer",
    ("prt_trace_closest_device_prec", "null input"): "prt_trace_closest_device: null buffer",
    ("prt_trace_closest_device_prec", "null output"): "prt_trace_closest_device: null buffer",
    ("prt_trace_closest_device_prec", "precision 7"): "prt_trace_closest_device: unsupported precision",
    ("prt_trace_closest_sorted_device", "null input"): "prt_trace_closest_sorted_device: null buffer",
    ("prt_trace_closest_sorted_device", "null output"): "prt_trace_closest_sorted_device: null buffer",
    ("prt_trace_closest_sorted_device", "precision 7"): "prt_trace_closest_sorted_device: unsupported precision",
    ("prt_trace_closest_sorted_device", "n = 2^32"): "prt_trace_closest_sorted_device: more than 2^32 - 1 rays in one batch",
    ("prt_trace_occluded_device", "null input"): "prt_trace_occluded_device: null buffer",
    ("prt_trace_occluded_device", "null output"): "prt_trace_occluded_device: null buffer",
    ("prt_trace_occluded_device", "precision 7"): "prt_trace_occluded_device: unsupported precision",
    ("prt_trace_occluded_sorted_device", "null input"): "prt_trace_occluded_sorted_device: null buffer",
    ("prt_trace_occluded_sorted_device", "null output"): "prt_trace_occluded_sorted_device: null buffer",
    ("prt_trace_occluded_sorted_device", "precision 7"): "prt_trace_occluded_sorted_device: unsupported precision",
    ("prt_trace_occluded_sorted_device", "n = 2^32"): "prt_trace_occluded_sorted_device: more than 2^32 - 1 rays in one batch",
    ("prt_trace_surface_device", "null input"): "prt_trace_surface_device: null buffer",
    ("prt_trace_surface_device", "null output"): "prt_trace_surface_device: null buffer",
    ("prt_trace_surface_device", "misaligned output"): "prt_trace_surface_device: output buffer is not 32-byte aligned",
    ("prt_trace_surface_device", "precision 7"): "prt_trace_surface_device: unsupported precision",
    ("prt_trace_surface_sorted_device", "null input"): "prt_trace_surface_sorted_device: null buffer",
    ("prt_trace_surface_sorted_device", "null output"): "prt_trace_surface_sorted_device: null buffer",
    ("prt_trace_surface_sorted_device", "misaligned output"): "prt_trace_surface_sorted_device: output buffer is not 32-byte aligned",
    ("prt_trace_surface_sorted_device", "precision 7"): "prt_trace_surface_sorted_device: unsupported precision",
    ("prt_trace_surface_sorted_device", "n = 2^32"): "prt_trace_surface_sorted_device: more than 2^32 - 1 rays in one batch",
    ("prt_trace_multi_device", "null input"): "prt_trace_multi_device: null buffer",
    ("prt_trace_multi_device", "null output"): "prt_trace_multi_device: null buffer",
    ("prt_trace_multi_device", "misaligned output"): "prt_trace_multi_device: output buffer is not 32-byte aligned",
    ("prt_trace_multi_device", "precision 7"): "prt_trace_multi_device: unsupported precision",
    ("prt_trace_multi_device", "k = 0"): "prt_trace_multi_device: k must be 1..8",
    ("prt_trace_multi_device", "k = 9"): "prt_trace_multi_device: k must be 1..8",
    ("prt_trace_multi_sorted_device", "null input"): "prt_trace_multi_sorted_device: null buffer",
    ("prt_trace_multi_sorted_device", "null output"): "prt_trace_multi_sorted_device: null buffer",
    ("prt_trace_multi_sorted_device", "misaligned output"): "prt_trace_multi_sorted_device: output buffer is not 32-byte aligned",
    ("prt_trace_multi_sorted_device", "precision 7"): "prt_trace_multi_sorted_device: unsupported precision",
    ("prt_trace_multi_sorted_device", "k = 0"): "prt_trace_multi_sorted_device: k must be 1..8",
    ("prt_trace_multi_sorted_device", "k = 9"): "prt_trace_multi_sorted_device: k must be 1..8",
    ("prt_trace_multi_sorted_device", "n = 2^32"): "prt_trace_multi_sorted_device: more than 2^32 - 1 rays in one batch",
    ("prt_closest_point_device", "null input"): "prt_closest_point_device: null buffer",
    ("prt_closest_point_device", "null output"): "prt_closest_point_device: null buffer",
    ("prt_closest_point_device", "misaligned output"): "prt_closest_point_device: output buffer is not 32-byte aligned",
    ("prt_closest_point_device", "n = 2^32"): "prt_closest_point_device: more than 2^32 - 1 queries in one batch",
    ("prt_closest_point_device", "distance queries off"):
        "prt_closest_point_device: distance queries are off for this scene (prt_scene_set_distance_queries)",
    ("prt_trace_closest", "null input"): "prt_trace_closest: null buffer",
    ("prt_trace_closest", "null output"): "prt_trace_closest: null buffer",
    ("prt_trace_occluded", "null input"): "prt_trace_occluded: null buffer",
    ("prt_trace_occluded", "null output"): "prt_trace_occluded: null buffer",
    ("prt_trace_surface", "null input"): "prt_trace_surface: null buffer",
    ("prt_trace_surface", "null output"): "prt_trace_surface: null buffer",
    ("prt_trace_multi", "null input"): "prt_trace_multi: null buffer",
    ("prt_trace_multi", "null output"): "prt_trace_multi: null buffer",
    ("prt_trace_multi", "k = 0"): "prt_trace_multi: k must be 1..8",
    ("prt_trace_multi", "k = 9"): "prt_trace_multi: k must be 1..8",
    ("prt_closest_point", "null input"): "prt_closest_point: null buffer",
    ("prt_closest_point", "null output"): "prt_closest_point: null buffer",
    ("prt_closest_point", "n = 2^32"): "prt_closest_point: more than 2^32 - 1 queries in one batch",
    ("prt_closest_point", "distance queries off"):
        "prt_closest_point: distance queries are off for this scene (prt_scene_set_distance_queries)",
}
assert _abi.MULTI_HIT_MAX == 8  # "k = 9" is PRT_MULTI_HIT_MAX + 1, and the texts say 1..8


def quad_scene(gpu):
    """The unit square in the plane z = 0 as two triangles (prim 0: y <= x, prim 1: y >= x), distance queries on."""
    b = scenes._Builder("quad")
    m = b.material(scenes.Material("White", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    b.mesh("quad", m, *scenes.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)))
    sc = api.Scene(b.build(scenes.Camera(8, 8, 40.0, eye=(0.5, 0.5, 3.0), look_at=(0.5, 0.5, 0.0))))
    sc.distance_queries = True
    return sc.upload(gpu)


def inputs(kind, n):
    """n rays straight down from z = 1 (queries at z = 0.5 for `cp`): the even ones over prim 0, the odd ones beside the
    quad (the odd queries with a search radius that ends above it)."""
    i = np.arange(n)
    x = 0.55 + 0.4 * (i % 97) / 97.0 + np.where(i % 2 == 1, 2.0, 0.0)
    if kind == "cp":
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"] = np.stack([x - np.where(i % 2 == 1, 2.0, 0.0), np.full(n, 0.3), np.full(n, 0.5)], axis=-1)
        q["max_dist"] = np.where(i % 2 == 1, 0.25, np.inf)
        return q
    r = np.zeros(n, dtype=_abi.RAY_DTYPE)
    r["o"] = np.stack([x, np.full(n, 0.3), np.ones(n)], axis=-1)
    r["d"] = (0.0, 0.0, -1.0)
    r["tmin"], r["tmax"] = 1e-4, np.inf
    return r


def check_answer(kind, out, u=2.0 ** -53):
    """`out` answers inputs(kind, n): hits on prim 0 at t = 1 (dist = 0.5), misses on the odd elements.  Tolerance: the
    triangle test and the point-triangle distance are a few dozen roundings on operands of magnitude <= 2, so 64 units in
    the last place of the kernel's precision bound a value near 1 with room to spare."""
    n = out.shape[0]
    hit = np.arange(n) % 2 == 0
    tol = 64 * u
    if kind == "occ":
        assert np.array_equal(out, hit.astype(np.uint8))
        return
    rec = out[:, 0] if kind == "multi" else out
    assert np.array_equal(rec["prim"], np.where(hit, 0, -1))
    if kind == "cp":
        assert np.all(np.abs(rec["dist"][hit] - 0.5) <= tol) and np.all(np.isinf(rec["dist"][~hit]))
        assert np.all(np.abs(rec["point"][hit][:, 2]) <= tol)
        return
    assert np.all(np.abs(rec["t"][hit] - 1.0) <= tol) and np.all(np.isinf(rec["t"][~hit]))
    if kind == "multi":  # a ray crosses the quad once
        assert np.all(out[:, 1]["prim"] == -1)
    if kind == "surf":
        assert np.all(np.abs(rec["position"][hit][:, 2]) <= tol) and np.all(rec["material"][hit] == 0)


def dev_buffer(nbytes, fill=0xAA):
    import torch
    return torch.full((max(nbytes, 32) + 64,), fill, dtype=torch.uint8, device="cuda")


def to_dev(a):
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = dev_buffer(raw.size)
    d[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return d


def call(sc, name, inp, n, out, k=K, precision=F64, count=0, stream=None):
    """The C entry point `name` with raw addresses (None = null); returns (code, message)."""
    kind, _, prec, _ = DEVICE.get(name, (HOST.get(name), None, False, False))
    fn = getattr(sc._L, name)
    if name in HOST:
        args = (inp, None, n, k, out, int(count)) if kind == "multi" else (inp, n, out, int(count))
    elif kind == "multi":
        args = (inp, None, n, k, out, int(count), precision, stream)
    elif prec:
        args = (inp, n, out, int(count), precision, stream)
    else:
        args = (inp, n, out, int(count), stream)
    rc = fn(sc._h, *args)
    return rc, (sc._L.prt_last_error().decode() if rc else "")


def run(sc, name, inp, **kw):
    """A valid call of `name` on the host array `inp`; returns the output array (multi: (n, K))."""
    import torch
    kind = DEVICE[name][0] if name in DEVICE else HOST[name]
    n, dt = inp.shape[0], OUT_DTYPE[kind]
    per = dt.itemsize * (K if kind == "multi" else 1)
    if name in HOST:
        src = np.ascontiguousarray(inp)
        out = np.full(max(n * per, 1), 0xAA, dtype=np.uint8)
        rc, msg = call(sc, name, src.ctypes.data, n, out.ctypes.data, **kw)
    else:
        d_in, d_out = to_dev(inp), dev_buffer(n * per)
        assert d_out.data_ptr() % 32 == 0
        rc, msg = call(sc, name, d_in.data_ptr(), n, d_out.data_ptr(), **kw)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.all(out[n * per:] == 0xAA)  # nothing behind the n-th record is written
    assert rc == 0, (name, rc, msg)
    got = out[:n * per].view(dt)
    return got.reshape(n, K) if kind == "multi" else got


def ray_counters(kind, n):
    """(rays_closest, rays_shadow) of a batch of n."""
    return {"occ": (0, n), "cp": (0, 0)}.get(kind, (n, 0))


# ------------------------------------------------------------------------------------------------ 1
def test_every_refusal_and_the_state_it_leaves(gpu):
    sc = quad_scene(gpu)
    seen = set()
    for name in list(DEVICE) + list(HOST):
        kind = DEVICE[name][0] if name in DEVICE else HOST[name]
        dt = OUT_DTYPE[kind]
        one, two = inputs(kind, 1), inputs(kind, 2)
        for (who, fault), text in REFUSALS.items():
            if who != name:
                continue
            run(sc, name, two)  # the call before: two elements
            if name in HOST:
                keep = (np.ascontiguousarray(one), np.zeros(K * dt.itemsize + 64, dtype=np.uint8))
                p_in, p_out = keep[0].ctypes.data, keep[1].ctypes.data
            else:
                keep = (to_dev(one), dev_buffer(K * dt.itemsize))
                p_in, p_out = keep[0].data_ptr(), keep[1].data_ptr()
            kw = dict(inp=p_in, n=1, out=p_out)
            if fault == "null input":
                kw["inp"] = None
            elif fault == "null output":
                kw["out"] = None
            elif fault == "misaligned output":
                kw["out"] = p_out + 8
            elif fault == "precision 7":
                kw["precision"] = 7
            elif fault == "k = 0":
                kw["k"] = 0
            elif fault == "k = 9":
                kw["k"] = _abi.MULTI_HIT_MAX + 1
            elif fault == "n = 2^32":
                kw["n"] = 1 << 32
            elif fault == "distance queries off":
                sc.distance_queries = False
            else:
                raise AssertionError(fault)
            rc, msg = call(sc, name, **kw)
            print(f"{name}, {fault}: {rc} {msg!r}")
            assert rc == _abi.PRT_E_INVALID and msg == text, (name, fault, rc, msg)
            if fault == "distance queries off":
                sc.distance_queries = True
            # the scene still answers, and the counters are that answer's (one element, not the two of the call before)
            check_answer(kind, run(sc, name, one, count=1))
            c = sc.counters()
            assert (c["rays_closest"], c["rays_shadow"]) == ray_counters(kind, 1) and c["samples"] == 0, (name, fault, c)
            assert c["tri_tests"] > 0 and c["kernel_ms"] > 0, (name, fault, c)
            seen.add((who, fault))
    assert seen == set(REFUSALS)
    sc.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("kind", ["hit", "occ", "surf", "multi", "cp"])
def test_sequencing(gpu, kind):
    """Per batch size: the host form, then every device form of the same query, plain and sorted, fp64 and fp32."""
    sc = quad_scene(gpu)
    for n in SIZES:
        inp = inputs(kind, n)
        base = {}
        for name, (knd, host, prec, sorts) in DEVICE.items():
            if knd != kind:
                continue
            for precision in ((F64, F32) if prec else (F64,)):
                kw = dict(precision=precision) if prec else {}
                got = run(sc, name, inp, **kw)
                c = sc.counters()
                where = (name, n, precision)
                assert (c["rays_closest"], c["rays_shadow"]) == ray_counters(kind, n) and c["samples"] == 0, (where, c)
                assert c["kernel_ms"] > 0 if n else c["kernel_ms"] >= 0, (where, c)
                if precision not in base:  # the first form of a precision is a plain one
                    assert not sorts
                    check_answer(kind, got, 2.0 ** -53 if precision == F64 else 2.0 ** -24)
                    base[precision] = got
                assert got.tobytes() == base[precision].tobytes(), where  # sorted == plain, _prec == the legacy call
                if host and precision == F64:
                    assert run(sc, host, inp).tobytes() == got.tobytes(), where
                    c = sc.counters()
                    assert (c["rays_closest"], c["rays_shadow"]) == ray_counters(kind, n), (where, host, c)
    sc.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["prt_trace_closest_sorted_device", "prt_trace_multi_sorted_device"])
def test_sorted_calls_of_two_sizes_on_two_streams(gpu, name):
    """The sort scratch is one per scene: a sorted call on another stream waits for the previous one's end before it sorts
    (and before a larger batch replaces the buffer).  small, LARGE, small back to back on two streams, on a scene whose
    scratch does not exist yet; every call returns the plain call's bytes."""
    import torch
    kind = DEVICE[name][0]
    plain = name.replace("_sorted", "") + ("_prec" if kind == "hit" else "")
    per = OUT_DTYPE[kind].itemsize * (K if kind == "multi" else 1)
    sizes = (65, K1_CHUNK + 1, 65)
    for precision in (F64, F32):
        sc = quad_scene(gpu)
        want = [run(sc, plain, inputs(kind, n), precision=precision).tobytes() for n in sizes]
        d_in = [to_dev(inputs(kind, n)) for n in sizes]
        d_out = [dev_buffer(n * per) for n in sizes]
        streams = (torch.cuda.Stream(), torch.cuda.Stream())
        torch.cuda.synchronize()
        for i, n in enumerate(sizes):
            rc, msg = call(sc, name, d_in[i].data_ptr(), n, d_out[i].data_ptr(), precision=precision,
                           stream=streams[i % 2].cuda_stream)
            assert rc == 0, (i, rc, msg)
        torch.cuda.synchronize()
        for i, n in enumerate(sizes):
            assert d_out[i].cpu().numpy()[:n * per].tobytes() == want[i], (name, precision, i, n)
        sc.close()
