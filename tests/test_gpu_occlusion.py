"""GPU tests of the any-hit occlusion queries (prt_trace_occluded*, Scene.trace_occluded*, Hittable::Occluded).

The statement under test is exact and tie-free: occluded[i] == (closest hit's prim >= 0) for the same ray record and
precision, whichever builder made the tree and whether or not the batch was sorted.  Against the CPU oracle the expected
answers are made unambiguous by the intervals: [tmin, t(1-m)] in front of the oracle's closest hit is empty, [tmin, t(1+m)]
contains it, with m far above the hit tolerance of the precision (1e-6 against 1e-12 in fp64, 1e-3 against 1e-5 in fp32).
Every case runs on host-built and device-built trees."""
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, build, scenes

pytestmark = pytest.mark.gpu

BUILDERS = (False, True)  # Scene(device_bvh=...)
K1_CHUNK = 1024           # PRT_K1_CHUNK: rays a wave takes from the global counter at a time


def _dev(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float64).reshape(-1, 8)).cuda()


def _closest(sc, rays, precision=0, sort=False, count_work=False, d_r=None):
    import torch
    n = rays.shape[0]
    d_r = _dev(rays) if d_r is None else d_r
    d_h = torch.zeros((max(n, 1), 4), dtype=torch.float64, device="cuda")
    sc.trace_closest_device(d_r.data_ptr(), n, d_h.data_ptr(), count_work=count_work, precision=precision, sort=sort)
    torch.cuda.synchronize()
    return d_h.cpu().numpy().view(_abi.HIT_DTYPE).reshape(-1)[:n]


def _occluded(sc, rays, precision=0, sort=False, count_work=False, d_r=None, extra=0):
    """The n answer bytes (and, with `extra`, the bytes behind them of a buffer prefilled with 0xAA)."""
    import torch
    n = rays.shape[0]
    d_r = _dev(rays) if d_r is None else d_r
    d_o = torch.full((n + max(extra, 1),), 0xAA, dtype=torch.uint8, device="cuda")
    sc.trace_occluded_device(d_r.data_ptr(), n, d_o.data_ptr(), count_work=count_work, precision=precision, sort=sort)
    torch.cuda.synchronize()
    out = d_o.cpu().numpy()
    return (out[:n], out[n:]) if extra else out[:n]


def _mixed_rays(data, n_each, seed):
    lo, hi = data.bounds()
    return np.concatenate([scenes.random_rays(n_each, lo, hi, seed=seed), scenes.camera_rays(data.camera, n_each, seed=seed + 1)])


def _finite_tmax(rays, t_closest, seed):
    """The same rays with a finite tmax each: hits get t * U(0.5, 1.5) — about half of them end in front of their hit —
    and misses a length of the same distribution."""
    rng = np.random.default_rng(seed)
    hit = np.isfinite(t_closest)
    scale = np.where(hit, t_closest, np.median(t_closest[hit]) if hit.any() else 1.0)
    out = rays.copy()
    out["tmax"] = scale * rng.uniform(0.5, 1.5, rays.shape[0])
    return out


SCENES_EQ = [
    ("cornell-box", lambda: scenes.cornell_box(ball_subdiv=4, width=256, height=256)),
    ("bathroom", lambda: scenes.bathroom(128, 72, detail=0.15)),
    ("mixed", lambda: scenes.mixed_materials(64, 64)),
]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name,scene_fn", SCENES_EQ)
def test_equals_closest_hit_exactly(gpu, name, scene_fn, device_bvh):
    data = scene_fn()
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    rays = _mixed_rays(data, 200_000, seed=21)
    t_inf = _closest(sc, rays)["t"]
    for batch in (rays, _finite_tmax(rays, t_inf, seed=23)):
        d_r = _dev(batch)
        for prec in (_abi.PRECISION_F64, _abi.PRECISION_F32):
            want = _closest(sc, batch, precision=prec, d_r=d_r)["prim"] >= 0
            got = _occluded(sc, batch, precision=prec, d_r=d_r)
            assert set(np.unique(got)) <= {0, 1}
            bad = int((got.astype(bool) != want).sum())
            print(f"{name} device_bvh={device_bvh} prec={prec} finite={batch is not rays}: occluded {got.mean():.3f}, mismatches {bad}")
            assert bad == 0
            assert 0.02 < want.mean() < 1.0 or batch is rays
    # the finite batch really cut hits off: fewer occluded rays than with tmax = inf, but not none
    fin = _occluded(sc, _finite_tmax(rays, t_inf, seed=23))
    hit = np.isfinite(t_inf)
    assert 0.3 < fin[hit].mean() < 0.7
    sc.close()


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("n_tris", [2_000_000, 3_000_000])
def test_equals_closest_hit_on_a_soup_plain_and_sorted(gpu, n_tris, device_bvh):
    """Records are padded to one per 128-byte line once they exceed PRT_TRI_PADDED_ABOVE (256 MiB: 2.8M fp64 records), so
    the 2M-triangle soup still runs the packed instantiations and the 3M-triangle one the PAD instantiations."""
    data = scenes.triangle_soup(n_tris=n_tris, with_light=False)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    info = sc.bvh_info()
    assert info["tri_stride"] == (128 if n_tris * info["tri_bytes"] > (256 << 20) else info["tri_bytes"])
    assert (info["tri_stride"] == 128) == (n_tris == 3_000_000)
    lo, hi = data.bounds()
    rays = scenes.random_rays(400_000, lo, hi, seed=31)
    t_inf = _closest(sc, rays)["t"]
    for batch in (rays, _finite_tmax(rays, t_inf, seed=33)):
        d_r = _dev(batch)
        for prec in (_abi.PRECISION_F64, _abi.PRECISION_F32):
            want = _closest(sc, batch, precision=prec, d_r=d_r)["prim"] >= 0
            for sort in (False, True):
                got = _occluded(sc, batch, precision=prec, sort=sort, d_r=d_r)
                bad = int((got.astype(bool) != want).sum())
                print(f"soup {n_tris} device_bvh={device_bvh} prec={prec} sort={sort}: occluded {got.mean():.3f}, mismatches {bad}")
                assert bad == 0
    sc.close()


# ------------------------------------------------------------------------------------------------ 2
SCENES_ORACLE = [
    ("tiny", scenes.tiny_scene, 30_000),
    ("mixed", lambda: scenes.mixed_materials(64, 64), 30_000),
    ("cornell-box", lambda: scenes.cornell_box(ball_subdiv=4, width=256, height=256), 30_000),
]


def _oracle_intervals(data, n_each, m, seed):
    """Rays the oracle hits at t, as two batches: over [tmin, t(1-m)] (empty: checked with the oracle itself, on every
    ray, nothing dropped) and over [tmin, t(1+m)] (holds the hit); and the rays the oracle misses, with tmax = inf."""
    orc = oracle.Oracle(data)
    rays = _mixed_rays(data, n_each, seed)
    h = orc.trace_closest(rays)
    hit = h["prim"] >= 0
    before, upto = rays[hit].copy(), rays[hit].copy()
    before["tmax"] = h["t"][hit] * (1.0 - m)
    upto["tmax"] = h["t"][hit] * (1.0 + m)
    assert (before["tmax"] > before["tmin"]).all()
    assert (orc.trace_closest(before)["prim"] < 0).all(), "generator: the interval in front of the closest hit is not empty"
    assert (orc.trace_closest(upto)["prim"] >= 0).all()
    orc.close()
    return before, upto, rays[~hit]


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("prec,m", [(_abi.PRECISION_F64, 1e-6), (_abi.PRECISION_F32, 1e-3)])
def test_equals_the_oracle_on_intervals_around_its_hits(gpu, prec, m, device_bvh):
    total = 0
    for name, scene_fn, n_each in SCENES_ORACLE:
        data = scene_fn()
        before, upto, missed = _oracle_intervals(data, n_each, m, seed=41)
        total += before.shape[0]
        sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
        a = _occluded(sc, before, precision=prec)
        b = _occluded(sc, upto, precision=prec)
        c = _occluded(sc, missed, precision=prec) if missed.shape[0] else np.zeros(0, np.uint8)
        print(f"{name} device_bvh={device_bvh} prec={prec} m={m}: {before.shape[0]} hits, occluded in front {int(a.sum())}, "
              f"not occluded up to the hit {int((b == 0).sum())}; {missed.shape[0]} misses, occluded {int(c.sum())}")
        assert int(a.sum()) == 0
        assert int((b == 0).sum()) == 0
        assert int(c.sum()) == 0
        sc.close()
    assert total >= 50_000


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_shadow_segments_between_surface_points_equal_the_oracle(gpu, device_bvh):
    data = scenes.cornell_box(ball_subdiv=4, width=256, height=256)
    rays = scenes.shadow_segments(data, 100_000, seed=51)
    orc = oracle.Oracle(data)
    want = orc.trace_closest(rays)["prim"] >= 0
    orc.close()
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    got = _occluded(sc, rays)
    bad = int((got.astype(bool) != want).sum())
    print(f"shadow segments device_bvh={device_bvh}: {rays.shape[0]} rays, occluded {want.mean():.3f}, mismatches {bad}")
    assert 0.05 < want.mean() < 0.95
    assert bad == 0
    assert np.array_equal(sc.trace_occluded(rays), got)  # the host-buffer call
    sc.close()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_invariances(gpu, device_bvh):
    import torch
    data = scenes.cornell_box(ball_subdiv=4, width=256, height=256)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    rays = _mixed_rays(data, 100_000, seed=61)
    rays = _finite_tmax(rays, _closest(sc, rays)["t"], seed=63)
    n = rays.shape[0]
    for prec in (_abi.PRECISION_F64, _abi.PRECISION_F32):
        base, tail = _occluded(sc, rays, precision=prec, extra=4096)
        assert (tail == 0xAA).all()  # nothing behind the n-th byte is written
        assert 0.1 < base.mean() < 0.9
        srt, tail = _occluded(sc, rays, precision=prec, sort=True, extra=4096)
        assert (tail == 0xAA).all() and np.array_equal(srt, base)
        perm = np.random.default_rng(65).permutation(n)
        assert np.array_equal(_occluded(sc, rays[perm], precision=prec), base[perm])
        assert np.array_equal(_occluded(sc, rays[perm], precision=prec, sort=True), base[perm])
        # two calls in flight on two streams against serial calls
        half = n // 2
        d_a, d_b = _dev(rays[:half]), _dev(rays[half:])
        o_a = torch.full((half,), 0xAA, dtype=torch.uint8, device="cuda")
        o_b = torch.full((n - half,), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
        for _ in range(3):
            with torch.cuda.stream(s_a):
                sc.trace_occluded_device(d_a.data_ptr(), half, o_a.data_ptr(), precision=prec, stream=s_a.cuda_stream)
            with torch.cuda.stream(s_b):
                sc.trace_occluded_device(d_b.data_ptr(), n - half, o_b.data_ptr(), precision=prec, stream=s_b.cuda_stream, sort=True)
        torch.cuda.synchronize()
        assert np.array_equal(np.concatenate([o_a.cpu().numpy(), o_b.cpu().numpy()]), base)
        # batch sizes around a wave and around the pool chunk; n = 0 writes nothing
        for m in (1, 63, 64, 65, K1_CHUNK - 1, K1_CHUNK + 1, 0):
            for sort in (False, True):
                got, tail = _occluded(sc, rays[:m], precision=prec, sort=sort, extra=256)
                assert np.array_equal(got, base[:m]) and (tail == 0xAA).all(), (m, sort)
        for m in (1, 65, K1_CHUNK + 1):
            assert np.array_equal(sc.trace_occluded(rays[:m]), _occluded(sc, rays[:m]))
    sc.close()


def test_argument_checks_on_an_uploaded_scene(gpu):
    import torch
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    d_r = torch.zeros((4, 8), dtype=torch.float64, device="cuda")
    d_o = torch.zeros(4, dtype=torch.uint8, device="cuda")
    for sort in (False, True):
        for args in ((None, 4, d_o.data_ptr()), (d_r.data_ptr(), 4, None)):
            with pytest.raises(api.PrtError) as e:
                sc.trace_occluded_device(*args, sort=sort)
            assert e.value.code == _abi.PRT_E_INVALID
        with pytest.raises(api.PrtError) as e:
            sc.trace_occluded_device(d_r.data_ptr(), 4, d_o.data_ptr(), precision=7, sort=sort)
        assert e.value.code == _abi.PRT_E_INVALID
        sc.trace_occluded_device(None, 0, None, sort=sort)
    with pytest.raises(api.PrtError) as e:
        sc.trace_occluded_device(d_r.data_ptr(), 1 << 32, d_o.data_ptr(), sort=True)
    assert e.value.code == _abi.PRT_E_INVALID
    # the messages of the seven public batch calls, closest-hit and any-hit, name the call (prt_trace_closest_device_prec
    # is prt_trace_closest_device with a precision and reports under that name)
    fresh = api.Scene(scenes.tiny_scene())
    d_h = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    h_r, h_h, h_o = np.zeros(4, dtype=_abi.RAY_DTYPE), np.zeros(4, dtype=_abi.HIT_DTYPE), np.zeros(4, dtype=np.uint8)
    L = sc._L
    for fn, who, rays_ptr, out_ptr, tail in (
            (L.prt_trace_closest, "prt_trace_closest", h_r.ctypes.data, h_h.ctypes.data, (0,)),
            (L.prt_trace_closest_device, "prt_trace_closest_device", d_r.data_ptr(), d_h.data_ptr(), (0, None)),
            (L.prt_trace_closest_device_prec, "prt_trace_closest_device", d_r.data_ptr(), d_h.data_ptr(), (0, 0, None)),
            (L.prt_trace_closest_sorted_device, "prt_trace_closest_sorted_device", d_r.data_ptr(), d_h.data_ptr(), (0, 0, None)),
            (L.prt_trace_occluded, "prt_trace_occluded", h_r.ctypes.data, h_o.ctypes.data, (0,)),
            (L.prt_trace_occluded_device, "prt_trace_occluded_device", d_r.data_ptr(), d_o.data_ptr(), (0, 0, None)),
            (L.prt_trace_occluded_sorted_device, "prt_trace_occluded_sorted_device", d_r.data_ptr(), d_o.data_ptr(), (0, 0, None))):
        for args in ((None, 4, out_ptr), (rays_ptr, 4, None)):
            assert fn(sc._h, *args, *tail) == _abi.PRT_E_INVALID, who
            assert L.prt_last_error().decode() == who + ": null buffer"
        assert fn(fresh._h, rays_ptr, 4, out_ptr, *tail) == _abi.PRT_E_NO_DEVICE, who
        assert L.prt_last_error().decode() == who + ": scene is not uploaded to a HIP device (no CPU path exists)"
    fresh.close()
    sc.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_counters_and_the_early_out(gpu, device_bvh):
    data = scenes.cornell_box(ball_subdiv=4, width=256, height=256)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    for prec, m in ((_abi.PRECISION_F64, 1e-6), (_abi.PRECISION_F32, 1e-3)):
        _, upto, _ = _oracle_intervals(data, 30_000, m, seed=41)  # every ray occluded (the second batch of the oracle test)
        n = upto.shape[0]
        for sort in (False, True):
            assert _occluded(sc, upto, precision=prec, sort=sort).all()
            c = sc.counters()
            assert c["rays_shadow"] == n and c["rays_closest"] == 0 and c["samples"] == 0 and c["kernel_ms"] > 0
        assert _occluded(sc, upto, precision=prec, count_work=True).all()
        c_any = sc.counters()
        assert c_any["rays_shadow"] == n and c_any["rays_closest"] == 0 and c_any["tri_tests"] > 0 and c_any["node_fetches"] > 0
        assert (_closest(sc, upto, precision=prec, count_work=True)["prim"] >= 0).all()
        c_cl = sc.counters()
        assert c_cl["rays_closest"] == n and c_cl["rays_shadow"] == 0
        print(f"device_bvh={device_bvh} prec={prec}: node fetches any-hit {c_any['node_fetches']} / closest {c_cl['node_fetches']}, "
              f"triangle tests {c_any['tri_tests']} / {c_cl['tri_tests']}")
        # any-hit can only stop earlier: this, not the equality of answers, shows the early-out is live
        assert c_any["node_fetches"] <= c_cl["node_fetches"]
    sc.close()


@functools.lru_cache(maxsize=None)
def _tiny_intervals(m):
    """A shuffled batch of the three kinds of _oracle_intervals rays on the tiny scene and the oracle's answer per ray;
    an odd number of rays above the pool chunk: a wave refills its pool, and the last pool and the last wave are partial."""
    before, upto, missed = _oracle_intervals(scenes.tiny_scene(), 1500, m, seed=81)
    rays = np.concatenate([before, upto, missed])
    lower = np.concatenate([np.zeros(before.shape[0]), before["tmax"], np.zeros(missed.shape[0])])  # t of a hit lies above it
    want = np.concatenate([np.zeros(before.shape[0], bool), np.ones(upto.shape[0], bool), np.zeros(missed.shape[0], bool)])
    n = rays.shape[0] - (rays.shape[0] % 2 == 0)
    order = np.random.default_rng(83).permutation(rays.shape[0])[:n]
    assert n > 2 * K1_CHUNK and n % 64 and want[order].any() and not want[order].all()
    rays, lower, want = rays[order], lower[order], want[order]
    for a in (rays, lower, want):
        a.setflags(write=False)
    return rays, lower, want


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("prec,m", [(_abi.PRECISION_F64, 1e-6), (_abi.PRECISION_F32, 1e-3)])
def test_counting_kernels_on_padded_records(gpu, dev_lib, monkeypatch, prec, m, device_bvh):
    """The counting instantiations on records padded to one per cache line (a layout only scenes beyond
    PRT_TRI_PADDED_ABOVE get by themselves), closest-hit and any-hit, plain and sorted."""
    monkeypatch.setenv("PRT_TUNE_TRI_STRIDE", "128")
    rays, lower, want = _tiny_intervals(m)
    n = rays.shape[0]
    sc = api.Scene(scenes.tiny_scene(), device_bvh=device_bvh).upload(gpu)
    assert sc.bvh_info()["tri_stride"] == 128
    d_r = _dev(rays.copy())
    for sort in (False, True):
        h = _closest(sc, rays, precision=prec, sort=sort, count_work=True, d_r=d_r)
        c = sc.counters()
        assert c["rays_closest"] == n and c["rays_shadow"] == 0 and c["node_fetches"] > 0 and 0 < c["tri_full"] <= c["tri_tests"]
        bad = int(((h["prim"] >= 0) != want).sum())
        print(f"device_bvh={device_bvh} prec={prec} sort={sort}: {n} rays, {int(want.sum())} hits, mismatches {bad}")
        assert bad == 0
        assert (h["t"][want] > lower[want]).all() and (h["t"][want] <= rays["tmax"][want]).all() and np.isinf(h["t"][~want]).all()
        got = _occluded(sc, rays, precision=prec, sort=sort, count_work=True, d_r=d_r)
        c = sc.counters()
        assert c["rays_shadow"] == n and c["rays_closest"] == 0 and c["node_fetches"] > 0 and c["tri_tests"] > 0
        assert set(np.unique(got)) <= {0, 1} and np.array_equal(got.astype(bool), h["prim"] >= 0)
    sc.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_answers_follow_update_vertices(gpu, device_bvh):
    data = scenes.cornell_box(ball_subdiv=3, width=128, height=128)
    rays = scenes.shadow_segments(data, 60_000, seed=71)
    sc = api.Scene(data, device_bvh=device_bvh).upload(gpu)
    before = _occluded(sc, rays)
    v = np.asarray(data.vertices, dtype=np.float64)
    lo, hi = data.bounds()
    centre = 0.5 * (np.asarray(lo) + np.asarray(hi))
    v2 = centre + (v - centre) * np.array([0.6, 1.0, 0.8])  # the walls move in, the segments' ends now hang in the air
    moved = dataclasses.replace(data, vertices=v2, normals=None)
    sc.update_vertices(v2)
    after = _occluded(sc, rays)
    fresh = api.Scene(moved, device_bvh=device_bvh).upload(gpu)
    want = _occluded(fresh, rays)
    assert np.array_equal(after, want)
    assert np.array_equal(after.astype(bool), _closest(sc, rays)["prim"] >= 0)
    assert (after != before).mean() > 0.01
    assert np.array_equal(_occluded(sc, rays, precision=_abi.PRECISION_F32), _occluded(fresh, rays, precision=_abi.PRECISION_F32))
    sc.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_cpp_occluded_agrees_with_hit(gpu, tmp_path, device_bvh):
    """Hittable::Occluded (one ray, and the batch overload) against Hittable::Hit's return value on main.cpp's world."""
    build.build_host_example()
    exe = str(tmp_path / "occluded_check")
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "occluded_check.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    data = scenes.cornell_box(ball_subdiv=2, width=48, height=40)
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    r = subprocess.run([exe, res, data.name, "400", "1" if device_bvh else "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    n, hits, bad = int(words[1]), int(words[3]), int(words[5])
    assert n == 400 and bad == 0 and 0.1 * n < hits < n
