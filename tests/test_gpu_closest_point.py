"""GPU tests (-m gpu) of the closest-point queries (prt_closest_point, include/prt.h; kernel K6 in closest_point.hip) against
the numpy restatement of the contract (tests/closest_point_model.py).

Tolerance against the model: 1e-12 S, S = max(1, largest |coordinate| of the scene and the queries) - the project's tier-1 hit
tolerance scaled as RefitCheck::scale scales it.  That is ten times the model's own verified error (float64 against
longdouble, tests/test_closest_point_cpu.py) on every scene but `flat` and `walls`: on-surface queries of their sliver
triangles carry up to 1.2e-12 S of the routine's own error, so there the tolerance shows agreement with the contract's
fp64 arithmetic - which the kernel evaluates operation for operation - not closeness to the exact distance.
The model's brute force is computed once per scene and query class and shared by the tests that need it.
"""
import os
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, build, scenes
from tests import bvh_model as M
from tests import closest_point_model as CM
from tests.test_closest_point_cpu import region_queries
from tests.test_gpu_refit import moved, sine, with_vertices

pytestmark = pytest.mark.gpu

BUILDERS = [pytest.param(False, id="host"), pytest.param(True, id="device")]
EPS = float(np.finfo(np.float64).eps)


def upload(data, device_bvh, on=True):
    sc = api.Scene(data, device_bvh=device_bvh)
    if on:
        sc.distance_queries = True
    return sc.upload(0)


def check_records(rec, p, v, ref, where):
    """The five checks of a batch of records against the model's brute force `ref` on vertices `v`."""
    S = CM.scene_scale(v, p)
    tol = 1e-12 * S
    assert np.all(rec["prim"] >= 0) and np.all(rec["prim"] < v.shape[0]) and np.all(rec["reserved"] == 0), where
    # 1. the distance is the model's minimum
    want = np.sqrt(ref["d2"])
    worst = float(np.abs(rec["dist"] - want).max())
    exact = float((rec["dist"] == want).mean())
    assert worst <= tol, (where, worst / S)
    # 2. `point` lies on triangle `prim`, at `dist` from the query
    tri = v[rec["prim"]]
    on = np.sqrt(CM.point_triangle(rec["point"], tri)["d2"])
    assert on.max() <= tol, (where, float(on.max()) / S)
    d = p - rec["point"]
    sep = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    assert np.all(np.abs(sep - rec["dist"]) <= 4 * np.spacing(rec["dist"])), where
    # 3. the reported triangle is (one of) the nearest: near-ties may pick either neighbour, exact ties may not
    own = CM.point_triangle(p, tri)
    assert (np.sqrt(own["d2"]) - want).max() <= tol, where
    tie = own["d2"] == ref["d2"]
    assert np.array_equal(rec["prim"][tie], ref["prim"][tie]), (where, "an exact tie went to the higher index")
    # 4. the barycentrics are a point of the triangle and reproduce `point`
    al, be = rec["alpha"], rec["beta"]
    assert np.all(al >= 0) and np.all(be >= 0) and np.all(al + be <= 1), where
    again = tri[:, 0] + al[:, None] * (tri[:, 1] - tri[:, 0]) + be[:, None] * (tri[:, 2] - tri[:, 0])
    assert np.abs(again - rec["point"]).max() <= 4 * EPS * S, where
    # 5. the feature is consistent with them
    f = rec["feature"]
    assert np.all((f >= 0) & (f <= 6)), where
    corners = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    vert = f >= 4
    assert np.array_equal(np.stack([al, be], 1)[vert], corners[f[vert] - 4]), where
    assert np.all(be[f == 1] == 0) and np.all(al[f == 3] == 0) and np.array_equal(al[f == 2], 1.0 - be[f == 2]), where
    assert np.all(np.isin(rec["side"], (-1, 0, 1))), where
    return worst / S, exact


_records = {}


def records(name, device_bvh):
    """The GPU's records for the three query classes of a scene, per builder: computed once, shared, not modified."""
    if (name, device_bvh) not in _records:
        sc = upload(CM.scene(name), device_bvh)
        _records[(name, device_bvh)] = {cls: sc.closest_point(CM.scene_queries(name)[cls][0]) for cls in CM.CLASSES}
        sc.close()
    return _records[(name, device_bvh)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", CM.SCENE_NAMES)
def test_brute_force(gpu, name, device_bvh):
    v = CM.scene(name).vertices
    for cls in CM.CLASSES:
        p = CM.scene_queries(name)[cls][0]
        worst, exact = check_records(records(name, device_bvh)[cls], p, v, CM.reference(name, cls), (name, cls))
        print(f"{name} {cls}: |dist - model| <= {worst:.2e} S, bit-equal to the model on {100 * exact:.2f} % of {p.shape[0]}")


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_one_triangle_seven_regions(gpu, device_bvh):
    """_TRI and a far copy of it (the device builder wants two triangles): queries well inside each Voronoi region of the
    first, on both sides."""
    tris = np.stack([M._TRI, M._TRI + np.array([50.0, 50.0, 50.0])])
    sc = upload(M._scene("regions", tris), device_bvh)
    p, want = region_queries(M._TRI)
    rec = sc.closest_point(p)
    m = CM.point_triangle(p, np.broadcast_to(M._TRI, (p.shape[0], 3, 3)))
    assert np.array_equal(m["feature"], want["feature"]) and np.array_equal(m["side"], want["side"])
    assert np.array_equal(rec["prim"], np.zeros(p.shape[0], np.int32))
    assert np.array_equal(rec["feature"], m["feature"]) and np.array_equal(rec["side"], m["side"])
    assert sorted(set(rec["feature"].tolist())) == list(range(7))
    sc.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", CM.SCENE_NAMES)
def test_tree_independence_bit_for_bit(gpu, name):
    """A host-built tree, a device-built tree and the same scene after rebuild() with unchanged vertices: the same bytes."""
    data = CM.scene(name)
    q = CM.scene_queries(name)
    sc = upload(data, False)
    sc.rebuild(np.ascontiguousarray(data.vertices))
    assert sc.bvh_info()["built_on_device"] == 1
    for cls in CM.CLASSES:
        a, b = records(name, False)[cls], records(name, True)[cls]
        c = sc.closest_point(q[cls][0])
        assert a.tobytes() == b.tobytes(), (name, cls, "host-built against device-built")
        assert a.tobytes() == c.tobytes(), (name, cls, "after rebuild")
        if name == "identical":
            assert np.all(a["prim"] == 0)
    sc.close()


# ------------------------------------------------------------------------------------------------ 4
def _device_call(fn, v):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    torch.cuda.synchronize()
    fn(d.data_ptr())
    torch.cuda.synchronize()


MOTIONS = {
    "refit": lambda sc, v: sc.refit(v),
    "refit_device": lambda sc, v: _device_call(sc.refit_device, v),
    "rebuild": lambda sc, v: sc.rebuild(v),
    "rebuild_device": lambda sc, v: _device_call(sc.rebuild_device, v),
    "update_vertices": lambda sc, v: sc.update_vertices(v),
}


@pytest.mark.parametrize("how", list(MOTIONS))
@pytest.mark.parametrize("name,device_bvh", [("cornell", False), ("triangle_soup", True)])
def test_geometry_follows(gpu, name, device_bvh, how):
    """Every triangle that may move (emitters stay put) displaced sinusoidally by 10 % of the extent: after each way of
    moving the resident geometry the records are those of a fresh scene made from the new vertices, and the model's."""
    data = CM.scene(name)
    v = np.ascontiguousarray(moved(data, sine))
    q = CM.scene_queries(name)
    sc = upload(data, device_bvh)
    MOTIONS[how](sc, v)
    assert sc.distance_queries is True
    fresh = upload(with_vertices(data, v), device_bvh)
    for cls in CM.CLASSES:
        p = q[cls][0]
        rec = sc.closest_point(p)
        assert rec.tobytes() == fresh.closest_point(p).tobytes(), (name, how, cls)
        check_records(rec, p, v, CM.reference(name, cls, v, "sine"), (name, how, cls))
    sc.close()
    fresh.close()


def test_switching_on_after_refit_device_is_refused(gpu):
    data = CM.scene("cornell")
    v = np.ascontiguousarray(moved(data, sine))
    sc = upload(data, False, on=False)
    _device_call(sc.refit_device, v)
    with pytest.raises(api.PrtError) as e:
        sc.distance_queries = True
    msg = str(e.value)
    assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_distance_queries" in msg
    assert "before moving geometry" in msg and "prt_scene_refit" in msg and "prt_scene_update_vertices" in msg
    assert sc.distance_queries is False
    sc.refit(v)  # every host position replaced: the host copy is current again
    sc.distance_queries = True
    p = CM.scene_queries("cornell")["near"][0]
    fresh = upload(with_vertices(data, v), False)
    assert sc.closest_point(p).tobytes() == fresh.closest_point(p).tobytes()
    sc.close()
    fresh.close()
    # switching on BEFORE the device refit is accepted (test_geometry_follows goes on from there)
    sc = upload(data, False)
    _device_call(sc.refit_device, v)
    assert sc.distance_queries is True
    sc.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_radius(gpu, device_bvh):
    name = "cornell"
    data = CM.scene(name)
    v = data.vertices
    p = CM.scene_queries(name)["near"][0]
    full = records(name, device_bvh)["near"]
    sc = upload(data, device_bvh)
    d = full["dist"]
    assert sc.closest_point(p, max_dist=d * (1 + 1e-6)).tobytes() == full.tobytes()
    pos = d > 0
    less = sc.closest_point(p[pos], max_dist=d[pos] * (1 - 1e-6))
    miss = less["prim"] < 0
    assert np.all(less["dist"][~miss] > d[pos][~miss]) and np.all(less["prim"][~miss] != full["prim"][pos][~miss])
    assert np.all(np.isinf(less["dist"][miss])) and np.all(less["feature"][miss] == -1) and np.all(less["side"][miss] == 0)
    for k in ("point", "alpha", "beta", "reserved"):
        assert not np.any(less[k][miss]), k
    assert miss.any()
    # max_dist = 0 on a query that IS a mesh vertex hits it (a triangle's v0: there alpha = beta = 0 and `point` is the
    # corner itself, d2 == 0 exactly; the contract's point = v0 + 1 (v1 - v0) need not round back to v1)
    corners = np.ascontiguousarray(v[::7, 0])
    at = sc.closest_point(corners, max_dist=0.0)
    assert np.all(at["prim"] >= 0) and np.all(at["dist"] == 0) and np.array_equal(at["point"], corners)
    # unbounded, 1e3 extents outside the bounds
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(256, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    far = 0.5 * (lo + hi) + dirs * 1e3 * float((hi - lo).max())
    rec = sc.closest_point(far)
    check_records(rec, far, v, CM.brute_force(far, v), (name, "far"))
    sc.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257])
def test_exactly_n_records_are_written(gpu, n):
    import torch
    name = "mixed_materials"
    sc = upload(CM.scene(name), False)
    p = CM.scene_queries(name)["near"][0][:n]
    q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
    q["p"], q["max_dist"] = p, np.inf
    d_q = torch.from_numpy(np.frombuffer(q.tobytes() + b"\0" * 32, dtype=np.uint8).copy()).cuda()
    d_out = torch.full(((n + 2) * 64,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sc.closest_point_device(d_q.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert np.all(raw[n * 64:] == 0xAA), "bytes beyond the n records were written"
    rec = raw[:n * 64].view(_abi.CLOSEST_POINT_DTYPE)
    assert rec.tobytes() == sc.closest_point(np.ascontiguousarray(p)).tobytes()
    assert np.all(rec["reserved"] == 0) and np.all(rec["prim"] >= 0)
    c = sc.counters()
    assert c["rays_closest"] == 0 and c["rays_shadow"] == 0 and c["samples"] == 0
    sc.close()


def test_refusals_on_the_device(gpu):
    import torch
    sc = upload(CM.scene("mixed_materials"), False)
    d_q = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    d_out = torch.full((66 * 64,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for off in (8, 16):
        with pytest.raises(api.PrtError) as e:
            sc.closest_point_device(d_q.data_ptr(), 64, d_out.data_ptr() + off)
        assert e.value.code == _abi.PRT_E_INVALID and "32-byte aligned" in str(e.value)
    for args in ((None, 4, d_out.data_ptr()), (d_q.data_ptr(), 4, None), (d_q.data_ptr(), 1 << 32, d_out.data_ptr())):
        with pytest.raises(api.PrtError) as e:
            sc.closest_point_device(*args)
        assert e.value.code == _abi.PRT_E_INVALID and "prt_closest_point_device" in str(e.value)
    sc.distance_queries = False
    for call in (lambda: sc.closest_point(np.zeros((4, 3))), lambda: sc.closest_point_device(d_q.data_ptr(), 4, d_out.data_ptr())):
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_INVALID and "prt_closest_point" in str(e.value) and "prt_scene_set_distance_queries" in str(e.value)
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == 0xAA)
    sc.distance_queries = True  # and on again, on the uploaded scene: the table is rebuilt from the host triangles
    p = CM.scene_queries("mixed_materials")["box"][0]
    assert sc.closest_point(p).tobytes() == records("mixed_materials", False)["box"].tobytes()
    sc.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_it_prunes(gpu, device_bvh):
    """On-surface queries in a soup of 0.01-extent triangles in a unit cube: once d2 ~ 0 is found, a strict-cull descent
    opens only the boxes that contain the point.  Conditions, not measurements: a scan of the leaves cannot meet them."""
    name = "triangle_soup"
    sc = upload(CM.scene(name), device_bvh)
    p = CM.scene_queries(name)["surface"][0]
    rec = sc.closest_point(p, count_work=True)
    c = sc.counters()
    n_tris, n_nodes = CM.scene(name).n_tris, sc.bvh_info()["n_nodes"]
    tests, fetches = c["tri_tests"] / p.shape[0], c["node_fetches"] / p.shape[0]
    print(f"{name}: {tests:.2f} triangle tests and {fetches:.2f} node fetches per query ({n_tris} triangles, {n_nodes} nodes); "
          f"{c['inner_rounds'] / p.shape[0]:.2f} inner and {c['leaf_rounds'] / p.shape[0]:.2f} leaf entries per query dropped at the pop; "
          f"{c['kernel_ms']:.3f} ms")
    assert rec.tobytes() == records(name, device_bvh)["surface"].tobytes()  # the counting instantiation answers alike
    assert c["rays_closest"] == 0 and c["rays_shadow"] == 0 and c["samples"] == 0 and c["kernel_ms"] > 0
    assert 0 < tests < n_tris / 8 and 0 < fetches < n_nodes / 4
    sc.close()


def test_schedules_agree(gpu, dev_lib, monkeypatch):
    """The kernel's plain instantiation (one lane per query, no refill of finished lanes; developer hook of the dev-hooks
    build) writes the bytes the shipped schedule writes: a record does not depend on which lane answered it, or when.
    Both sets of records are made here, by the dev-hooks library: without the variable it launches the shipped schedule."""
    monkeypatch.delenv("PRT_TUNE_CLOSEST_PLAIN", raising=False)
    for name in ("cornell", "soup_at_1e6"):
        sc = upload(CM.scene(name), False)
        q = CM.scene_queries(name)
        refill = {cls: sc.closest_point(q[cls][0]) for cls in CM.CLASSES}
        counted = sc.closest_point(q["box"][0], count_work=True)
        work = sc.counters()
        monkeypatch.setenv("PRT_TUNE_CLOSEST_PLAIN", "1")
        for cls in CM.CLASSES:
            assert sc.closest_point(q[cls][0]).tobytes() == refill[cls].tobytes(), (name, cls)
        # the counting instantiations too, and the same descents query for query: the work counters agree
        assert sc.closest_point(q["box"][0], count_work=True).tobytes() == counted.tobytes() == refill["box"].tobytes()
        again = sc.counters()
        assert (again["node_fetches"], again["tri_tests"]) == (work["node_fetches"], work["tri_tests"]) and work["tri_tests"] > 0
        monkeypatch.delenv("PRT_TUNE_CLOSEST_PLAIN")
        assert refill["box"].tobytes() == records(name, False)["box"].tobytes()  # ... and the shipped library's
        sc.close()


# ------------------------------------------------------------------------------------------------ 8
def test_nothing_else_moved(gpu):
    """A frame and a closest-hit batch before switching on, after switching on and querying, and after switching off."""
    data = CM.scene("cornell")
    rays = scenes.random_rays(4096, (-1, -1, -1), (1, 1, 1))
    sc = upload(data, False, on=False)
    frame = lambda: sc.render(spp=4, max_depth=5, seed=9)  # noqa: E731
    states = [(frame().tobytes(), sc.trace_closest(rays).tobytes())]
    sc.distance_queries = True
    for cls in CM.CLASSES:
        sc.closest_point(CM.scene_queries("cornell")[cls][0], count_work=(cls == "box"))
    states.append((frame().tobytes(), sc.trace_closest(rays).tobytes()))
    sc.distance_queries = False
    states.append((frame().tobytes(), sc.trace_closest(rays).tobytes()))
    assert states[0] == states[1] == states[2]
    assert (data.camera.width, data.camera.height) == (64, 64)
    sc.close()


# ------------------------------------------------------------------------------------------------ 9
def test_cpp_closest_point_equals_the_binding(gpu, tmp_path):
    """Hittable::ClosestPoint, one point at a time and as a batch, on main.cpp's world against Scene.closest_point."""
    build.build_host_example()
    exe = str(tmp_path / "closest_point_check")
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "closest_point_check.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    data = scenes.cornell_box(ball_subdiv=2, width=48, height=40)
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    fixed = scenes.apply_loader_uv_fixup(data)
    q = CM.queries(fixed.vertices, 128, 21)
    p = np.ascontiguousarray(np.concatenate([q["near"][0], q["box"][0]]))
    assert p.shape == (256, 3)
    p.tofile(str(tmp_path / "points.f64"))
    sc = upload(fixed, False)
    for radius in (np.inf, 0.05):
        out = str(tmp_path / "out.f64")
        r = subprocess.run([exe, res, data.name, str(tmp_path / "points.f64"), repr(float(radius)), out], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, dtype=np.float64).reshape(256, 2, 5)
        rec = sc.closest_point(p, max_dist=radius)
        found = rec["prim"] >= 0
        want = np.where(found[:, None], np.concatenate([np.ones((256, 1)), rec["dist"][:, None], rec["point"]], axis=1), 0.0)
        assert np.array_equal(got[:, 0], want), "batch overload"
        assert np.array_equal(got[:, 1], want), "single-point overload"
        assert found.any() and (np.isinf(radius) or not found.all())
    sc.close()
