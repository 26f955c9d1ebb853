"""GPU tests (-m gpu) of the signed distance queries (prt_signed_distance, include/prt.h; pseudonormals.hip, the SIGNED
instantiations of K6 in closest_point.hip) against the numpy model (tests/signed_distance_model.py).

Pseudonormals are held to (valence + 16) 2^-50 sum|weights| per component (derived at signed_distance_model.per_triangle); the
sign is then checked bit for bit on EVERY query from the device's own record and the device's own pseudonormals, so no
tolerance enters it.  The device's records and pseudonormals are computed once per scene and builder and shared.
"""
import os
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, build, scenes
from tests import bvh_model as M
from tests import closest_point_model as CM
from tests import signed_distance_model as SM
from tests.test_gpu_refit import with_vertices
from tests.test_signed_distance_cpu import ball_alone

pytestmark = pytest.mark.gpu

BUILDERS = [pytest.param(False, id="host"), pytest.param(True, id="device")]
SCENES = ("tetrahedron", "notched_pyramid", "cornell", "mixed_materials", "walls", "identical", "soup_at_1e6")
CLOSED = ("tetrahedron", "notched_pyramid", "cornell_ball")
_cache = {}


def scene(name):
    if ("scene", name) not in _cache:
        make = {"tetrahedron": SM.tetrahedron, "notched_pyramid": SM.notched_pyramid, "cornell_ball": ball_alone}.get(name)
        _cache[("scene", name)] = make() if make else CM.scene(name)
    return _cache[("scene", name)]


def queries(name):
    """The three query classes of closest_point_model.queries: the shared ones of its scenes, a fixed seed for the others."""
    if name in CM.SCENE_NAMES:
        return {cls: CM.scene_queries(name)[cls][0] for cls in CM.CLASSES}
    if ("queries", name) not in _cache:
        q = CM.queries(scene(name).vertices, 4096, 2000 + len(name))
        _cache[("queries", name)] = {cls: q[cls][0] for cls in CM.CLASSES}
    return _cache[("queries", name)]


def upload(data, device_bvh, on=True):
    sc = api.Scene(data, device_bvh=device_bvh)
    if on:
        sc.signed_queries = True
    return sc.upload(0)


def state(name, device_bvh):
    """Per scene and builder: the device's pseudonormals, its signed records and its closest-point records per class."""
    if ("state", name, device_bvh) not in _cache:
        sc = upload(scene(name), device_bvh)
        q = queries(name)
        _cache[("state", name, device_bvh)] = {"P": sc.pseudonormals(), "info": sc.topology_info(),
                                               "signed": {cls: sc.signed_distance(q[cls]) for cls in CM.CLASSES},
                                               "closest": {cls: sc.closest_point(q[cls]) for cls in CM.CLASSES}}
        sc.close()
    return _cache[("state", name, device_bvh)]


def model(name):
    if ("model", name) not in _cache:
        _cache[("model", name)] = SM.per_triangle(SM.pseudonormals(scene(name).vertices))
    return _cache[("model", name)]


def check_contract(signed, closest, p, v, P, where):
    """Contract items 1 and 2 on a batch: every byte but sdist / sign is closest_point's, |sdist| is its dist bit for bit, and
    sign / sdist follow from the device's own record and pseudonormals - every query, no exclusions."""
    a, b = signed.view(_abi.CLOSEST_POINT_DTYPE), closest
    for f in ("point", "alpha", "beta", "prim", "feature", "side"):
        assert a[f].tobytes() == b[f].tobytes(), (where, f)
    assert np.abs(signed["sdist"]).tobytes() == closest["dist"].tobytes(), where
    assert np.all(closest["reserved"] == 0), where
    want = SM.sign_of_records(p, signed["point"], signed["prim"], signed["feature"], v, P)
    assert np.array_equal(signed["sign"], want), (where, int((signed["sign"] != want).sum()))
    face = signed["feature"] == 0
    assert np.array_equal(signed["sign"][face], signed["side"][face]), where
    assert np.array_equal(signed["sdist"], np.where(want < 0, -closest["dist"], closest["dist"])), where
    miss = signed["prim"] < 0
    assert np.all(signed["sign"][miss] == 0) and np.all(signed["sdist"][miss] == np.inf), where


# ------------------------------------------------------------------------------------------------ pseudonormals
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", SCENES)
def test_pseudonormals_agree_with_the_model(gpu, name, device_bvh):
    got = state(name, device_bvh)["P"]
    want, tol = model(name)
    err = np.abs(got - want)
    worst = float((err / np.maximum(tol, 1e-300)[:, :, None]).max())
    print(f"{name}: worst |device - model| = {float(err.max()):.3e}, {worst:.3f} of its tolerance")
    assert np.all(err <= tol[:, :, None]), (name, worst)
    assert np.all(got[tol == 0] == 0)  # a slot without an id, or one no face contributes to
    assert state(name, False)["P"].tobytes() == state(name, True)["P"].tobytes(), "host-built against device-built tree"
    info = state(name, device_bvh)["info"]
    assert info["table_bytes"] > 0
    assert {k: x for k, x in info.items() if k != "table_bytes"} == SM.topology(scene(name).vertices)["info"]


# ------------------------------------------------------------------------------------------------ contract items 1, 2, 4
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", SCENES)
def test_sign_bit_for_bit(gpu, name, device_bvh):
    st, v = state(name, device_bvh), scene(name).vertices
    for cls in CM.CLASSES:
        check_contract(st["signed"][cls], st["closest"][cls], queries(name)[cls], v, st["P"], (name, cls))
        assert st["signed"][cls].tobytes() == state(name, not device_bvh)["signed"][cls].tobytes(), (name, cls, "the two builders")
    used = np.concatenate([st["signed"][cls]["feature"] for cls in CM.CLASSES])
    assert (used > 0).any() or name == "identical"


def test_miss_records_under_a_finite_radius(gpu):
    name = "notched_pyramid"
    sc = upload(scene(name), False)
    p = queries(name)["box"]
    d = state(name, False)["closest"]["box"]["dist"]
    radius = float(np.median(d))
    signed, closest = sc.signed_distance(p, max_dist=radius), sc.closest_point(p, max_dist=radius)
    miss = signed["prim"] < 0
    assert miss.any() and not miss.all() and np.array_equal(miss, d > radius)
    check_contract(signed, closest, p, scene(name).vertices, state(name, False)["P"], (name, "radius"))
    for f in ("point", "alpha", "beta", "side", "sign"):
        assert not np.any(signed[f][miss]), f
    assert np.all(signed["feature"][miss] == -1)
    assert signed[~miss].tobytes() == state(name, False)["signed"]["box"][~miss].tobytes()
    sc.close()


# ------------------------------------------------------------------------------------------------ contract item 3
@pytest.mark.parametrize("name", CLOSED)
def test_sign_is_inside_outside_on_closed_shapes(gpu, name):
    v = scene(name).vertices
    assert SM.topology(v)["info"]["closed"] == 1
    ext = float((v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)).max())
    batches = {"box": SM.box_queries(v)}
    if name == "notched_pyramid":
        batches["apex"] = SM.apex_queries()
    sc = upload(scene(name), True)
    for tag, p in batches.items():
        rec = sc.signed_distance(p)
        truth = SM.tetrahedron_inside(p) if name == "tetrahedron" else SM.inside_truth(p, v)
        far = np.abs(rec["sdist"]) > 1e-6 * ext
        wrong = int((rec["sign"][far] != truth[far]).sum())
        wrong_side = int((rec["side"][far] != truth[far]).sum())
        print(f"{name} {tag}: sign wrong on {wrong}, `side` on {wrong_side} of {int(far.sum())} ({int((truth == -1).sum())} inside)")
        assert far.sum() > 4000 and (truth == -1).sum() > 50
        assert wrong == 0
        assert np.array_equal(rec["sdist"][far] < 0, truth[far] < 0)
        if (name, tag) in (("tetrahedron", "box"), ("notched_pyramid", "apex")):
            assert wrong_side > 0  # what the plane-side sign gets wrong is in the batch
    sc.close()


# ------------------------------------------------------------------------------------------------ independence
def test_batch_order_split_and_counting_do_not_matter(gpu):
    name = "notched_pyramid"
    p = np.ascontiguousarray(np.concatenate([queries(name)["near"], SM.apex_queries(1024)]))
    sc = upload(scene(name), False)
    base = sc.signed_distance(p)
    perm = np.random.default_rng(5).permutation(p.shape[0])
    assert sc.signed_distance(np.ascontiguousarray(p[perm])).tobytes() == base[perm].tobytes()
    cut = 1000
    parts = np.concatenate([sc.signed_distance(np.ascontiguousarray(p[:cut])), sc.signed_distance(np.ascontiguousarray(p[cut:]))])
    assert parts.tobytes() == base.tobytes()
    counted = sc.signed_distance(p, count_work=True)
    c = sc.counters()
    assert counted.tobytes() == base.tobytes() and c["tri_tests"] > 0 and c["rays_closest"] == 0 and c["samples"] == 0
    sc.close()
    other = upload(scene(name), True)
    assert other.signed_distance(p).tobytes() == base.tobytes()
    other.close()


@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_exactly_n_records_are_written(gpu, n):
    import torch
    name = "tetrahedron"
    sc = upload(scene(name), False)
    p = np.ascontiguousarray(queries(name)["near"][:n])
    q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
    q["p"], q["max_dist"] = p, np.inf
    d_q = torch.from_numpy(np.frombuffer(q.tobytes() + b"\0" * 32, dtype=np.uint8).copy()).cuda()
    d_out = torch.full(((n + 2) * 64,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sc.signed_distance_device(d_q.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert np.all(raw[n * 64:] == 0xAA), "bytes beyond the n records were written"
    assert raw[:n * 64].tobytes() == sc.signed_distance(p).tobytes()
    with pytest.raises(api.PrtError) as e:
        sc.signed_distance_device(d_q.data_ptr(), 1, d_out.data_ptr() + 8)
    assert e.value.code == _abi.PRT_E_INVALID and "32-byte aligned" in str(e.value) and "prt_signed_distance_device" in str(e.value)
    sc.close()


# ------------------------------------------------------------------------------------------------ moving geometry
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
}


def wobble(v0):
    """A smooth deformation that is a pure function of position (its constants come from the undeformed shape), so that
    welded corners stay welded."""
    p = v0.reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    return np.ascontiguousarray(v0 + 0.05 * ext * np.sin((3.0 / ext) * v0[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3])))


@pytest.mark.parametrize("how", list(MOTIONS))
@pytest.mark.parametrize("name,device_bvh", [("cornell_ball", False), ("notched_pyramid", True)])
def test_geometry_follows(gpu, name, device_bvh, how):
    data = scene(name)
    v = wobble(data.vertices)
    assert SM.topology(v)["info"] == SM.topology(data.vertices)["info"]  # the welds survived
    p = np.ascontiguousarray(np.concatenate([queries(name)["near"][:2048], queries(name)["box"][:2048]]))
    sc = upload(data, device_bvh)
    before = sc.refit_info()["refits"]
    MOTIONS[how](sc, v)
    assert sc.signed_queries is True and sc.distance_queries is True
    if how.startswith("refit"):
        assert sc.refit_info()["refits"] == before + 1
    assert sc.refit_info()["host_stale"] == (1 if how.endswith("_device") else 0)
    if ("fresh", name) not in _cache:
        fresh = upload(with_vertices(data, v), device_bvh)
        _cache[("fresh", name)] = (fresh.pseudonormals(), fresh.signed_distance(p))
        fresh.close()
    P, rec = _cache[("fresh", name)]
    assert sc.pseudonormals().tobytes() == P.tobytes(), (name, how)
    got = sc.signed_distance(p)
    assert got.tobytes() == rec.tobytes(), (name, how)
    check_contract(got, sc.closest_point(p), p, v, P, (name, how))
    if how == "refit":  # a refused refit leaves the tables and the records as they were
        bad = v.copy()
        bad[3, 1, 2] = np.nan
        with pytest.raises(api.PrtError):
            sc.refit(bad)
        assert sc.pseudonormals().tobytes() == P.tobytes() and sc.signed_distance(p).tobytes() == rec.tobytes()
    sc.close()


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_life_cycle(gpu):
    name = "tetrahedron"
    data, p = scene(name), queries(name)["box"]
    want = state(name, False)
    sc = upload(data, False, on=False)  # on after the upload
    assert sc.topology_info()["table_bytes"] == 0
    sc.signed_queries = True
    assert sc.distance_queries is True
    # 4 triangles, 4 vertices, 6 edges: ids 4 x 6, lists (5 + 12) + (7 + 12) words; reals 4 x 6 + 10 x 3
    assert sc.topology_info()["table_bytes"] == 4 * (24 + 17 + 19) + 8 * (24 + 30)
    assert sc.pseudonormals().tobytes() == want["P"].tobytes() and sc.signed_distance(p).tobytes() == want["signed"]["box"].tobytes()
    with pytest.raises(api.PrtError) as e:
        sc.distance_queries = False
    assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_signed_queries" in str(e.value)
    sc.signed_queries = False  # off: the tables go, distance queries stay
    assert sc.topology_info()["table_bytes"] == 0 and sc.distance_queries is True
    for call in (lambda: sc.signed_distance(p), sc.pseudonormals):
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_signed_queries" in str(e.value)
    assert sc.closest_point(p).tobytes() == want["closest"]["box"].tobytes()
    sc.signed_queries = True  # survives update_vertices, which welds again
    v = wobble(data.vertices)
    sc.update_vertices(v)
    assert sc.signed_queries is True and sc.topology_info()["table_bytes"] > 0
    fresh = upload(with_vertices(data, v), True)
    assert sc.pseudonormals().tobytes() == fresh.pseudonormals().tobytes()
    assert sc.signed_distance(p).tobytes() == fresh.signed_distance(p).tobytes()
    fresh.close()
    sc.close()


def test_switching_on_while_the_host_geometry_is_stale_is_refused(gpu):
    data = scene("notched_pyramid")
    v = wobble(data.vertices)
    sc = upload(data, False, on=False)
    _device_call(sc.refit_device, v)
    assert sc.refit_info()["host_stale"] == 1
    with pytest.raises(api.PrtError) as e:
        sc.signed_queries = True
    msg = str(e.value)
    assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_signed_queries" in msg
    assert "before moving geometry" in msg and "prt_scene_refit" in msg and "prt_scene_update_vertices" in msg
    assert sc.signed_queries is False and sc.distance_queries is False
    with pytest.raises(api.PrtError) as e:
        sc.topology_info()
    assert e.value.code == _abi.PRT_E_INVALID
    sc.refit(v)  # every host position replaced
    sc.signed_queries = True
    fresh = upload(with_vertices(data, v), False)
    assert sc.pseudonormals().tobytes() == fresh.pseudonormals().tobytes()
    fresh.close()
    sc.close()


def test_closest_point_is_unchanged_by_the_switch(gpu):
    name = "cornell"
    sc = api.Scene(scene(name))
    sc.distance_queries = True
    sc.upload(0)
    q = queries(name)
    before = {cls: sc.closest_point(q[cls]) for cls in CM.CLASSES}
    sc.signed_queries = True
    for cls in CM.CLASSES:
        after = sc.closest_point(q[cls])
        assert after.tobytes() == before[cls].tobytes() and np.all(after["reserved"] == 0), cls
        assert before[cls].tobytes() == state(name, False)["closest"][cls].tobytes()
    sc.close()


# ------------------------------------------------------------------------------------------------ C++
def test_cpp_signed_distance_equals_the_binding(gpu, tmp_path):
    """Hittable::SignedDistance on the tetrahedron, loaded as main.cpp loads a model, against Scene.signed_distance."""
    build.build_host_example()
    exe = str(tmp_path / "signed_distance_check")
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "signed_distance_check.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    data = scene("tetrahedron")
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    p = np.ascontiguousarray(queries("tetrahedron")["box"][:256])
    p.tofile(str(tmp_path / "points.f64"))
    sc = upload(scenes.apply_loader_uv_fixup(data), False)
    for radius in (np.inf, 0.3):
        out = str(tmp_path / "out.f64")
        r = subprocess.run([exe, res, data.name, str(tmp_path / "points.f64"), repr(float(radius)), out], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, dtype=np.float64).reshape(256, 5)
        rec = sc.signed_distance(p, max_dist=radius)
        found = rec["prim"] >= 0
        want = np.where(found[:, None], np.concatenate([np.ones((256, 1)), rec["sdist"][:, None], rec["point"]], axis=1), 0.0)
        assert np.array_equal(got, want)
        assert found.any() and (rec["sdist"][found] < 0).any() and (np.isinf(radius) or not found.all())
    sc.close()
