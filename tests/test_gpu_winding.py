"""GPU tests (-m gpu) of the winding-number queries (prt_winding_number, include/prt.h; winding_number.hip) against the
numpy model (tests/winding_model.py) on the tree the device holds (PRT_TEST_DUMP_BVH of the dev-hooks library).

  a) the moments hook against the model's table, per slot to 1e-12 (1 + scale), scale = max|c| + r + sqrt(A) of the slot
     (winding_model.moment_scale), for both builders and a scene translated by 1e6;
  b) the kernel against the model's walk on the DEVICE's own table, so that every far decision is the same comparison on
     the same bits: values within 1e-10, the four work counters equal as integers.  The batch is made of the candidate
     queries all of whose terms the model finds above 1e-7 (in units of 4 pi): a dropped or doubled term cannot hide
     under the bound.  The kernel adds a query's terms one after the other in fp64: with at most a few hundred terms whose
     absolute sum is a few units, its rounding stays below 1e-12;
  c) beta = inf against the brute-force sum, within 1e-10 (scenes whose |w| stays of order 1: the bound is absolute);
  d) batch sizes 0, 1, 257 and 2^17; the large batch shuffled and split, count_work on and off, host and device call: bit
     for bit;
  e) refit_device and rebuild_device of a deformed mesh: table and values follow the new tree and the new vertices; the
     switch before and after the upload; update_vertices keeps it;
  f) closest_point and signed_distance records do not change with the switch.
  g) Hittable::WindingNumber (tests/cpp/winding_check.cpp): beta = inf against brute force, the default beta's inside / outside.
"""
import contextlib
import os

import numpy as np
import pytest

from pooraytracer_amd import _abi, api
from tests import bvh_model as M
from tests import closest_point_model as CM
from tests import signed_distance_model as SM
from tests import winding_model as W
from tests.test_gpu_refit import with_vertices
from tests.test_signed_distance_cpu import ball_alone

pytestmark = pytest.mark.gpu

BUILDERS = [pytest.param(False, id="host"), pytest.param(True, id="device")]
SCENES = {
    "tetrahedron": SM.tetrahedron,
    "notched_pyramid": SM.notched_pyramid,
    "cornell_ball": lambda: ball_alone(CM.scene("cornell")),
    "open_sphere": W.open_sphere,
    "open_box": W.open_box,
    "cornell": lambda: CM.scene("cornell"),
    "mixed_sizes": M.mixed_sizes,
    "soup_at_1e6": lambda: M.translated(M.soup(4096)),
}
MOMENT_SCENES = ("tetrahedron", "notched_pyramid", "open_sphere", "cornell", "mixed_sizes", "soup_at_1e6")
WALK_SCENES = ("notched_pyramid", "cornell_ball", "open_sphere", "open_box", "cornell")
_cache = {}


def scene(name):
    if ("scene", name) not in _cache:
        _cache[("scene", name)] = SCENES[name]()
    return _cache[("scene", name)]


def points(name):
    if ("points", name) not in _cache:
        _cache[("points", name)] = W.box_queries(scene(name).vertices)
    return _cache[("points", name)]


@contextlib.contextmanager
def dumping(path):
    """Inside: scenes come from the dev-hooks library, and every upload, refit and rebuild writes its tree to `path`."""
    saved = os.environ.get("PRT_TEST_DUMP_BVH")
    os.environ["PRT_TEST_DUMP_BVH"] = path
    try:
        with api.dev_hooks():
            yield
    finally:
        if saved is None:
            del os.environ["PRT_TEST_DUMP_BVH"]
        else:
            os.environ["PRT_TEST_DUMP_BVH"] = saved


def state(name, device_bvh, tmp):
    """Per scene and builder, made once: the device's tree and table, the model's table, the candidate queries' model walk
    on the device's table at beta = 2 and the device's values for all of them at beta = 2 and beta = inf."""
    key = ("state", name, device_bvh)
    if key not in _cache:
        data = scene(name)
        path = str(tmp / f"{name}-{int(device_bvh)}.bin")
        with dumping(path):
            sc = api.Scene(data, device_bvh=device_bvh)
            sc.winding_queries = True
            sc.upload(0)
        tree = M.read_dump(path)
        M.check_tree(tree, data.vertices, sc.bvh_info())
        table = sc.winding_moments()
        p = points(name)
        st = {"tree": tree, "table": table, "model_table": W.moments(tree, data.vertices)}
        st["walk"] = w = W.walk(tree, data.vertices, p, 2.0, table)
        st["w2"], st["winf"] = sc.winding_number(p, 2.0), sc.winding_number(p, np.inf)
        # the batch of test b): the candidates all of whose terms the model finds above 1e-7 (in units of 4 pi)
        smallest = np.full(p.shape[0], np.inf)
        np.minimum.at(smallest, w.terms[0], np.abs(w.terms[1]) / W.FOUR_PI)
        st["keep"] = smallest > 1e-7
        st["counted"] = sc.winding_number(np.ascontiguousarray(p[st["keep"]]), 2.0, count_work=True)
        st["counters"] = sc.counters()
        sc.close()
        _cache[key] = st
    return _cache[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("winding")


def check_table(got, tree, vertices, where):
    want = W.moments(tree, vertices)
    assert got.shape == want.shape == (tree.n_nodes, 4, 8), where
    tol = 1e-12 * (1.0 + W.moment_scale(tree, want))
    err = np.abs(got - want).max(axis=-1)
    print(f"{where}: {tree.n_nodes} nodes, worst |device - model| = {float(err.max()):.3e}, {float((err / tol).max()):.3e} of its tolerance; "
          f"{int((got != want).sum())} of {got.size} values differ at all")
    assert (err <= tol).all(), where
    assert not got[tree.nodes["ref"] == M.UNUSED].any(), where


# ------------------------------------------------------------------------------------------------ a) the table
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", MOMENT_SCENES)
def test_moments_agree_with_the_model(gpu, tmp, name, device_bvh):
    st = state(name, device_bvh, tmp)
    assert st["tree"].built_on_device == int(device_bvh)
    check_table(st["table"], st["tree"], scene(name).vertices, (name, device_bvh))
    assert st["table"][:, :, 7].max() > 0.0


# ------------------------------------------------------------------------------------------------ b) the walk
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", WALK_SCENES)
def test_kernel_takes_the_models_walk(gpu, tmp, name, device_bvh):
    st, p, w = state(name, device_bvh, tmp), points(name), state(name, device_bvh, tmp)["walk"]
    tq, tv, tk = w.terms
    keep = st["keep"]
    in_batch = keep[tq]
    assert float((np.abs(tv[in_batch]) / W.FOUR_PI).min()) > 1e-7  # the condition under which 1e-10 sees every term
    assert keep.sum() >= 1024, int(keep.sum())
    assert all((tk[in_batch] == k).any() for k in (W.FAR_INNER, W.FAR_LEAF, W.EXACT)), "every kind of term is in the batch"
    # the model's sum, in extended precision, against the kernel's fp64 one
    assert int(np.bincount(tq, minlength=p.shape[0])[keep].max()) < 4096 and np.abs(tv).max() < 4.0 * W.FOUR_PI
    got, c = st["counted"], st["counters"]
    err = float(np.abs(got - w.value[keep]).max())
    print(f"{name}: {int(keep.sum())} of {p.shape[0]} queries; max |kernel - model| = {err:.3e}; per query {w.nodes[keep].mean():.1f} nodes, "
          f"{w.tris[keep].mean():.1f} solid angles, {w.far_inner[keep].mean():.1f} + {w.far_leaf[keep].mean():.1f} far terms")
    assert err <= 1e-10
    assert got.tobytes() == st["w2"][keep].tobytes()  # (and a pure function of the query: the same bits inside another batch)
    assert (c["node_fetches"], c["tri_tests"], c["inner_rounds"], c["leaf_rounds"]) == \
        (int(w.nodes[keep].sum()), int(w.tris[keep].sum()), int(w.far_inner[keep].sum()), int(w.far_leaf[keep].sum()))
    # every candidate, the small terms included
    assert float(np.abs(st["w2"] - w.value).max()) <= 1e-10


# ------------------------------------------------------------------------------------------------ c) exact mode
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", ("tetrahedron",) + WALK_SCENES + ("mixed_sizes",))
def test_exact_mode_is_the_brute_force_sum(gpu, tmp, name, device_bvh):
    key = ("exact", name)
    if key not in _cache:
        _cache[key] = SM.winding_number(points(name), scene(name).vertices)
    exact = _cache[key]
    assert np.abs(exact).max() < 4.0
    got = state(name, device_bvh, tmp)["winf"]
    err = float(np.abs(got - exact).max())
    print(f"{name}: beta = inf, max |kernel - brute force| = {err:.3e}")
    assert err <= 1e-10
    if name in ("tetrahedron", "notched_pyramid", "cornell_ball"):  # closed: inside / outside, at the default beta too
        assert np.array_equal(got > 0.5, exact > 0.5) and np.array_equal(state(name, device_bvh, tmp)["w2"] > 0.5, exact > 0.5)


# ------------------------------------------------------------------------------------------------ d) batches
def _device_winding(sc, q, beta, count_work=False):
    import torch
    dq = torch.from_numpy(q.view(np.uint8).reshape(-1)).cuda()
    out = torch.full((max(q.shape[0], 1) + 1,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sc.winding_number_device(dq.data_ptr(), q.shape[0], out.data_ptr(), beta=beta, count_work=count_work)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[q.shape[0]:] == -7.0).all()  # exactly n doubles are written
    return host[:q.shape[0]].copy()


def test_batch_boundaries_and_invariance(gpu, tmp):
    name = "open_sphere"
    data = scene(name)
    sc = api.Scene(data)
    sc.winding_queries = True
    sc.upload(0)
    n = 1 << 17
    p = W.box_queries(data.vertices, n=n, seed=17)
    p[:4096] = points(name)
    whole = sc.winding_number(p, 2.0)
    assert np.isfinite(whole).all() and whole[:4096].tobytes() == state(name, False, tmp)["w2"].tobytes()
    assert sc.winding_number(p, 2.0, count_work=True).tobytes() == whole.tobytes()
    assert sc.counters()["node_fetches"] >= n
    for m in (0, 1, 257):
        got = sc.winding_number(np.ascontiguousarray(p[:m]), 2.0)
        assert got.shape == (m,) and got.tobytes() == whole[:m].tobytes(), m
    order = np.random.default_rng(3).permutation(n)
    cuts = [0, 1, 64, 65, 257, 4096 + 13, 50000, n]
    got = np.empty(n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        got[order[a:b]] = sc.winding_number(np.ascontiguousarray(p[order[a:b]]), 2.0)
    assert got.tobytes() == whole.tobytes()
    q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
    q["p"] = p
    q["max_dist"] = np.nan  # (not read)
    assert _device_winding(sc, q, 2.0).tobytes() == whole.tobytes()
    assert _device_winding(sc, q, 2.0, count_work=True).tobytes() == whole.tobytes()
    assert _device_winding(sc, q[:1], 2.0).tobytes() == whole[:1].tobytes()
    assert _device_winding(sc, q[:0], 2.0).shape == (0,)
    assert np.array_equal(sc.inside(p[:300]), whole[:300] > 0.5)
    # a query on the surface: finite
    v = data.vertices.reshape(-1, 3, 3)
    on = np.ascontiguousarray(np.concatenate([v[:64, 0], v[:64].mean(axis=1), 0.5 * (v[:64, 0] + v[:64, 1])]))
    for beta in (2.0, np.inf):
        assert np.isfinite(sc.winding_number(on, beta)).all()
    with pytest.raises(api.PrtError) as e:
        sc.winding_number(p[:8], beta=1.0)
    assert e.value.code == _abi.PRT_E_INVALID
    sc.close()


# ------------------------------------------------------------------------------------------------ e) moving geometry
def _device_call(fn, v):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    torch.cuda.synchronize()
    fn(d.data_ptr())
    torch.cuda.synchronize()


def wobble(v0):
    p = v0.reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    return np.ascontiguousarray(v0 + 0.05 * ext * np.sin((3.0 / ext) * v0[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3])))


@pytest.mark.parametrize("how", ("refit_device", "rebuild_device", "refit", "rebuild"))
@pytest.mark.parametrize("name,device_bvh", [("open_sphere", False), ("cornell_ball", True)])
def test_geometry_follows(gpu, tmp, name, device_bvh, how):
    data = scene(name)
    v = wobble(data.vertices)
    p = points(name)
    path = str(tmp / f"moved-{name}-{how}.bin")
    with dumping(path):
        sc = api.Scene(data, device_bvh=device_bvh)
        sc.winding_queries = True
        sc.upload(0)
        before = sc.winding_moments()
        if how.endswith("_device"):
            _device_call(getattr(sc, how), v)
        else:
            getattr(sc, how)(v)
    assert sc.winding_queries is True and sc.distance_queries is True
    tree = M.read_dump(path)
    M.check_tree(tree, v, sc.bvh_info())
    table = sc.winding_moments()
    assert table.tobytes() != before.tobytes()
    check_table(table, tree, v, (name, how))
    w = W.walk(tree, v, p, 2.0, table)
    got = sc.winding_number(p, 2.0, count_work=True)
    c = sc.counters()
    assert float(np.abs(got - w.value).max()) <= 1e-10, (name, how)
    assert (c["node_fetches"], c["tri_tests"], c["inner_rounds"], c["leaf_rounds"]) == \
        (int(w.nodes.sum()), int(w.tris.sum()), int(w.far_inner.sum()), int(w.far_leaf.sum()))
    key = ("moved-exact", name)
    if key not in _cache:
        _cache[key] = SM.winding_number(p, v)
    assert float(np.abs(sc.winding_number(p, np.inf) - _cache[key]).max()) <= 1e-10, (name, how)
    if how == "refit":  # a refused refit leaves the table and the values as they were
        bad = v.copy()
        bad[3, 1, 2] = np.nan
        with pytest.raises(api.PrtError):
            sc.refit(bad)
        assert sc.winding_moments().tobytes() == table.tobytes() and sc.winding_number(p, 2.0).tobytes() == got.tobytes()
    if how == "rebuild":  # the rebuilt tree is the one a fresh device build of the moved scene gets: the same table
        fresh = api.Scene(with_vertices(data, v), device_bvh=True)
        fresh.winding_queries = True
        fresh.upload(0)
        assert fresh.winding_moments().shape == table.shape
        assert float(np.abs(fresh.winding_number(p, np.inf) - _cache[key]).max()) <= 1e-10
        fresh.close()
    sc.close()


def test_switch_life_cycle(gpu, tmp):
    name = "notched_pyramid"
    data, p = scene(name), points(name)
    want = state(name, False, tmp)
    sc = api.Scene(data).upload(0)  # on after the upload
    assert sc.winding_queries is False and sc.distance_queries is False
    for call in (lambda: sc.winding_number(p), sc.winding_moments):
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_winding_queries" in str(e.value)
    sc.winding_queries = True
    assert sc.distance_queries is True
    assert sc.winding_moments().tobytes() == want["table"].tobytes() and sc.winding_number(p).tobytes() == want["w2"].tobytes()
    with pytest.raises(api.PrtError) as e:
        sc.distance_queries = False
    assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_winding_queries" in str(e.value)
    sc.winding_queries = False  # off: the table goes, distance queries stay
    assert sc.distance_queries is True
    with pytest.raises(api.PrtError) as e:
        sc.winding_number(p)
    assert e.value.code == _abi.PRT_E_INVALID
    sc.winding_queries = True
    assert sc.winding_moments().tobytes() == want["table"].tobytes()
    v = wobble(data.vertices)
    sc.update_vertices(v)  # survives update_vertices, which builds a new tree on the device
    assert sc.winding_queries is True
    fresh = api.Scene(with_vertices(data, v), device_bvh=True)
    fresh.winding_queries = True
    fresh.upload(0)
    assert sc.winding_moments().tobytes() == fresh.winding_moments().tobytes()
    assert sc.winding_number(p).tobytes() == fresh.winding_number(p).tobytes()
    exact = SM.winding_number(p, v)
    assert float(np.abs(sc.winding_number(p, np.inf) - exact).max()) <= 1e-10
    fresh.close()
    # stale host geometry: switching on is refused, as for the other query switches
    sc.winding_queries = False
    _device_call(sc.refit_device, data.vertices)
    assert sc.refit_info()["host_stale"] == 1
    with pytest.raises(api.PrtError) as e:
        sc.winding_queries = True
    assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_winding_queries" in str(e.value) and "before moving geometry" in str(e.value)
    assert sc.winding_queries is False
    sc.close()


# ------------------------------------------------------------------------------------------------ f) the other point queries
def test_other_point_queries_are_unchanged_by_the_switch(gpu):
    name = "cornell_ball"
    sc = api.Scene(scene(name))
    sc.signed_queries = True
    sc.upload(0)
    p = points(name)
    before = (sc.closest_point(p), sc.signed_distance(p), sc.pseudonormals())
    sc.winding_queries = True
    w = sc.winding_number(p)
    after = (sc.closest_point(p), sc.signed_distance(p), sc.pseudonormals())
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    # on this closed shape the two inside / outside answers agree wherever the distance decides robustly
    far = np.abs(after[1]["sdist"]) > 1e-9
    assert np.array_equal((w > 0.5)[far], (after[1]["sign"] < 0)[far])
    sc.winding_queries = False
    assert sc.closest_point(p).tobytes() == before[0].tobytes() and sc.signed_distance(p).tobytes() == before[1].tobytes()
    sc.close()


# ------------------------------------------------------------------------------------------------ C++
def test_cpp_winding_number_equals_the_exact_sum(gpu, tmp_path):
    """Hittable::WindingNumber on the notched pyramid, loaded as main.cpp loads a model: beta = inf against brute force, and
    at the default beta the same inside / outside (the C++ world's tree need not be the binding's: values are not compared
    bit for bit, contract item 5)."""
    import subprocess
    from pooraytracer_amd import build, scenes
    build.build_host_example()
    exe = str(tmp_path / "winding_check")
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "winding_check.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    name = "notched_pyramid"
    data = scene(name)
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    p = np.ascontiguousarray(points(name)[:512])
    p.tofile(str(tmp_path / "points.f64"))
    exact = SM.winding_number(p, data.vertices)
    for beta in ("inf", "2"):
        out = str(tmp_path / "out.f64")
        r = subprocess.run([exe, res, data.name, str(tmp_path / "points.f64"), beta, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, dtype=np.float64)
        assert got.shape == (512,)
        if beta == "inf":
            assert float(np.abs(got - exact).max()) <= 1e-10
        assert np.array_equal(got > 0.5, exact > 0.5) and (got > 0.5).any() and not (got > 0.5).all()
