"""CPU tests of the winding-number queries (prt_winding_number, include/prt.h): header, ABI and symbols agree; the numpy
model (tests/winding_model.py) on host-built trees (the dev-hooks library's PRT_TEST_DUMP_BVH dump at prt_scene_create; no
GPU needed) against the brute-force sum of signed_distance_model.winding_number; the switch and the refusals that need no
device; the api wrappers.

Queries: 4,096 uniform points in 1.5 x the bounds of each scene.  BETA2_ERROR is the model's largest error against brute
force at beta = 2 per scene, rounded up to one significant digit (DESIGN.md section 7 has the measured values); the host
builder is deterministic, so the bound needs no wider margin.  Where the beta = 2 walk takes no far term at all (the
tetrahedron, the identical triangles: every query lies within twice the radius of every cluster) the beta = 4 walk is the
same walk and "smaller error" is checked as "the same values"."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from pooraytracer_amd import _abi, api
from tests import bvh_model as M
from tests import closest_point_model as CM
from tests import signed_distance_model as SM
from tests import winding_model as W
from tests.test_signed_distance_cpu import ball_alone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prt_scene_set_winding_queries", "prt_scene_get_winding_queries", "prt_scene_winding_moments", "prt_winding_number",
               "prt_winding_number_device")

SCENES = {
    "tetrahedron": SM.tetrahedron,
    "notched_pyramid": SM.notched_pyramid,
    "cornell_ball": lambda: ball_alone(CM.scene("cornell")),
    "open_sphere": W.open_sphere,
    "open_box": W.open_box,
    "cornell": lambda: CM.scene("cornell"),
    "identical": lambda: M.identical(1000),
    "mixed_sizes": M.mixed_sizes,
}
CLOSED = ("tetrahedron", "notched_pyramid", "cornell_ball")
OPEN = ("open_sphere", "open_box", "cornell")
# the model's largest |w(beta = 2) - w_exact| over the 4,096 queries, rounded up to one significant digit
BETA2_ERROR = {"tetrahedron": 3e-16, "notched_pyramid": 3e-3, "cornell_ball": 3e-2, "open_sphere": 4e-2, "open_box": 4e-2,
               "cornell": 3e-2, "identical": 3e-13, "mixed_sizes": 3e-3}


def dump_tree(data):
    """The host-built tree of `data` as the kernels would get it (bvh_model.Tree), checked against the vertices."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tree.bin")
        saved = os.environ.get("PRT_TEST_DUMP_BVH")
        os.environ["PRT_TEST_DUMP_BVH"] = path
        try:
            with api.dev_hooks():
                api.Scene(data).close()
        finally:
            if saved is None:
                del os.environ["PRT_TEST_DUMP_BVH"]
            else:
                os.environ["PRT_TEST_DUMP_BVH"] = saved
        tree = M.read_dump(path)
    M.check_tree(tree, data.vertices)
    return tree


@functools.lru_cache(maxsize=None)
def case(name):
    """(data, tree, queries, brute force, moments), computed once and left unchanged."""
    data = SCENES[name]()
    tree = dump_tree(data)
    p = W.box_queries(data.vertices)
    exact = SM.winding_number(p, data.vertices)
    for a in (p, exact):
        a.setflags(write=False)
    return data, tree, p, exact, W.moments(tree, data.vertices)


@functools.lru_cache(maxsize=None)
def walked(name, beta):
    data, tree, p, _, table = case(name)
    return W.walk(tree, data.vertices, p, beta, table)


# ------------------------------------------------------------------------------------------------- header and ABI
def test_abi_is_additive(prt_lib, tmp_path):
    src = tmp_path / "w.c"
    src.write_text('#include <stdio.h>\n#include "prt.h"\nint main(){printf("%d %.17g %zu\\n",PRT_ABI_VERSION,PRT_WINDING_BETA_DEFAULT,'
                   "sizeof(PrtPointQuery));\n"
                   "int (*a)(PrtScene*, const PrtPointQuery*, size_t, double, double*, int) = prt_winding_number;\n"
                   "int (*b)(PrtScene*, const void*, size_t, double, void*, int, void*) = prt_winding_number_device;\n"
                   "int (*c)(PrtScene*, double*, uint64_t, uint64_t*) = prt_scene_winding_moments;\n"
                   "int (*d)(PrtScene*, int) = prt_scene_set_winding_queries;\n"
                   "int (*e)(const PrtScene*, int*) = prt_scene_get_winding_queries;\n"
                   "return !(a && b && c && d && e);}\n")
    exe = tmp_path / "w"
    lib_dir = os.path.dirname(api.__file__)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib_dir, "-Wl,-rpath," + lib_dir, "-lprt_hip",
                           "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["6", "2", "32"]
    assert _abi.PRT_ABI_VERSION == 6 and prt_lib.prt_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "prt.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _abi.EXPORTS and hasattr(prt_lib, name) and f"int {name}(" in hdr, name
    assert "depend on the tree" in hdr  # contract item 5 says so


# ------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", list(SCENES))
def test_exact_mode_is_the_brute_force_sum(prt_lib, name):
    data, tree, p, exact, _ = case(name)
    assert data.vertices.shape[0] <= 3100
    w = walked(name, np.inf)
    err = float(np.abs(w.value - exact).max())
    print(f"{name}: {data.vertices.shape[0]} triangles, {tree.n_nodes} nodes, beta = inf: max |model - brute force| = {err:.3e}")
    assert err <= 1e-10
    assert (w.far_inner == 0).all() and (w.far_leaf == 0).all()
    assert (w.tris == tree.n_tris).all() and (w.nodes == tree.n_nodes).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_error_at_the_default_beta_and_beyond(prt_lib, name):
    _, tree, p, exact, _ = case(name)
    w2, w4 = walked(name, 2.0), walked(name, 4.0)
    e2, e4 = float(np.abs(w2.value - exact).max()), float(np.abs(w4.value - exact).max())
    far2 = w2.far_inner + w2.far_leaf
    print(f"{name}: beta = 2: max error {e2:.3e}, per query {far2.mean():.1f} far terms, {w2.nodes.mean():.1f} nodes, "
          f"{w2.tris.mean():.1f} exact triangles; beta = 4: max error {e4:.3e}, {(w4.far_inner + w4.far_leaf).mean():.1f} far terms, "
          f"{w4.nodes.mean():.1f} nodes, {w4.tris.mean():.1f} exact triangles")
    assert e2 <= BETA2_ERROR[name]
    if far2.any():
        assert e4 < e2
        assert w4.nodes.sum() > w2.nodes.sum()  # the price
    else:
        assert np.array_equal(w4.value, w2.value) and e4 == e2
    assert np.isfinite(w2.value).all()


@pytest.mark.parametrize("name", CLOSED + OPEN)
def test_inside_outside_at_the_default_beta(prt_lib, name):
    _, _, p, exact, _ = case(name)
    w = walked(name, 2.0).value
    wrong = (w > 0.5) != (exact > 0.5)
    if name in CLOSED:
        assert np.abs(exact - np.round(exact)).max() < 1e-9 and (exact > 0.5).any() and not (exact > 0.5).all()
        assert not wrong.any()
    else:
        clear = np.abs(exact - 0.5) >= 0.25
        print(f"{name}: {int(wrong.sum())} of {p.shape[0]} queries classified differently, all with |w - 0.5| < 0.25; "
              f"{int((~clear).sum())} queries are that close")
        # (the cornell room's walls face inward: w is about -0.9 inside it, and nothing there is "inside" by the threshold)
        assert clear.sum() > p.shape[0] // 2 and np.abs(exact[clear]).max() > 0.5
        assert not (wrong & clear).any()


def test_moments_of_a_slot_hold_its_triangles(prt_lib):
    """The record's own invariants on an adversarial tree: every corner below a slot lies within r of c (up to rounding),
    A is the area below it and N the area vector; unused slots are zero; the root's slots sum to the whole scene."""
    data, tree, _, _, table = case("mixed_sizes")
    v = data.vertices.reshape(-1, 3, 3)
    av = 0.5 * np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    refs = tree.nodes["ref"].astype(np.int64)
    assert not table[refs == M.UNUSED].any()
    root = table[0][refs[0] != M.UNUSED]
    assert abs(root[:, 7].sum() - np.linalg.norm(av, axis=1).sum()) <= 1e-12 * root[:, 7].sum()
    assert np.abs(root[:, 0:3].sum(0) - av.sum(0)).max() <= 1e-12 * np.abs(av).sum()

    def below(node, slot):
        r = refs[node, slot]
        if r < 0:
            f, c = M.decode_leaf(r)
            return list(tree.order[int(f):int(f + c)])
        return [t for s in range(4) if refs[r, s] != M.UNUSED for t in below(r, s)]

    for node in range(0, tree.n_nodes, 37):
        for slot in range(4):
            if refs[node, slot] == M.UNUSED:
                continue
            rec, tris = table[node, slot], below(node, slot)
            d = np.linalg.norm(v[tris].reshape(-1, 3) - rec[3:6], axis=1)
            assert d.max() <= rec[6] * (1 + 1e-12) + 1e-300, (node, slot)
            assert abs(rec[7] - np.linalg.norm(av[tris], axis=1).sum()) <= 1e-12 * max(rec[7], 1e-300)


# ------------------------------------------------------------------------------------------------- the switch, the refusals
def test_switch_and_refusals_without_a_device(prt_lib):
    sc = api.Scene(SM.tetrahedron())
    p = np.zeros((3, 3))
    assert sc.winding_queries is False
    for call, fn in ((lambda: sc.winding_number(p), "prt_winding_number:"),
                     (lambda: sc.winding_number_device(64, 3, 128), "prt_winding_number_device:"),
                     (sc.winding_moments, "prt_scene_winding_moments:")):
        with pytest.raises(api.PrtError) as e:  # the switch is off: before the missing device
            call()
        assert e.value.code == _abi.PRT_E_INVALID and fn in str(e.value) and "prt_scene_set_winding_queries" in str(e.value)
    sc.winding_queries = True
    assert sc.winding_queries is True and sc.distance_queries is True and sc.signed_queries is False
    with pytest.raises(api.PrtError) as e:
        sc.distance_queries = False
    assert e.value.code == _abi.PRT_E_INVALID and "prt_scene_set_winding_queries" in str(e.value)
    for beta in (1.0, 0.5, 0.0, -2.0, float("nan"), -np.inf):  # beta before the missing device
        for call in (lambda: sc.winding_number(p, beta=beta), lambda: sc.winding_number_device(64, 3, 128, beta=beta)):
            with pytest.raises(api.PrtError) as e:
                call()
            assert e.value.code == _abi.PRT_E_INVALID and "beta" in str(e.value), beta
    for beta in (2.0, 1.0000001, np.inf):  # a good beta: what is missing now is the device
        with pytest.raises(api.PrtError) as e:
            sc.winding_number(p, beta=beta)
        assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_winding_number:" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.inside(p)
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    with pytest.raises(api.PrtError) as e:
        sc.winding_moments()
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    bad = p.copy()
    bad[1, 2] = np.inf
    with pytest.raises(api.PrtError) as e:  # the host call checks the batch before the device
        sc.winding_number(bad)
    assert e.value.code == _abi.PRT_E_INVALID and "query 1" in str(e.value)
    sc.winding_queries = False
    assert sc.winding_queries is False and sc.distance_queries is True  # distance queries stay on
    sc.distance_queries = False
    sc.signed_queries = True  # the two switches are independent, and each holds the corner table
    sc.winding_queries = True
    sc.signed_queries = False
    with pytest.raises(api.PrtError):
        sc.distance_queries = False
    sc.close()


def test_api_wrappers_check_shapes_before_any_call(prt_lib):
    sc = api.Scene(SM.tetrahedron())
    sc.winding_queries = True
    with pytest.raises(TypeError, match="winding_number: points must be float64"):
        sc.winding_number(np.zeros((2, 3), dtype=np.float32))
    with pytest.raises(ValueError, match=r"winding_number: points must have shape \(n, 3\)"):
        sc.winding_number(np.zeros((2, 4)))
    with pytest.raises(TypeError, match="winding_number: points must be a numpy array"):
        sc.inside([[0.0, 0.0, 0.0]])
    import inspect
    assert inspect.signature(api.Scene.winding_number).parameters["beta"].default == 2.0
    assert inspect.signature(api.Scene.inside).parameters["beta"].default == 2.0
    assert inspect.signature(api.Scene.winding_number_device).parameters["beta"].default == 2.0
    sc.close()
    L = prt_lib
    on = __import__("ctypes").c_int(7)
    assert L.prt_scene_get_winding_queries(None, on) == _abi.PRT_E_INVALID
    assert L.prt_scene_set_winding_queries(None, 1) == _abi.PRT_E_INVALID
    assert L.prt_winding_number(None, None, 0, 2.0, None, 0) == _abi.PRT_E_INVALID
