"""CPU tests of the signed distance queries (prt_signed_distance, include/prt.h): header, ABI and symbols agree; the host
topology pass (mesh_topology.cpp) equals the numpy model (tests/signed_distance_model.py); the model's sign equals the
winding-number truth where the plane-side sign and an equal-weight normal sum do not; the switch and the refusals that need
no device; and mesh_topology.cpp under AddressSanitizer and UBSan as a plain executable."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from tests import bvh_model as M
from tests import signed_distance_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prt_scene_topology_info", "prt_scene_set_signed_queries", "prt_scene_get_signed_queries", "prt_scene_pseudonormals",
               "prt_signed_distance", "prt_signed_distance_device")


# ------------------------------------------------------------------------------------------------- header and ABI
def test_abi_is_additive(prt_lib, tmp_path):
    fields = ("sdist", "point", "alpha", "beta", "prim", "feature", "side", "sign")
    twin = ("dist", "point", "alpha", "beta", "prim", "feature", "side", "reserved")
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "prt.h"\nint main(){printf("%d %zu %zu %zu\\n",PRT_ABI_VERSION,'
                   "sizeof(PrtSignedDistance),sizeof(PrtClosestPoint),sizeof(PrtTopologyInfo));"
                   + "".join(f'printf("%zu %zu\\n",offsetof(PrtSignedDistance,{a}),offsetof(PrtClosestPoint,{b}));' for a, b in zip(fields, twin))
                   + "".join(f'printf("%zu\\n",offsetof(PrtTopologyInfo,{f}));' for f, _ in _abi.PrtTopologyInfo._fields_)
                   + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().strip().split("\n")
    assert lines[0].split() == ["6", "64", "64", str(C.sizeof(_abi.PrtTopologyInfo))]
    assert _abi.PRT_ABI_VERSION == 6 and prt_lib.prt_abi_version() == 6
    assert C.sizeof(_abi.PrtSignedDistance) == _abi.SIGNED_DISTANCE_DTYPE.itemsize == 64
    for f, line in zip(fields, lines[1:9]):  # the layout of PrtClosestPoint, in the header, in ctypes and in numpy
        a, b = (int(x) for x in line.split())
        assert a == b == getattr(_abi.PrtSignedDistance, f).offset == _abi.SIGNED_DISTANCE_DTYPE.fields[f][1], f
    for (f, _), line in zip(_abi.PrtTopologyInfo._fields_, lines[9:]):
        assert int(line) == getattr(_abi.PrtTopologyInfo, f).offset, f
    for name in NEW_SYMBOLS:
        assert name in _abi.EXPORTS and hasattr(prt_lib, name), name
    hdr = open(os.path.join(ROOT, "include", "prt.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in hdr, name


# ------------------------------------------------------------------------------------------------- topology
def _cornell():
    return scenes.cornell_box(ball_subdiv=3, width=64, height=64)


def ball_alone(data=None):
    """The cornell ball as a scene of its own: the mesh with the most triangles."""
    data = data or _cornell()
    first = list(np.asarray(data.mesh_first_tri, dtype=np.int64)) + [data.vertices.shape[0]]
    k = int(np.argmax(np.diff(first)))
    return M._scene("cornell_ball", np.ascontiguousarray(data.vertices[first[k]:first[k + 1]]))


TOPOLOGY_SCENES = {
    "tetrahedron": SM.tetrahedron,
    "notched_pyramid": SM.notched_pyramid,
    "cornell": _cornell,
    "cornell_ball": ball_alone,
    "walls": M.walls,
    "identical": M.identical,
    "mixed_materials": scenes.mixed_materials,
    "soup_at_1e6": lambda: M.translated(M.soup(4096)),
}
# what the issue's throwaway model counted: (V, E, boundary, non-manifold, closed) - a cross-check of the model here
CROSS_CHECK = {"tetrahedron": (4, 6, 0, 0, 1), "notched_pyramid": (134, 396, 0, 0, 1), "cornell": (654, 1942, 8, 0, 0),
               "cornell_ball": (642, 1920, 0, 0, 1), "walls": (18000, 18000, 18000, 0, 0), "identical": (3, 3, 0, 3, 0)}


@pytest.mark.parametrize("name", list(TOPOLOGY_SCENES))
def test_topology_info_equals_the_model(prt_lib, name):
    data = TOPOLOGY_SCENES[name]()
    sc = api.Scene(data)
    info = sc.topology_info()
    want = SM.topology(data.vertices)["info"]
    print(name, info)
    assert info.pop("table_bytes") == 0
    assert info == want
    if name in CROSS_CHECK:
        got = (want["n_vertices"], want["n_edges"], want["boundary_edges"], want["nonmanifold_edges"], want["closed"])
        assert got == CROSS_CHECK[name]
    if name == "identical":
        assert info["max_valence"] == 3000
    sc.close()


def test_topology_special_cases(prt_lib):
    rev = M._scene("tet_reversed", SM.tetrahedron_vertices(reverse_face=0))
    sc = api.Scene(rev)
    info = sc.topology_info()
    assert info["inconsistent_edges"] == 3 and info["closed"] == 0 and info["boundary_edges"] == 0
    assert SM.topology(rev.vertices)["info"]["inconsistent_edges"] == 3
    sc.close()
    # two equal corners: degenerate; -0.0 welds to +0.0 (the second triangle shares the edge (0,0,0)-(1,0,0) through a -0.0)
    v = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]],
                  [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
                  [[1.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, -1.0, 0.0]]])
    sc = api.Scene(M._scene("special", v))
    info = sc.topology_info()
    want = SM.topology(v)["info"]
    info.pop("table_bytes")
    assert info == want
    assert info["degenerate_tris"] == 1 and info["n_vertices"] == 4
    # edge (0,0,0)-(1,0,0): twice from the degenerate triangle, once from each of the others -> four faces
    assert info["nonmanifold_edges"] == 1 and info["n_edges"] == 5 and info["boundary_edges"] == 4
    assert prt_lib.prt_scene_topology_info(None, None) == _abi.PRT_E_INVALID
    sc.close()


# ------------------------------------------------------------------------------------------------- the model against the truth
def test_model_sign_on_the_tetrahedron():
    v = SM.tetrahedron_vertices()
    p = np.random.default_rng(2005).random((4096, 3)) * 4.0 - 2.0
    truth = SM.tetrahedron_inside(p)
    assert np.array_equal(truth, SM.inside_truth(p, v))  # the winding number agrees with the analytic answer
    sign, r = SM.model_sign(p, v)
    far = np.sqrt(r["d2"]) > 1e-6
    assert far.sum() > 4000 and (truth == -1).sum() > 100
    assert np.array_equal(sign[far], truth[far])
    wrong_side = int((r["side"][far] != truth[far]).sum())
    print(f"tetrahedron: `side` wrong on {wrong_side} of {int(far.sum())}, pseudonormal sign on 0")
    assert wrong_side > 0
    assert set(r["feature"].tolist()) == set(range(7))


def test_model_sign_near_the_apex_of_the_notched_pyramid():
    v = SM.notched_pyramid_vertices()
    assert v.shape == (264, 3, 3)
    p = SM.apex_queries()
    truth = SM.inside_truth(p, v)
    sign, r = SM.model_sign(p, v)
    far = np.sqrt(r["d2"]) > 1e-6
    assert far.sum() > 4000 and 100 < (truth == -1).sum() < 3996
    assert np.array_equal(sign[far], truth[far])
    wrong_side = int((r["side"][far] != truth[far]).sum())
    equal, _ = SM.model_sign(p, v, equal_weight=True)
    wrong_equal = int((equal[far] != truth[far]).sum())
    print(f"notched pyramid: `side` wrong on {wrong_side}, equal-weight sum on {wrong_equal}, angle-weighted on 0 of {int(far.sum())}")
    assert wrong_side > 0 and wrong_equal > 0  # the angle weights are what makes it exact


# ------------------------------------------------------------------------------------------------- without a GPU
def test_switch_works_without_upload(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    assert sc.signed_queries is False and sc.distance_queries is False
    sc.signed_queries = True
    assert sc.signed_queries is True and sc.distance_queries is True  # it switches distance queries on
    with pytest.raises(api.PrtError) as e:
        sc.distance_queries = False
    assert e.value.code == _abi.PRT_E_INVALID
    assert "prt_scene_set_distance_queries" in str(e.value) and "prt_scene_set_signed_queries" in str(e.value)
    assert sc.distance_queries is True
    sc.update_vertices(scenes.tiny_scene().vertices * 2.0)  # survives a (host-only) update
    assert sc.signed_queries is True and sc.distance_queries is True
    sc.signed_queries = False
    assert sc.signed_queries is False and sc.distance_queries is True  # distance queries stay as they are
    sc.distance_queries = False
    assert prt_lib.prt_scene_set_signed_queries(None, 1) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_get_signed_queries(sc._h, None) == _abi.PRT_E_INVALID
    sc.close()


def test_queries_fail_loudly_without_upload(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    p = np.zeros((3, 3))
    calls = {"prt_signed_distance": lambda: sc.signed_distance(p), "prt_signed_distance_device": lambda: sc.signed_distance_device(256, 3, 512),
             "prt_scene_pseudonormals": sc.pseudonormals}
    for name, call in calls.items():  # the switch is off
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_INVALID and name + ":" in str(e.value) and "prt_scene_set_signed_queries" in str(e.value)
    sc.distance_queries = True  # distance queries alone are not enough
    with pytest.raises(api.PrtError) as e:
        sc.signed_distance(p)
    assert e.value.code == _abi.PRT_E_INVALID
    sc.signed_queries = True
    for name, call in calls.items():  # on, but no device
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_NO_DEVICE and name + ":" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.signed_distance(np.zeros((0, 3)))  # no query, still no device
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc.close()


def test_host_call_refuses_bad_queries(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    for bad in (np.nan, np.inf, -np.inf):
        p = np.zeros((4, 3))
        p[2, 1] = bad
        with pytest.raises(api.PrtError) as e:
            sc.signed_distance(p)
        assert e.value.code == _abi.PRT_E_INVALID and "prt_signed_distance" in str(e.value) and "query 2" in str(e.value)
    for bad in (-1.0, -1e-300, np.nan, -np.inf):
        md = np.ones(4)
        md[1] = bad
        with pytest.raises(api.PrtError) as e:
            sc.signed_distance(np.zeros((4, 3)), max_dist=md)
        assert e.value.code == _abi.PRT_E_INVALID and "max_dist" in str(e.value) and "query 1" in str(e.value)
    with pytest.raises(TypeError):
        sc.signed_distance([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError):
        sc.signed_distance(np.zeros((2, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        sc.signed_distance(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        sc.signed_distance(np.zeros((2, 3)), max_dist=np.ones(3))
    sc.close()


# ------------------------------------------------------------------------------------------------- sanitizers
def test_mesh_topology_under_sanitizers(tmp_path):
    """mesh_topology.cpp and its stand-alone driver as ONE plain executable with AddressSanitizer and UBSan (nothing is loaded
    into Python): the shapes above, an empty scene, one triangle, all-degenerate input and 3000 duplicates."""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mesh_topology_sanitize")
    # the sanitizer runtimes are linked statically: the executable needs nothing from its environment
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "pooraytracer_amd", "csrc", "mesh_topology.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "mesh_topology_sanitize.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mesh_topology: ok" in r.stdout, r.stdout + r.stderr
