"""Surface queries without a GPU: the ABI surface of prt_trace_surface* (symbols, the PrtSurface layout in C, ctypes and
numpy), the refusals that need no device, and hand-derived known answers of tests/surface_model.py — the model the GPU
tests (tests/test_gpu_surface.py) compare the kernel's records with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from tests import surface_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prt_trace_surface", "prt_trace_surface_device", "prt_trace_surface_sorted_device")
FIELDS = ("t", "alpha", "beta", "prim", "front", "position", "normal", "tangent", "uv", "albedo", "emission", "material",
          "material_type", "reserved")
OFFSETS = (0, 8, 16, 24, 28, 32, 56, 80, 104, 120, 144, 168, 172, 176)  # the header's field order, doubles first in each run


# ------------------------------------------------------------------------------------------------ 1
def test_symbols_are_declared_listed_and_exported(prt_lib):
    hdr = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, name
        assert name in _abi.EXPORTS, name
        assert hasattr(prt_lib, name), name
    assert "typedef struct PrtSurface" in hdr
    assert re.search(r"#define\s+PRT_ABI_VERSION\s+6\b", hdr)
    assert _abi.PRT_ABI_VERSION == 6 and prt_lib.prt_abi_version() == 6


# ------------------------------------------------------------------------------------------------ 2
def test_record_layout_agrees_between_c_ctypes_and_numpy(tmp_path):
    src = tmp_path / "surf.c"
    offs = ",".join(f"offsetof(PrtSurface,{f})" for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "prt.h"\nint main(){size_t o[]={' + offs + "};"
                   'printf("%zu %zu",sizeof(PrtSurface),sizeof(PrtHit));for(unsigned i=0;i<sizeof o/sizeof o[0];++i)printf(" %zu",o[i]);'
                   'printf("\\n");return 0;}\n')
    exe = tmp_path / "surf"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert nums[0] == 192 and nums[1] == 32
    assert tuple(nums[2:]) == OFFSETS
    assert C.sizeof(_abi.PrtSurface) == 192 and _abi.SURFACE_DTYPE.itemsize == 192
    assert tuple(f for f, _ in _abi.PrtSurface._fields_) == FIELDS
    assert tuple(_abi.SURFACE_DTYPE.names) == FIELDS
    for f, off in zip(FIELDS, OFFSETS):
        assert getattr(_abi.PrtSurface, f).offset == off, f
        assert _abi.SURFACE_DTYPE.fields[f][1] == off, f
    # the first 32 bytes ARE a PrtHit: same names, types and offsets as HIT_DTYPE
    for f in _abi.HIT_DTYPE.names:
        assert _abi.SURFACE_DTYPE.fields[f][:2] == _abi.HIT_DTYPE.fields[f][:2], f
    assert max(_abi.HIT_DTYPE.fields[f][1] + _abi.HIT_DTYPE.fields[f][0].itemsize for f in _abi.HIT_DTYPE.names) == 32
    shapes = {"position": (3,), "normal": (3,), "tangent": (3,), "uv": (2,), "albedo": (3,), "emission": (3,), "reserved": (4,)}
    for f, shp in shapes.items():
        assert _abi.SURFACE_DTYPE.fields[f][0].shape == shp, f


# ------------------------------------------------------------------------------------------------ 3, 4
def test_a_scene_that_is_not_uploaded_is_refused_by_name(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    rays = scenes.random_rays(4, (-1, -1, -1), (1, 1, 1))
    out = np.full(4 * 192 + 64, 0xAA, dtype=np.uint8)
    L = sc._L
    dev = (0, 0, None)
    for fn, who, tail in ((L.prt_trace_surface, "prt_trace_surface", (0,)),
                          (L.prt_trace_surface_device, "prt_trace_surface_device", dev),
                          (L.prt_trace_surface_sorted_device, "prt_trace_surface_sorted_device", dev)):
        assert fn(sc._h, rays.ctypes.data, 4, out.ctypes.data, *tail) == _abi.PRT_E_NO_DEVICE, who
        assert L.prt_last_error().decode() == who + ": scene is not uploaded to a HIP device (no CPU path exists)"
        assert (out == 0xAA).all(), who
    with pytest.raises(api.PrtError) as e:
        sc.trace_surface(rays)
    assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_trace_surface" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.trace_surface_device(1 << 20, 4, 1 << 21)  # (never dereferenced: the scene check comes first)
    assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_trace_surface_device" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.trace_surface_device(1 << 20, 4, 1 << 21, sort=True)
    assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_trace_surface_sorted_device" in str(e.value)
    sc.close()


def test_an_empty_batch_answers_as_closest_hit_does(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    L = sc._L
    assert L.prt_trace_surface(sc._h, None, 0, None, 0) == L.prt_trace_closest(sc._h, None, 0, None, 0)
    assert L.prt_trace_surface_device(sc._h, None, 0, None, 0, 0, None) == L.prt_trace_closest_device_prec(sc._h, None, 0, None, 0, 0, None)
    assert L.prt_trace_surface_sorted_device(sc._h, None, 0, None, 0, 0, None) == L.prt_trace_closest_sorted_device(sc._h, None, 0, None, 0, 0, None)
    sc.close()


# ------------------------------------------------------------------------------------------------ 5
def _one_triangle(verts, uvs, material, normals=None, textures=()):
    v = np.asarray(verts, np.float64).reshape(1, 3, 3)
    return scenes.SceneData(name="one", vertices=v, texcoords=np.asarray(uvs, np.float64).reshape(1, 3, 2),
                            normals=np.zeros((1, 3, 3)) if normals is None else np.asarray(normals, np.float64).reshape(1, 3, 3),
                            mesh_first_tri=np.array([0, 1], np.uint64), mesh_material=np.array([0], np.int32), mesh_names=["t"],
                            materials=[material], camera=scenes.Camera(4, 4, 40.0, (0, 0, 3), (0, 0, 0)), textures=list(textures))


def _head(t, alpha, beta, prim, front):
    h = np.zeros(len(t), dtype=_abi.HIT_DTYPE)
    h["t"], h["alpha"], h["beta"], h["prim"], h["front"] = t, alpha, beta, prim, front
    return h


def _rays(o, d):
    r = np.zeros(len(o), dtype=_abi.RAY_DTYPE)
    r["o"], r["d"], r["tmin"], r["tmax"] = o, d, 1e-4, np.inf
    return r


UNIT_TRI = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
IDENT_UV = [(0, 0), (1, 0), (0, 1)]
WHITE = scenes.Material("w", _abi.MAT_LAMBERTIAN, kd=(0.25, 0.5, 0.75))


def test_model_unit_triangle_from_both_sides():
    data = _one_triangle(UNIT_TRI, IDENT_UV, WHITE)
    # from +z straight down at (0.25, 0.5), direction of length 2: t = 1.5 / 2; from -z upwards: t = 1
    rays = _rays([(0.25, 0.5, 1.5), (0.25, 0.5, -1.0)], [(0, 0, -2.0), (0, 0, 1.0)])
    head = _head([0.75, 1.0], [0.25, 0.25], [0.5, 0.5], [0, 0], [1, 0])
    r = M.records(data, rays, head)
    assert np.array_equal(r["position"], [(0.25, 0.5, 0.0), (0.25, 0.5, 0.0)])
    assert np.array_equal(r["normal"], [(0, 0, 1), (0, 0, -1)])          # on the ray's side
    assert np.array_equal(r["tangent"], [(1, 0, 0), (1, 0, 0)])          # as stored, not flipped
    assert np.array_equal(r["uv"], [(0.25, 0.5), (0.25, 0.5)])           # identity uv: the barycentric mix
    assert np.array_equal(r["albedo"], [(0.25, 0.5, 0.75)] * 2) and (r["emission"] == 0).all()
    assert r["material"].tolist() == [0, 0] and r["material_type"].tolist() == [_abi.MAT_LAMBERTIAN] * 2
    assert (r["reserved"] == 0).all()
    assert r.view(np.uint8).reshape(2, 192)[:, :32].tobytes() == head.tobytes()
    # a non-trivial uv map: u along +y, v along -x  ->  uv = (0,1) + alpha (0,-1)... checked as the weighted sum
    data2 = _one_triangle(UNIT_TRI, [(0.0, 1.0), (0.0, 0.0), (1.0, 1.0)], WHITE)
    r2 = M.records(data2, rays, head)
    assert np.allclose(r2["uv"], [(0.5, 0.75)] * 2, rtol=0, atol=1e-16)  # 0.25 (0,1) + 0.25 (0,0) + 0.5 (1,1)
    # tangent = direction of growing u in the plane: u grows along +y here
    assert np.allclose(r2["tangent"], [(0, 1, 0)] * 2, rtol=0, atol=1e-16)


def test_model_miss_pattern():
    data = _one_triangle(UNIT_TRI, IDENT_UV, WHITE)
    r = M.records(data, _rays([(5, 5, 5)], [(0, 0, 1)]), _head([np.inf], [0], [0], [-1], [0]))[0]
    assert np.isinf(r["t"]) and r["t"] > 0 and r["alpha"] == 0 and r["beta"] == 0 and r["prim"] == -1 and r["front"] == 0
    for f in ("position", "normal", "tangent", "uv", "albedo", "emission", "reserved"):
        assert (r[f] == 0).all(), f
    assert r["material"] == -1 and r["material_type"] == -1
    want = bytearray(192)
    want[0:8] = np.float64(np.inf).tobytes()
    want[24:28] = b"\xff" * 4
    want[168:176] = b"\xff" * 8
    assert r.tobytes() == bytes(want)


def test_model_degenerate_face_uses_the_vertex_normals():
    line = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]  # zero area: cross = 0, normalize = NaN
    vn = [(0, 3, 0), (0, 1, 0), (0, 4, 0)]    # their sum normalises to +y
    n, t = M.triangle_frames([line], [vn], [IDENT_UV])
    assert np.array_equal(n, [(0, 1, 0)])
    assert np.array_equal(t, [(1, 0, 0)])     # from the uv deltas: f (dv1 e0 - dv0 e1) = e0 = +x
    n, t = M.triangle_frames([line], None, [IDENT_UV])  # no vertex normals either: +z
    assert np.array_equal(n, [(0, 0, 1)])
    # the record's normal is that fallback, flipped to the ray's side
    data = _one_triangle(line, IDENT_UV, WHITE, normals=vn)
    r = M.records(data, _rays([(0.5, 1, 0), (0.5, -1, 0)], [(0, -1, 0), (0, 1, 0)]), _head([1, 1], [0.5, 0.5], [0, 0], [0, 0], [1, 0]))
    assert np.array_equal(r["normal"], [(0, 1, 0), (0, -1, 0)])


def test_model_zero_area_uv_triangle_uses_the_helper_axis():
    same_uv = [(0.3, 0.3)] * 3
    n, t = M.triangle_frames([UNIT_TRI], None, [same_uv])
    assert np.array_equal(n, [(0, 0, 1)])
    assert np.array_equal(t, [(0, 1, 0)])     # |n.x| < 0.9: helper +x, cross(+z, +x) = +y
    yz = [(0, 0, 0), (0, 1, 0), (0, 0, 1)]    # normal +x: helper +y, cross(+x, +y) = +z
    n, t = M.triangle_frames([yz], None, [same_uv])
    assert np.array_equal(n, [(1, 0, 0)]) and np.array_equal(t, [(0, 0, 1)])
    # scenes without texture coordinates marshal zeros: every triangle takes this path
    n, t = M.triangle_frames([UNIT_TRI])
    assert np.array_equal(t, [(0, 1, 0)])


def test_model_material_kinds():
    uv = np.array([[0.2, 0.7], [0.9, 0.1]])
    tex = lambda ti, q: np.stack([q[:, 0], q[:, 1], 0.5 + 0 * q[:, 0]], -1) * (ti + 1)  # noqa: E731  (a stand-in map)
    mk = scenes.Material
    one, zero = np.ones((2, 3)), np.zeros((2, 3))
    cases = [
        (mk("l", _abi.MAT_LAMBERTIAN, kd=(0.1, 0.2, 0.3)), [(0.1, 0.2, 0.3)] * 2, zero),
        (mk("lt", _abi.MAT_LAMBERTIAN, kd=(0.1, 0.2, 0.3), texture=0), tex(0, uv), zero),
        (mk("p", _abi.MAT_PHONG, kd=(0.25, 0.5, 0.125), ks=(0.5, 0.25, 0.125), ns=20.0), [(0.75, 0.75, 0.25)] * 2, zero),
        (mk("pt", _abi.MAT_PHONG, kd=(0.25, 0.5, 0.125), ks=(0.5, 0.25, 0.125), ns=20.0, texture=1), 2 * tex(1, uv), zero),
        (mk("m", _abi.MAT_MIRROR, kd=(0.3, 0.3, 0.3)), one, zero),
        (mk("c", _abi.MAT_COOKTORRANCE, kd=(0.8, 0.6, 0.2)), one, zero),
        (mk("e", _abi.MAT_DIFFUSE_LIGHT, kd=(0.5, 0.5, 0.5), emission=(17.0, 12.0, 4.0)), one, [(17.0, 12.0, 4.0)] * 2),
        (mk("d", _abi.MAT_DEBUG, kd=(0.1, 0.4, 0.1)), [(0.1, 0.4, 0.1)] * 2, [(0.1, 0.4, 0.1)] * 2),
        (mk("dt", _abi.MAT_DEBUG, kd=(0.1, 0.4, 0.1), texture=0), tex(0, uv), [(0.1, 0.4, 0.1)] * 2),  # emits Kd, not the map
        (mk("x", _abi.MAT_EMPTY, kd=(0.9, 0.9, 0.9)), one, zero),
    ]
    for m, albedo, emission in cases:
        a, e = M.material_response(m, uv, tex)
        assert np.array_equal(a, np.asarray(albedo, np.float64)), m.name
        assert np.array_equal(e, np.asarray(emission, np.float64)), m.name
    # through records(): material index and type per hit
    data = _one_triangle(UNIT_TRI, IDENT_UV, cases[6][0])
    r = M.records(data, _rays([(0.25, 0.25, 1)], [(0, 0, -1)]), _head([1.0], [0.25], [0.25], [0], [1]))[0]
    assert r["material"] == 0 and r["material_type"] == _abi.MAT_DIFFUSE_LIGHT
    assert np.array_equal(r["emission"], (17.0, 12.0, 4.0)) and np.array_equal(r["albedo"], (1, 1, 1))


def test_model_frames_are_orthonormal_on_the_test_scenes():
    """On the two scenes of the GPU tests every normal and tangent is finite, unit and orthogonal to the other (sanity of the
    vectorised restatement on real meshes)."""
    for data in (scenes.tiny_scene(), scenes.mixed_materials(48, 48)):
        n, t = M.triangle_frames(data.vertices, data.normals, data.texcoords)
        assert np.isfinite(n).all() and np.isfinite(t).all()
        assert np.allclose((n * n).sum(1), 1.0, rtol=0, atol=1e-14) and np.allclose((t * t).sum(1), 1.0, rtol=0, atol=1e-14)
        assert np.abs((n * t).sum(1)).max() < 1e-9
