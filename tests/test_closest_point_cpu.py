"""CPU tests of the closest-point queries (prt_closest_point, include/prt.h): the numpy model is a fit reference, the kernel's
fp32 box bound is conservative with exact rational arithmetic as the judge, the ABI is additive, and everything that can be
said without a GPU (the switch, the refusals, the wrapper's argument checks)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from tests import closest_point_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the model
# The two generators whose triangles are ARBITRARY RANDOM SLIVERS: three random points of a small cell, flattened into a
# plane (tests/bvh_model.py: flat, walls).  For a query ON such a triangle the fp64 routine's own error - the face region's
# ratio of nearly cancelling products - is not 1e-13 S: on arbitrary random slivers it was measured to reach 1.4e-12 S
# when the 1e-13 S figure was taken (and 1.17e-12 S on `flat`, 1.24e-12 S on `walls` here).  Their on-surface class is
# therefore held to SLIVER_CEILING = 2 x 1.4e-12 S: that measured maximum, with a factor of two because it is the
# maximum of one sample of slivers, not a bound.  Their `near` and `box` classes, whose queries lie off the triangle,
# are held to 1e-13 S like every class of every other scene.
# On those two scenes the GPU tests' 1e-12 S against the float64 model therefore shows agreement with the contract's
# arithmetic (the kernel evaluates the model's operations in the model's order), not closeness to the exact distance.
SLIVER_SCENES = ("flat", "walls")
SLIVER_CEILING = 2.8e-12
FIT = 1e-13


def _fit(v, queries_by_class, own, name):
    """Worst float64-vs-longdouble disagreement of distance and point per class, in units of S; asserts nothing."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: nothing to judge the fp64 routine with")
    worst = {}
    for cls, p in queries_by_class.items():
        S = CM.scene_scale(v, p)
        a = CM.point_triangle(p, v[own])
        b = CM.point_triangle(p, v[own], dtype=np.longdouble)
        dist = np.abs(np.sqrt(a["d2"]) - np.sqrt(b["d2"]).astype(np.float64)).max() / S
        point = np.abs(a["point"] - b["point"].astype(np.float64)).max() / S
        print(f"{name} {cls}: |dist - dist_ld| <= {dist:.2e} S, |point - point_ld| <= {point:.2e} S")
        worst[cls] = max(dist, point)
    return worst


@pytest.mark.parametrize("name", CM.SCENE_NAMES)
def test_model_is_a_fit_reference(name):
    """On the inputs the GPU tests use, the float64 and np.longdouble evaluations of the routine agree to 1e-13 S on every
    (query, own-triangle) pair: distance and point.  (`box` queries, which belong to no triangle, are paired with the
    triangle of the same index in the draw.)  The on-surface class of the two sliver generators is held to
    SLIVER_CEILING instead: see SLIVER_SCENES."""
    v = CM.scene(name).vertices
    q = CM.scene_queries(name)
    worst = _fit(v, {cls: q[cls][0] for cls in CM.CLASSES}, q["surface"][1], name)
    for cls in CM.CLASSES:
        bound = SLIVER_CEILING if (name in SLIVER_SCENES and cls == "surface") else FIT
        assert worst[cls] <= bound, (name, cls, worst[cls], bound)


@pytest.mark.parametrize("name,make", [("triangle_soup(20000)", lambda: scenes.triangle_soup(20000)),
                                       ("cornell_box(ball_subdiv=3)", lambda: scenes.cornell_box(ball_subdiv=3, width=32, height=32)),
                                       ("bathroom(detail=0.15)", lambda: scenes.bathroom(width=64, height=36, detail=0.15)),
                                       ("mixed_materials", scenes.mixed_materials)])
def test_model_is_a_fit_reference_on_300k_pairs(name, make):
    """The same agreement on 300,000 pairs per class of the four scenes it was first measured on (worst case there:
    4.2e-14 S, on-surface on the soup); no pair is left out."""
    v = make().vertices
    q = CM.queries(v, 300_000, 5)
    worst = _fit(v, {cls: q[cls][0] for cls in CM.CLASSES}, q["surface"][1], name)
    assert max(worst.values()) <= 1e-13, worst


def test_model_regions_of_one_triangle():
    """Seven Voronoi regions of one triangle, both sides: feature, barycentrics and side as constructed."""
    from tests.bvh_model import _TRI
    p, want = region_queries(_TRI)
    r = CM.point_triangle(p, np.broadcast_to(_TRI, (p.shape[0], 3, 3)))
    assert np.array_equal(r["feature"], want["feature"])
    assert np.array_equal(r["side"], want["side"])
    vert = r["feature"] >= 4
    corners = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    assert np.array_equal(np.stack([r["alpha"], r["beta"]], 1)[vert], corners[r["feature"][vert] - 4])
    assert np.all(r["beta"][r["feature"] == 1] == 0) and np.all(r["alpha"][r["feature"] == 3] == 0)
    e12 = r["feature"] == 2
    assert np.array_equal(r["alpha"][e12], 1.0 - r["beta"][e12])


def region_queries(tri):
    """Points well inside each Voronoi region of `tri`, on both sides of its plane: (points, dict feature / side)."""
    a, b, c = tri
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    cen = (a + b + c) / 3.0

    def outward(u, w, other):  # in-plane unit normal of edge uw pointing away from `other`
        e = w - u
        d = np.cross(e, n)
        d /= np.linalg.norm(d)
        return d if np.dot(d, other - u) < 0 else -d

    base = [(cen, 0),
            (0.5 * (a + b) + 0.3 * outward(a, b, c), 1), (0.5 * (b + c) + 0.3 * outward(b, c, a), 2),
            (0.5 * (c + a) + 0.3 * outward(c, a, b), 3),
            (a + 0.5 * (a - cen), 4), (b + 0.5 * (b - cen), 5), (c + 0.5 * (c - cen), 6)]
    pts, feat, side = [], [], []
    for q, f in base:
        for s in (1, -1):
            pts.append(q + s * 0.2 * n)
            feat.append(f)
            side.append(s)
    return np.array(pts), {"feature": np.array(feat, np.int32), "side": np.array(side, np.int32)}


# ------------------------------------------------------------------------------------------------- the box bound
def _exact_box_d2(p, qlo, qhi, origin, step):
    """Squared distance from p to the decoded box [origin + qlo step, origin + qhi step], exactly."""
    d2 = Fraction(0)
    for a in range(3):
        g0, gs, x = Fraction(float(origin[a])), Fraction(float(step[a])), Fraction(float(p[a]))
        lo, hi = g0 + int(qlo[a]) * gs, g0 + int(qhi[a]) * gs
        gap = max(lo - x, x - hi, Fraction(0))
        d2 += gap * gap
    return d2


# the fp64 side the pad is derived for: d2 = |p - point|^2 carries a few fp64 roundings; the bound keeps 2^-22 below the
# exact value (the derivation at box_bound, closest_point.hip, gives 2^-21)
_MARGIN = 1 - Fraction(1, 1 << 22)


def _check_bound(p, qlo, qhi, origin, step):
    lb = CM.box_bound(p, qlo, qhi, origin, step, CM.grid_extent(step))
    assert np.all(np.isfinite(lb)) and np.all(lb >= 0)
    for i in range(p.shape[0]):
        exact = _exact_box_d2(p[i], qlo[i], qhi[i], origin, step)
        assert Fraction(float(lb[i])) <= exact * _MARGIN, (p[i], qlo[i], qhi[i], origin, step, float(lb[i]), float(exact))
    return lb


def _random_boxes(rng, n):
    lo = rng.integers(0, 65536, (n, 3))
    hi = rng.integers(0, 65536, (n, 3))
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    one = rng.random(n) < 0.1  # one-cell boxes
    hi[one] = np.minimum(lo[one] + 1, 65535)
    lo[one] = hi[one] - 1
    return lo, hi


GRIDS = [((0.0, 0.0, 0.0), (1.0 / 65535, 1.0 / 65535, 1.0 / 65535)),
         ((-0.3, 2.5, -7.25), (3.1e-5, 1.7e-6, 9.0e-4)),
         ((1.0e6, -1.0e6, 1.0e6), (1.6e-5, 1.6e-5, 2.0e-5)),
         ((-1.0e6, 1.0e6, -1.0e6), (4.0e-3, 1.0e-7, 4.0e-3))]


@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_box_bound_is_conservative_on_random_points(grid):
    """2 10^5 random points against random boxes, 50,000 on each of four grids (two of them at +-1e6): the bound never
    exceeds the exact squared distance to the decoded box, less the margin; and it is no vacuous bound."""
    rng = np.random.default_rng(77 + grid)
    per = 50_000
    origin, step = np.float32(GRIDS[grid][0]), np.float32(GRIDS[grid][1])
    g, st = origin.astype(np.float64), step.astype(np.float64)
    qlo, qhi = _random_boxes(rng, per)
    p = g + (rng.random((per, 3)) * 1.5 - 0.25) * (65535.0 * st)
    lb = _check_bound(p, qlo, qhi, origin, step)
    gap = np.maximum(np.maximum(g + qlo * st - p, p - (g + qhi * st)), 0.0)
    far = (gap > st).any(axis=1)  # outside the box by more than one grid step
    outside, positive = int(far.sum()), int((lb[far] > 0).sum())
    print(f"bound positive for {positive} of {outside} points more than a grid step outside their box")
    assert outside > per // 4 and positive > outside // 2


def test_box_bound_is_conservative_on_adversarial_points():
    """A point on a face, edge or corner plane of the box; 1 ulp outside; 1e6 extents away; grid origins at +-1e6; one-cell
    boxes."""
    rng = np.random.default_rng(78)
    for origin, step in GRIDS:
        origin, step = np.float32(origin), np.float32(step)
        g, st = origin.astype(np.float64), step.astype(np.float64)
        ext = 65535.0 * st
        n = 600
        qlo, qhi = _random_boxes(rng, n)
        qhi[:100] = np.minimum(qlo[:100] + 1, 65535)  # one-cell boxes
        qlo[:100] = qhi[:100] - 1
        lo, hi = g + qlo * st, g + qhi * st  # (fp64 roundings of the planes: the points are near them, the judge is exact)
        inside = lo + rng.random((n, 3)) * (hi - lo)
        pts, boxes = [], []
        for k in (1, 2, 3):  # on k of the box's planes: face, edge, corner
            p = inside.copy()
            for a in range(k):
                upper = rng.random(n) < 0.5
                p[:, a] = np.where(upper, hi[:, a], lo[:, a])
            pts.append(p)
            boxes.append((qlo, qhi))
            for towards in (np.inf, -np.inf):  # and 1 ulp to either side of those planes
                q = p.copy()
                q[:, :k] = np.nextafter(p[:, :k], towards)
                pts.append(q)
                boxes.append((qlo, qhi))
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(g + 0.5 * ext + d * 1e6 * ext.max())  # 1e6 extents away
        boxes.append((qlo, qhi))
        for p, (bl, bh) in zip(pts, boxes):
            _check_bound(p, bl, bh, origin, step)


# ------------------------------------------------------------------------------------------------- ABI
def test_abi_is_additive(prt_lib, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "prt.h"\nint main(){printf("%d %zu %zu\\n",PRT_ABI_VERSION,sizeof(PrtPointQuery),'
                   "sizeof(PrtClosestPoint));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["6", "32", "64"]
    assert _abi.PRT_ABI_VERSION == 6 and prt_lib.prt_abi_version() == 6
    assert C.sizeof(_abi.PrtPointQuery) == _abi.POINT_QUERY_DTYPE.itemsize == 32
    assert C.sizeof(_abi.PrtClosestPoint) == _abi.CLOSEST_POINT_DTYPE.itemsize == 64
    for f, _ in _abi.PrtClosestPoint._fields_:
        assert getattr(_abi.PrtClosestPoint, f).offset == _abi.CLOSEST_POINT_DTYPE.fields[f][1]
    for name in ("prt_scene_set_distance_queries", "prt_scene_get_distance_queries", "prt_closest_point", "prt_closest_point_device"):
        assert name in _abi.EXPORTS and hasattr(prt_lib, name)


# ------------------------------------------------------------------------------------------------- without a GPU
def test_switch_works_without_upload(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    assert sc.distance_queries is False
    sc.distance_queries = True
    assert sc.distance_queries is True
    sc.update_vertices(scenes.tiny_scene().vertices * 2.0)  # survives a (host-only) update
    assert sc.distance_queries is True
    sc.distance_queries = False
    assert sc.distance_queries is False
    assert prt_lib.prt_scene_set_distance_queries(None, 1) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_get_distance_queries(sc._h, None) == _abi.PRT_E_INVALID
    sc.close()


def test_queries_fail_loudly_without_upload(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    sc.distance_queries = True
    p = np.zeros((3, 3))
    with pytest.raises(api.PrtError) as e:
        sc.closest_point(p)
    assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_closest_point:" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.closest_point_device(256, 3, 512)
    assert e.value.code == _abi.PRT_E_NO_DEVICE and "prt_closest_point_device:" in str(e.value)
    with pytest.raises(api.PrtError) as e:
        sc.closest_point(np.zeros((0, 3)))  # no query, still no device
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_host_call_refuses_a_non_finite_point(prt_lib, bad):
    sc = api.Scene(scenes.tiny_scene())
    p = np.zeros((4, 3))
    p[2, 1] = bad
    with pytest.raises(api.PrtError) as e:
        sc.closest_point(p)
    assert e.value.code == _abi.PRT_E_INVALID and "prt_closest_point" in str(e.value) and "query 2" in str(e.value)
    sc.close()


@pytest.mark.parametrize("bad", [-1.0, -1e-300, np.nan, -np.inf])
def test_host_call_refuses_a_bad_radius(prt_lib, bad):
    sc = api.Scene(scenes.tiny_scene())
    md = np.ones(4)
    md[1] = bad
    with pytest.raises(api.PrtError) as e:
        sc.closest_point(np.zeros((4, 3)), max_dist=md)
    assert e.value.code == _abi.PRT_E_INVALID and "max_dist" in str(e.value)
    for ok in (0.0, np.inf):  # legal radii get as far as the missing device
        with pytest.raises(api.PrtError) as e:
            sc.closest_point(np.zeros((4, 3)), max_dist=ok)
        assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc.close()


def test_wrapper_raises_shape_and_dtype_errors_before_any_call(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    with pytest.raises(TypeError):
        sc.closest_point([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError):
        sc.closest_point(np.zeros((2, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        sc.closest_point(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        sc.closest_point(np.zeros(3))
    with pytest.raises(ValueError):
        sc.closest_point(np.zeros((2, 3)), max_dist=np.ones(3))
    with pytest.raises(TypeError):
        sc.closest_point(np.zeros((2, 3)), max_dist="far")
    sc.close()
