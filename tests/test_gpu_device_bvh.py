"""GPU tests (-m gpu) of the trees bvh_build_gpu.hip builds, against the fp64 tree model (tests/bvh_model.py) and against
the host builder's trees, on adversarial scenes (identical triangles, clusters of them, flat and zero-thickness scenes,
collapsed Morton cells, wall-sized triangles among tiny ones, sizes around the exhaustive-search boundary and around powers
of two, a soup larger than one k_centroid_bounds pass with far outliers at its end; each also at 1e6 from the origin) and on
cornell, bathroom and a 300k soup.

PRT_VALIDATE_BVH is set for every upload, so a malformed device tree fails the upload before any ray visits it;
PRT_TEST_DUMP_BVH brings the tree back for the model.  Rays: one per triangle aimed at its centroid from just off its plane,
and (on at most 200k triangles) one at each vertex and edge midpoint from a random direction, which graze leaf-box faces.

Prims are compared modulo identical triangles (the first of a set of identical triangles stands for all of them).  A hit
on another primitive than the reference's counts as a tie when that primitive's plane meets the ray at the reference's t
(coplanar overlaps and shared edges); ties are counted and bounded (TIE_BOUND).  The device tree's SAH cost is bounded
relative to the host tree's (SAH_BOUND, from measured ratios).

Against the oracle: centroid rays only, of triangles fp64 resolves at the scene's magnitude (rays through vertices and edge
midpoints sit on the inclusive edge test, where FMA contraction decides hit or miss; they are compared device against host,
bit for bit, where the arithmetic is the same).  At 1e6 the t tolerance is test_gpu_parity's far-from-origin one and the
fp32 mode is not checked: one fp32 ulp there (0.0625) exceeds the triangles.
"""
import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from tests import bvh_model as M
from tests.test_gpu_f32 import check_hits_tier2, trace
from tests.test_gpu_parity import compare_hits

pytestmark = pytest.mark.gpu

SCENES = {
    **{name: fn for name, fn in M.GENERATORS.items()},
    "large_soup": M.large_soup,
    "cornell": lambda: scenes.cornell_box(ball_subdiv=4, width=48, height=48),
    "bathroom": lambda: scenes.bathroom(64, 36, detail=0.3),
    "soup300k": lambda: scenes.triangle_soup(300_000),
}
MOVED = [k for k in M.GENERATORS] + ["large_soup"]  # the adversarial scenes are also built at 1e6 from the origin

# Device / host SAH cost of the wide tree (scenes of n >= 1000), measured on one MI355X, the same at the origin and at 1e6
# (the larger where they differ): identical 1.100, clusters 1.084, flat 1.049, walls 1.178, geometric 1.000, mixed_sizes
# 0.960, soup1024 1.075, soup1025 1.076, soup4096 1.075, soup4097 1.076, large_soup 1.454, cornell 1.187, bathroom 1.332,
# soup300k 1.083.  Bound: the measured ratio + 25 %, rounded up to 0.05.  (k_centroid_bounds taking a single pass measured
# 2.23 / 2.28 on large_soup: its far outliers are left out of the Morton frame.)
SAH_BOUND = {"identical": 1.4, "clusters": 1.4, "flat": 1.35, "walls": 1.5, "geometric": 1.25, "mixed_sizes": 1.2,
             "soup1024": 1.35, "soup1025": 1.35, "soup4096": 1.35, "soup4097": 1.35, "large_soup": 1.85, "cornell": 1.5,
             "bathroom": 1.7, "soup300k": 1.4}
# Exact-t ties between the device and the host tree (a different primitive at a bit-identical t), as a fraction of all the
# rays; measured: flat 14.2 %, walls 3.3 %, geometric@1e6 1.5 %, cornell 2.0 %, bathroom 6.0 % (coplanar overlaps and the
# vertex / edge rays on shared edges), every other scene at most 1 ray.  Bound: about 1.5x the measured fraction.
TIE_BOUND = {"flat": 0.2, "walls": 0.05, "geometric": 0.025, "cornell": 0.03, "bathroom": 0.09}
TIE_BOUND_DEFAULT = 1e-3
ORACLE_RAYS = 200_000


def _params():
    out = []
    for name in SCENES:
        out.append(pytest.param(name, False, id=name))
        if name in MOVED:
            out.append(pytest.param(name, True, id=name + "@1e6"))
    return out


def _build(data, tmp_path, tag, device_bvh, monkeypatch):
    path = str(tmp_path / f"{tag}.bin")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    return sc, M.read_dump(path)


def representatives(vertices):
    """Index of the first triangle with the same nine coordinates, per triangle."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 9)
    _, first, inv = np.unique(v, axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


def aimed_rays(vertices, seed=1, max_tris=200_000):
    """One ray per triangle at its centroid from just off its plane (random side); then, for at most max_tris triangles,
    one ray at each vertex and edge midpoint from a random direction and distance."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    n = v.shape[0]
    c = v.mean(axis=1)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 0.0, 1.0]))  # (triangles degenerate at 1e6: +z)
    size = np.sqrt(0.5 * ln)
    side = np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)
    o1 = c + side * nrm * (1e-3 * size)
    d1 = -side * nrm
    pick = np.sort(rng.choice(n, size=min(n, max_tris), replace=False))
    w = v[pick]
    targets = np.concatenate([w[:, 0], w[:, 1], w[:, 2], 0.5 * (w[:, 0] + w[:, 1]), 0.5 * (w[:, 1] + w[:, 2]),
                              0.5 * (w[:, 2] + w[:, 0])])
    m = targets.shape[0]
    z = 2.0 * rng.random(m) - 1.0
    phi = 2.0 * np.pi * rng.random(m)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d2 = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)
    ext = float((v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0)).max())
    o2 = targets - d2 * (ext * rng.uniform(0.05, 0.5, (m, 1)))
    rays = np.zeros(n + m, dtype=_abi.RAY_DTYPE)
    rays["o"] = np.concatenate([o1, o2])
    rays["d"] = np.concatenate([d1, d2])
    rays["tmin"] = 0.0
    rays["tmax"] = np.inf
    return rays, n


EPS64, EPS32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)


def min_altitude(vertices):
    """Smallest altitude of each triangle (2 area / longest edge)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    area2 = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    longest = np.max([np.linalg.norm(v[:, i] - v[:, (i + 1) % 3], axis=1) for i in range(3)], axis=0)
    return area2 / np.maximum(longest, 1e-300)


def settle_ties(g, ref, rays, vertices, rep):
    """g's prims mapped to representatives; where g hit another primitive than `ref` whose plane meets the ray at ref's t
    (to 1e-9), g takes ref's hit record (a tie).  Returns (patched g, ref with mapped prims, number of ties)."""
    g = g.copy()
    ref = ref.copy()
    for h in (g, ref):
        h["prim"] = np.where(h["prim"] >= 0, rep[np.maximum(h["prim"], 0)], h["prim"])
    diff = np.nonzero((g["prim"] != ref["prim"]) & (g["prim"] >= 0) & (ref["prim"] >= 0))[0]
    if diff.size == 0:
        return g, ref, 0
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)[g["prim"][diff]]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    o, d = rays["o"][diff], rays["d"][diff]
    t = ((v[:, 0] - o) * nrm).sum(-1) / (d * nrm).sum(-1)
    tie = np.abs(t - ref["t"][diff]) <= 1e-9 * np.maximum(1.0, np.abs(ref["t"][diff]))
    k = diff[tie]
    for f in ("prim", "alpha", "beta", "front"):
        g[f][k] = ref[f][k]
    return g, ref, int(k.size)


@pytest.mark.parametrize("name,moved", _params())
def test_device_tree_against_the_model_and_the_host_tree(dev_lib, tmp_path, monkeypatch, name, moved):
    data = SCENES[name]()
    if moved:
        data = M.translated(data)
    n = data.n_tris
    host, th = _build(data, tmp_path, "host", False, monkeypatch)
    dev, td = _build(data, tmp_path, "dev", True, monkeypatch)
    dev2, td2 = _build(data, tmp_path, "dev2", True, monkeypatch)
    assert td.built_on_device == 1 and th.built_on_device == 0
    M.check_tree(th, data.vertices, host.bvh_info())
    rep_d = M.check_tree(td, data.vertices, dev.bvh_info())
    M.check_tree(td2, data.vertices, dev2.bvh_info())
    assert M.canonical(td) == M.canonical(td2), "two device builds of one scene differ beyond node numbering"
    ratio = M.sah_cost(td) / M.sah_cost(th)

    rays, n_centroid = aimed_rays(data.vertices)
    rep = representatives(data.vertices)
    a, b = host.trace_closest(rays), dev.trace_closest(rays)
    # the closest t does not depend on the tree: bit-equal, or a box is too tight somewhere
    assert np.array_equal(a["t"], b["t"]), f"{int((a['t'] != b['t']).sum())} rays differ in t"
    ap = np.where(a["prim"] >= 0, rep[np.maximum(a["prim"], 0)], -1)
    bp = np.where(b["prim"] >= 0, rep[np.maximum(b["prim"], 0)], -1)
    same = ap == bp
    ties = int((~same).sum())
    both = same & (ap >= 0)
    assert np.array_equal(a["alpha"][both], b["alpha"][both]) and np.array_equal(a["front"][both], b["front"][both])

    # the oracle, on at most ORACLE_RAYS centroid rays of triangles that fp64 resolves at their coordinates' magnitude
    mag = max(1.0, float(np.abs(data.vertices).max()))
    tmag = np.maximum(1.0, np.abs(data.vertices).reshape(n, 9).max(axis=1))
    alt = min_altitude(data.vertices) / tmag
    rng = np.random.default_rng(3)
    pool = np.nonzero(alt >= 1e4 * EPS64)[0]
    assert pool.size > 0
    csub = np.sort(rng.choice(pool, size=min(pool.size, ORACLE_RAYS), replace=False))
    orc = oracle.Oracle(data)
    want = orc.trace_closest(rays[csub])
    g, o, oties = settle_ties(b[csub], want, rays[csub], data.vertices, rep)
    # rays through vertices and edge midpoints sit on the inclusive edge test: hit or miss can follow FMA contraction (counted)
    esub = n_centroid + np.sort(rng.choice(rays.shape[0] - n_centroid, size=min(rays.shape[0] - n_centroid, ORACLE_RAYS // 4),
                                           replace=False))
    eflip = int(((b["prim"][esub] >= 0) != (orc.trace_closest(rays[esub])["prim"] >= 0)).sum())

    print(f"[bvh] {name}{'@1e6' if moved else ''}: n {n} nodes {td.n_nodes} depth {td.depth} stack {rep_d['stack_need']} "
          f"sah host {M.sah_cost(th):.3f} device {M.sah_cost(td):.3f} ratio {ratio:.3f} "
          f"ties device/host {ties} of {rays.shape[0]} oracle {oties} of {csub.size} edge flips {eflip} of {esub.size}")
    if not moved:
        compare_hits(g, o)
        # fp32 kernels, tier 2, on the centroid rays of triangles whose altitude is 1e4 fp32 ulps of the coordinates (a
        # sliver's fp32 barycentrics are off by ulp / altitude); not at 1e6, where one fp32 ulp (0.0625) exceeds the triangles
        k32 = csub[alt[csub] >= 1e4 * EPS32]
        assert k32.size > 0
        g32, o32, _ = settle_ties(trace(dev, rays[k32], _abi.PRECISION_F32), want[np.isin(csub, k32)], rays[k32],
                                  data.vertices, rep)
        check_hits_tier2(g32, o32)
    else:
        # far from the origin t = (D - n.o) / (n.d) cancels ~|o| digits: the tolerance of test_scaled_and_translated_scene_hits
        tol = 64 * EPS64 * mag * 1e3 + 1e-12
        assert np.array_equal(g["prim"] >= 0, o["prim"] >= 0)
        hit = o["prim"] >= 0
        assert (np.abs(g["t"][hit] - o["t"][hit]) <= tol * np.maximum(1.0, o["t"][hit])).all()
        assert (g["prim"][hit] == o["prim"][hit]).all()
    assert ties <= max(2, TIE_BOUND.get(name, TIE_BOUND_DEFAULT) * rays.shape[0]), ties
    if n >= 1000:
        assert ratio <= SAH_BOUND[name], ratio


@pytest.mark.parametrize("name", ["identical", "flat"])
def test_moving_geometry_rebuilds_a_valid_tree(dev_lib, tmp_path, monkeypatch, name):
    """update_vertices on an uploaded scene rebuilds the tree on the GPU: the rebuilt tree passes the checker for the new
    positions and gives the hits of a fresh scene made from them."""
    data = M.GENERATORS[name]()
    v = data.vertices * np.array([1.5, 0.75, 1.0]) + np.array([0.25, -0.5, 2.0])
    if name == "flat":
        v[..., 1] = 0.0  # and the flat axis moves: now y
    moved = M.translated(data, (0.0, 0.0, 0.0))
    moved.vertices = v
    path = str(tmp_path / "moved.bin")
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    sc = api.Scene(data).upload(0)
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    sc.update_vertices(v)
    t = M.read_dump(path)
    assert t.built_on_device == 1
    M.check_tree(t, v, sc.bvh_info())
    fresh, tf = _build(moved, tmp_path, "fresh", True, monkeypatch)
    assert M.canonical(t) == M.canonical(tf)
    rays, _ = aimed_rays(v, seed=4)
    a, b = sc.trace_closest(rays), fresh.trace_closest(rays)
    assert np.array_equal(a["t"], b["t"])
    rep = representatives(v)
    assert np.array_equal(np.where(a["prim"] >= 0, rep[np.maximum(a["prim"], 0)], -1),
                          np.where(b["prim"] >= 0, rep[np.maximum(b["prim"], 0)], -1))
