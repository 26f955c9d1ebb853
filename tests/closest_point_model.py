"""numpy restatement of the closest-point contract (include/prt.h, prt_closest_point; kernel in closest_point.hip).

  point_triangle   the region-classifying point-triangle routine of Ericson, Real-Time Collision Detection 5.1.5,
                   vectorised over (query, triangle) pairs and generic over the dtype (float64: the contract's
                   arithmetic, operation for operation what the kernel evaluates without fused multiply-adds;
                   np.longdouble: the reference it is judged against)
  brute_force      every triangle for every query with the (d2, prim) rule, in chunks
  box_bound        the kernel's fp32 lower bound of the squared point-box distance, operation for operation
  queries          the three query classes of the tests: on the surface, near it, uniform in the padded bounds
"""
import numpy as np

FEATURE_NAMES = ("face", "edge v0v1", "edge v1v2", "edge v2v0", "vertex v0", "vertex v1", "vertex v2")


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def point_triangle(p, tri, dtype=np.float64):
    """p (..., 3), tri (..., 3, 3) -> dict of d2, alpha, beta, feature, point, side, all of the leading shape.
    point = v0 + alpha (v1 - v0) + beta (v2 - v0); d2 = |p - point|^2; feature 0 face, 1/2/3 edge v0v1 / v1v2 / v2v0,
    4/5/6 vertex v0 / v1 / v2; side = sign of dot(cross(v1 - v0, v2 - v0), p - point)."""
    p = np.asarray(p, dtype=dtype)
    tri = np.asarray(tri, dtype=dtype)
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    one, zero = dtype(1), dtype(0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        regions = [(d1 <= 0) & (d2 <= 0),                          # vertex v0
                   (d3 >= 0) & (d4 <= d3),                         # vertex v1
                   (vc <= 0) & (d1 >= 0) & (d3 <= 0),              # edge v0v1
                   (d6 >= 0) & (d5 <= d6),                         # vertex v2
                   (vb <= 0) & (d2 >= 0) & (d6 <= 0),              # edge v2v0
                   (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]  # edge v1v2
        feature = np.select(regions, [4, 5, 1, 6, 3, 2], 0).astype(np.int32)
        w12 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = one / (va + vb + vc)
        z, o = np.zeros_like(d1), np.ones_like(d1)
        alpha = np.select(regions, [z, o, d1 / (d1 - d3), z, z, one - w12], vb * denom)
        beta = np.select(regions, [z, z, z, o, d2 / (d2 - d6), w12], vc * denom)
        point = a + alpha[..., None] * ab + beta[..., None] * ac
        diff = p - point
        dist2 = _dot(diff, diff)
        s = _dot(_cross(ab, ac), diff)
    side = np.where(s > zero, 1, np.where(s < zero, -1, 0)).astype(np.int32)
    return {"d2": dist2, "alpha": alpha, "beta": beta, "feature": feature, "point": point, "side": side}


def brute_force(points, vertices, max_dist=np.inf, chunk=256):
    """The contract's answer for every query: the minimum of (d2, prim) over ALL triangles with d2 <= max_dist^2, in fp64.
    Returns dict of d2 (inf on a miss), prim (-1), alpha, beta, feature (-1), point, side.

    Every triangle is considered for every query; the routine itself runs on the pairs that can still win: a pair is set
    aside only when a lower bound of its distance (to the triangle's bounding box) exceeds an upper bound of the query's
    answer (its distance to the nearest first corner) by more than a slack that no winner and no tie can make up: 1e-9
    relative for the roundings of the two bounds, plus 2e-11 S absolute - twice ten times the 1e-12 S by which the
    routine's COMPUTED distance can differ from the exact one on sliver triangles (S = scene_scale)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    n, nt = points.shape[0], v.shape[0]
    lim = np.broadcast_to(np.asarray(max_dist, dtype=np.float64), (n,))
    lim2 = lim * lim
    out = {"d2": np.full(n, np.inf), "prim": np.full(n, -1, np.int32), "alpha": np.zeros(n), "beta": np.zeros(n),
           "feature": np.full(n, -1, np.int32), "point": np.zeros((n, 3)), "side": np.zeros(n, np.int32)}
    if nt == 0:
        return out
    # bitwise copies of a triangle have one d2 (a pure function of the query and the corners) and the lowest index wins:
    # they are represented by their first occurrence
    _, prim_of = np.unique(v.reshape(nt, 9), axis=0, return_index=True)
    prim_of = np.sort(prim_of)
    v = v[prim_of]
    lo, hi = v.min(axis=1), v.max(axis=1)
    slack = 2e-11 * scene_scale(v, points)
    for s in range(0, n, chunk):
        p = points[s:s + chunk]
        gap = np.maximum(np.maximum(lo[None] - p[:, None], p[:, None] - hi[None]), 0.0)
        lb = (gap * gap).sum(-1)
        d0 = p[:, None] - v[None, :, 0]
        ub = (d0 * d0).sum(-1).min(axis=1)
        qi, ti = np.nonzero(np.sqrt(lb) <= (np.sqrt(ub) * (1.0 + 1e-9) + slack)[:, None])
        r = point_triangle(p[qi], v[ti])
        ok = r["d2"] <= lim2[s + qi]  # (a NaN d2 - a degenerate triangle - is no candidate)
        qi, ti = qi[ok], ti[ok]
        d2 = r["d2"][ok]
        order = np.lexsort((ti, d2, qi))
        first = np.ones(order.size, dtype=bool)
        first[1:] = qi[order][1:] != qi[order][:-1]
        win = order[first]
        at = s + qi[win]
        out["d2"][at] = d2[win]
        out["prim"][at] = prim_of[ti[win]]  # (prim_of ascends: ordering by ti above is ordering by prim)
        for k in ("alpha", "beta", "feature", "point", "side"):
            out[k][at] = r[k][ok][win]
    return out


# ---- the kernel's box bound (closest_point.hip, box_bound), every operation an individually rounded fp32 one
PAD = np.float32(2.0 ** -21)
SHRINK = np.float32(1.0 - 2.0 ** -20)
CLAMP = np.float32(1e18)


def grid_extent(step):
    """DScene::slab_scale: the grid's largest extent, rounded up."""
    e = max(65535.0 * float(s) for s in step)
    return np.nextafter(np.float32(e), np.float32(np.inf))


def box_bound(p, qlo, qhi, origin, step, extent):
    """p (n, 3) float64, qlo / qhi (n, 3) grid indices, origin / step (3,) float32, extent float32 -> (n,) float32."""
    p = np.asarray(p, dtype=np.float64)
    g0 = np.asarray(origin, dtype=np.float32)
    gs = np.asarray(step, dtype=np.float32)
    E = np.float32(extent)
    with np.errstate(over="ignore", invalid="ignore"):
        r = (p - g0.astype(np.float64)).astype(np.float32)
        pad = (np.abs(r) + E) * PAD
        lo = np.asarray(qlo).astype(np.float32) * gs
        hi = np.asarray(qhi).astype(np.float32) * gs
        d = np.maximum(np.maximum(lo - r, r - hi), np.float32(0))
        d = np.minimum(np.maximum(d - pad, np.float32(0)), CLAMP)
        sq = d * d
        return ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) * SHRINK


# ---- query classes
def scene_scale(vertices, points=None):
    """S = max(1, largest |coordinate| of the scene and the queries)."""
    s = max(1.0, float(np.abs(vertices).max()) if np.size(vertices) else 0.0)
    return s if points is None or not np.size(points) else max(s, float(np.abs(points).max()))


def queries(vertices, n, seed):
    """dict class -> ((n, 3) points, (n,) triangle each was made from, or -1): `surface` points on random triangles (uniform
    barycentrics), `near` those displaced by up to 1 % of the extent in a random direction, `box` uniform in the bounds
    padded by 10 % of the extent."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    t = rng.integers(0, v.shape[0], n)
    u = rng.random((n, 2))
    flip = u.sum(1) > 1.0
    u[flip] = 1.0 - u[flip]
    on = v[t, 0] + u[:, :1] * (v[t, 1] - v[t, 0]) + u[:, 1:] * (v[t, 2] - v[t, 0])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = on + d * (rng.random((n, 1)) * 0.01 * ext)
    box = lo - 0.1 * ext + rng.random((n, 3)) * (hi - lo + 0.2 * ext)
    return {"surface": (on, t), "near": (near, t), "box": (box, np.full(n, -1))}


# ---- the scenes and queries the CPU and GPU tests share
def _scenes():
    from pooraytracer_amd import scenes
    from tests import bvh_model as M
    return {
        "cornell": lambda: scenes.cornell_box(ball_subdiv=3, width=64, height=64),
        "bathroom": lambda: scenes.bathroom(width=64, height=36, detail=0.15),
        "mixed_materials": scenes.mixed_materials,
        "triangle_soup": lambda: scenes.triangle_soup(4096),
        "identical": M.identical,
        "clusters": M.clusters,
        "flat": M.flat,
        "walls": M.walls,
        "geometric": M.geometric,
        "mixed_sizes": M.mixed_sizes,
        "soup_at_1e6": lambda: M.translated(M.soup(4096)),
    }


SCENE_NAMES = ("cornell", "bathroom", "mixed_materials", "triangle_soup", "identical", "clusters", "flat", "walls", "geometric",
               "mixed_sizes", "soup_at_1e6")
N_QUERIES = 4096
CLASSES = ("surface", "near", "box")
_cache = {}


def scene(name):
    """The scene's data, made once per process."""
    if ("scene", name) not in _cache:
        _cache[("scene", name)] = _scenes()[name]()
    return _cache[("scene", name)]


def scene_queries(name):
    """N_QUERIES points per class on scene `name` (one fixed seed per scene), made once per process."""
    if ("queries", name) not in _cache:
        _cache[("queries", name)] = queries(scene(name).vertices, N_QUERIES, 1000 + SCENE_NAMES.index(name))
    return _cache[("queries", name)]


def reference(name, cls, vertices=None, tag=None):
    """brute_force for one query class of a scene (on `vertices`, cached under `tag`, when the geometry has moved),
    computed once per process and shared; callers do not modify it."""
    key = ("reference", name, cls, tag)
    if key not in _cache:
        v = scene(name).vertices if vertices is None else vertices
        _cache[key] = brute_force(scene_queries(name)[cls][0], v)
    return _cache[key]
