"""A hit certifier and adversarial ray batches (numpy, CPU; used by test_hit_certifier_cpu.py, test_gpu_hit_edges.py and
tools/f32_accounting.py).

certify() takes a ray batch, the oracle's closest hits Y = (prim, t), a kernel's hits X = (prim', t'), the scene's vertices
and the unit roundoff u of the kernel's arithmetic (2^-24 fp32, 2^-53 fp64) and accounts for EVERY ray on which the two
disagree: a disagreement is explained when the exact arithmetic puts the ray within a first-order rounding bound of the
decision the kernel took the other way, and unexplained otherwise.  A budget ("1e-4 of the rays may be off") lets a
traversal lose robust hits; this does not.

For a (ray, triangle) pair the expressions of DTriT / tri_test (csrc/prt_types.h, csrc/prt_device.h) are evaluated above
the kernel's precision (fp64 for u = 2^-24, long double for u = 2^-53):

    n = n_un / |n_un|, D = n . v0, w = n_un / |n_un|^2, A = e1 x w, B = w x e0, a0 = v0 . A, b0 = v0 . B
    t = (D - n . o) / (n . d), p = o + d t, alpha = p . A - a0, beta = p . B - b0

with the running error bound (c = 8: the input roundings of ray and record, three-term dot products, the reciprocal and
the product each contribute at most one or two u of the magnitudes below)

    E_num = c u (|D| + sum |n_i o_i|)            E_den = c u sum |n_i d_i|
    dt    = (E_num + |t| E_den) / |n . d| + c u |t|
    dp_i  = c u (|o_i| + |d_i t|) + |d_i| dt
    e_a   = c u (sum |p_i A_i| + |a0|) + sum |A_i| dp_i         (e_b likewise)

Verdict per ray (SAME_TOL = prt.h's tier-2 hit figure for fp32, the fp64 parity figure for fp64):
  same primitive        |t' - t| <= max(SAME_TOL max(1, t), dt)
  kernel lost Y         (a miss, or t' > t + dt): Y must be MARGINAL — alpha <= e_a, or beta <= e_b, or alpha + beta >=
                        1 - e_a - e_b, or t within dt of tmin / tmax, or |n . d| within E_den of 1e-8
  kernel returned X!=Y  X, evaluated for this ray, must be ALMOST A HIT — alpha >= -e_a, beta >= -e_b, alpha + beta <=
                        1 + e_a + e_b, t_X in [tmin - dt, tmax + dt], |n . d| >= 1e-8 - E_den and |t_X - t'| <= dt
A ray that lost Y and got a farther X needs both.  Anything else is unexplained.
"""
import dataclasses

import numpy as np

from pooraytracer_amd import _abi, scenes

U32, U64 = 2.0 ** -24, 2.0 ** -53
C_BOUND = 8.0
SAME_TOL = {U32: 1e-5, U64: 1e-12}
DENOM_MIN = 1e-8                        # tri_test's |n . d| threshold
KINDS = ("lost", "farther", "tie", "nearer", "phantom")
# lost: the kernel missed where the oracle hit; farther: it returned another primitive behind Y; tie: another primitive
# within dt of Y; nearer: another primitive in front of Y; phantom: a hit where the oracle missed.


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def tri_records(vertices, dtype=np.float64):
    """DTriT's fields for every triangle of `vertices` (T, 3, 3), computed in `dtype`."""
    v = np.asarray(vertices).astype(dtype)
    v0, e0, e1 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nu = _cross(e0, e1)
    nn = (nu * nu).sum(-1, keepdims=True)
    n, w = nu / np.sqrt(nn), nu / nn
    A, B = _cross(e1, w), _cross(w, e0)
    rec = {"n": n, "D": (n * v0).sum(-1), "A": A, "a0": (v0 * A).sum(-1), "B": B, "b0": (v0 * B).sum(-1)}
    assert all(np.isfinite(np.asarray(x, np.float64)).all() for x in rec.values()), "degenerate triangle"
    return rec


def evaluate(rec, prim, o, d, u):
    """tri_test's quantities and their error bounds for ray i against triangle prim[i], in the dtype of `rec`."""
    dtype = rec["D"].dtype
    o, d, cu = o.astype(dtype), d.astype(dtype), dtype.type(C_BOUND * u)
    n, D, A, a0, B, b0 = (rec[k][prim] for k in ("n", "D", "A", "a0", "B", "b0"))
    with np.errstate(all="ignore"):
        nd = (n * d).sum(-1)
        t = (D - (n * o).sum(-1)) / nd
        e_num = cu * (np.abs(D) + np.abs(n * o).sum(-1))
        e_den = cu * np.abs(n * d).sum(-1)
        dt = (e_num + np.abs(t) * e_den) / np.abs(nd) + cu * np.abs(t)
        p = o + d * t[:, None]
        dp = cu * (np.abs(o) + np.abs(d * t[:, None])) + np.abs(d) * dt[:, None]
        alpha = (p * A).sum(-1) - a0
        beta = (p * B).sum(-1) - b0
        e_a = cu * (np.abs(p * A).sum(-1) + np.abs(a0)) + (np.abs(A) * dp).sum(-1)
        e_b = cu * (np.abs(p * B).sum(-1) + np.abs(b0)) + (np.abs(B) * dp).sum(-1)
    return {"t": t, "nd": np.abs(nd), "alpha": alpha, "beta": beta, "dt": dt, "e_a": e_a, "e_b": e_b, "e_den": e_den}


def _marginal_ratio(E, tmin, tmax):
    """How far inside its decisions a hit sits, in units of the bound: <= 1 when some rounding could have rejected it."""
    with np.errstate(all="ignore"):
        r = np.stack([E["alpha"] / E["e_a"], E["beta"] / E["e_b"], (1 - E["alpha"] - E["beta"]) / (E["e_a"] + E["e_b"]),
                      np.abs(E["t"] - tmin) / E["dt"], np.abs(tmax - E["t"]) / E["dt"],
                      np.abs(E["nd"] - DENOM_MIN) / E["e_den"]])
    return np.where(np.isnan(r), np.inf, r).min(0)


def _almost_hit_ratio(E, tmin, tmax, t_kernel):
    """How far outside a triangle test's decisions a returned hit sits: <= 1 when some rounding could have accepted it."""
    with np.errstate(all="ignore"):
        r = np.stack([-E["alpha"] / E["e_a"], -E["beta"] / E["e_b"], (E["alpha"] + E["beta"] - 1) / (E["e_a"] + E["e_b"]),
                      (tmin - E["t"]) / E["dt"], (E["t"] - tmax) / E["dt"], (DENOM_MIN - E["nd"]) / E["e_den"],
                      np.abs(E["t"] - t_kernel) / E["dt"]])
    return np.where(np.isnan(r), np.inf, r).max(0)


@dataclasses.dataclass
class Verdict:
    unexplained: np.ndarray   # indices of the rays whose disagreement no rounding explains
    ratio: float              # largest margin / bound among the explained rays (<= 1 by construction)
    same_ratio: float         # largest |t' - t| / dt among the rays with the same primitive (not floored by SAME_TOL)
    kinds: dict               # kind -> number of rays on which the primitive differs
    disagree: int             # sum of the kinds
    ratio_of: np.ndarray      # per ray: the ratio its verdict rests on (inf where unexplained)

    def summary(self):
        return {"unexplained": int(self.unexplained.size), "worst_ratio": self.ratio, "same_prim_dt_ratio": self.same_ratio,
                "disagree": self.disagree, **self.kinds}


def certify(rays, want, got, vertices, u):
    """Account for every ray of `rays` on which the kernel's hits `got` differ from the oracle's `want` (module docstring)."""
    dtype = np.longdouble if u < 2.0 ** -40 else np.float64
    rec = tri_records(vertices, dtype)
    n = rays.shape[0]
    o, d = rays["o"], rays["d"]
    tmin, tmax = rays["tmin"].astype(dtype), rays["tmax"].astype(dtype)
    y, x = want["prim"].astype(np.int64), got["prim"].astype(np.int64)
    ty, tx = want["t"].astype(dtype), got["t"].astype(dtype)
    hy, hx = y >= 0, x >= 0
    ratio = np.zeros(n)
    kind = np.full(n, -1)

    EY = {k: np.full(n, np.nan, dtype) for k in ("t", "nd", "alpha", "beta", "dt", "e_a", "e_b", "e_den")}
    EX = {k: v.copy() for k, v in EY.items()}
    for E, h, prim in ((EY, hy, y), (EX, hx, x)):
        for k, val in evaluate(rec, prim[h], o[h], d[h], u).items():
            E[k][h] = val

    same = hy & hx & (x == y)
    with np.errstate(all="ignore"):
        floor = SAME_TOL[u] * np.maximum(1.0, ty)
        gap = np.abs(tx - ty)
        ratio[same] = (gap / np.maximum(floor, EY["dt"]))[same]
        same_ratio = float((gap / EY["dt"])[same].max()) if same.any() else 0.0
        farther = hy & hx & ~same & (tx > ty + EY["dt"])
        nearer = hy & hx & ~same & (tx < ty - EY["dt"])
    lost = hy & ~hx
    phantom = ~hy & hx
    tie = hy & hx & ~same & ~farther & ~nearer
    for i, m in enumerate((lost, farther, tie, nearer, phantom)):
        kind[m] = i
    need_marginal = lost | farther
    need_almost = farther | tie | nearer | phantom
    ratio[need_marginal] = _marginal_ratio(EY, tmin, tmax)[need_marginal]
    ratio[need_almost] = np.maximum(ratio, _almost_hit_ratio(EX, tmin, tmax, tx))[need_almost]
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    bad = ratio > 1.0
    kinds = {k: int((kind == i).sum()) for i, k in enumerate(KINDS)}
    return Verdict(np.flatnonzero(bad), float(ratio[~bad].max()) if (~bad).any() else 0.0, same_ratio, kinds,
                   int((kind >= 0).sum()), np.where(bad, np.inf, ratio))


# ------------------------------------------------------------------------------------------ brute force (CPU tests)
def brute_force_closest(vertices, rays, dtype, drop=None, chunk=256):
    """The closest hit of every ray over ALL triangles, tri_test's expressions evaluated in `dtype` operation by operation:
    the records are computed in float64 and rounded to `dtype` (as the fp32 tables are converted from the fp64 ones), the
    ray is rounded to `dtype` (a long-double pass computes its records in long double).  `drop`: a triangle left out.  Returns a HIT_DTYPE array (alpha, beta included)."""
    wide = np.longdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.float64
    rec = {k: v.astype(dtype) for k, v in tri_records(vertices, wide).items()}
    n, D, A, a0, B, b0 = (rec[k] for k in ("n", "D", "A", "a0", "B", "b0"))
    out = np.zeros(rays.shape[0], dtype=_abi.HIT_DTYPE)
    thr = dtype(DENOM_MIN)

    def dot3(ax, ay, az, b):  # (R, 1) components against (T, 3): ((x + y) + z), one rounding per operation
        return (ax * b[None, :, 0] + ay * b[None, :, 1]) + az * b[None, :, 2]

    for s in range(0, rays.shape[0], chunk):
        r = rays[s:s + chunk]
        o, d = r["o"].astype(dtype)[:, None, :], r["d"].astype(dtype)[:, None, :]
        tmin, tmax = r["tmin"].astype(dtype)[:, None], r["tmax"].astype(dtype)[:, None]
        with np.errstate(all="ignore"):
            nd = dot3(d[..., 0], d[..., 1], d[..., 2], n)
            t = (D[None, :] - dot3(o[..., 0], o[..., 1], o[..., 2], n)) / nd
            ok = (np.abs(nd) >= thr) & (tmin <= t) & (t <= tmax)
            px, py, pz = (o[..., k] + d[..., k] * t for k in range(3))
            alpha = dot3(px, py, pz, A) - a0[None, :]
            beta = dot3(px, py, pz, B) - b0[None, :]
            ok &= (alpha >= 0) & (beta >= 0) & (alpha + beta <= 1)
        if drop is not None:
            ok[:, drop] = False
        t = np.where(ok, t, np.inf)
        best = t.argmin(1)
        rows = np.arange(r.shape[0])
        hit = ok[rows, best]
        o_ = out[s:s + chunk]
        o_["prim"] = np.where(hit, best, -1)
        o_["t"] = np.where(hit, t[rows, best], r["tmax"])
        o_["alpha"] = np.where(hit, alpha[rows, best], 0)
        o_["beta"] = np.where(hit, beta[rows, best], 0)
    return out


# ------------------------------------------------------------------------------------------ adversarial ray batches
DELTAS = np.array([0.0, 2.0 ** -26, -2.0 ** -26, 2.0 ** -22, -2.0 ** -22, 2.0 ** -18, -2.0 ** -18, 2.0 ** -14])


def _targets(data, n, rng):
    """n points on (s = 0 for an eighth: at the first vertex of) a random edge of a random triangle, moved along the in-plane
    edge normal (positive: into the triangle) by DELTAS x the scene's extent."""
    v = np.asarray(data.vertices, dtype=np.float64)
    lo, hi = data.bounds()
    extent = float((hi - lo).max())
    tri, e = rng.integers(0, v.shape[0], n), rng.integers(0, 3, n)
    a, b, c = v[tri, e], v[tri, (e + 1) % 3], v[tri, (e + 2) % 3]
    s = np.where(rng.random(n) < 0.125, 0.0, rng.random(n))
    ab = b - a
    m = (c - a) - ab * (((c - a) * ab).sum(-1) / (ab * ab).sum(-1))[:, None]
    m /= np.linalg.norm(m, axis=-1, keepdims=True)
    delta = DELTAS[rng.integers(0, DELTAS.size, n)]
    return a + s[:, None] * ab + (delta * extent)[:, None] * m, extent


def edge_aimed_rays(data, n, seed):
    """Rays aimed at triangle edges and vertices.  Origins: one half uniform in the scene's box, one quarter the camera's eye,
    one quarter points on other triangles — those end at distance x (1 +- 2^-20), so the interval's end is hit as well."""
    rng = np.random.default_rng(seed)
    target, extent = _targets(data, n, rng)
    lo, hi = data.bounds()
    eye = np.asarray(data.camera.eye, dtype=np.float64)
    o = lo + rng.random((n, 3)) * (hi - lo)
    q1, q2 = n // 2, n // 2 + n // 4
    o[q1:q2] = eye
    o[q2:] = scenes.surface_points(data, n - q2, rng)
    o[np.linalg.norm(target - o, axis=-1) < 1e-3 * extent] = eye
    dist = np.linalg.norm(target - o, axis=-1)
    rays = np.zeros(n, dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"] = o, (target - o) / dist[:, None]
    rays["tmin"], rays["tmax"] = 1e-4 * extent, np.inf
    rays["tmax"][q2:] = dist[q2:] * (1.0 + np.where(rng.random(n - q2) < 0.5, 1.0, -1.0) * 2.0 ** -20)
    perm = rng.permutation(n)  # the three kinds of origin mixed through the batch
    return rays[perm]


def axis_rays(data, n, seed):
    """The same targets approached along a coordinate axis: the origin is the target displaced along one axis, the direction
    is exactly +- that axis (two zero components).  On an axis-aligned box such rays run inside faces and through corners."""
    rng = np.random.default_rng(seed)
    target, extent = _targets(data, n, rng)
    axis, sign = rng.integers(0, 3, n), np.where(rng.random(n) < 0.5, 1.0, -1.0)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign
    rays = np.zeros(n, dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"] = target - d * (extent * rng.uniform(0.05, 1.0, n))[:, None], d
    rays["tmin"], rays["tmax"] = 1e-4 * extent, np.inf
    return rays


def scaled(data, s):
    """`data` with every position (and the camera) multiplied by s."""
    cam = data.camera
    cam = dataclasses.replace(cam, eye=tuple(s * np.asarray(cam.eye, float)), look_at=tuple(s * np.asarray(cam.look_at, float)))
    return dataclasses.replace(data, name=f"{data.name}-x{s:g}", vertices=np.asarray(data.vertices, dtype=np.float64) * s, camera=cam)
