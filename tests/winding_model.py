"""numpy restatement of the winding-number contract (include/prt.h: prt_scene_set_winding_queries, prt_winding_number;
kernels in winding_number.hip).

  moments        the table of a tree (a bvh_model.Tree dump) and the scene's vertices: one record N[3], c[3], r, A per child
                 slot, [n_nodes, 4, 8], with the header's formulas, every sum from 0.0 in leaf / slot order
  walk           the contract's walk for a batch of points, on a given table (the model's or the device's own): the values,
                 the four work counts per query and the list of terms (query, value, kind)
  moment_scale   per slot the size its record's roundings scale with (the GPU test's tolerance)
  brute force    is signed_distance_model.winding_number
  open_sphere, open_box   two open shapes beside the closed ones of signed_distance_model / closest_point_model

The walk visits the tree level by level for the whole batch and adds each query's terms in extended precision, so the
order in which one query's terms are added differs from the kernel's (the contract leaves it open): values agree to the
kernel's rounding, counts and terms exactly.
"""
import numpy as np

from tests import bvh_model as M
from tests import closest_point_model as CM

FOUR_PI = 4.0 * np.pi
FAR_INNER, FAR_LEAF, EXACT = 0, 1, 2


def _leaf_slots(tree):
    refs = tree.nodes["ref"].astype(np.int64)
    used = refs != M.UNUSED
    li, ls = np.nonzero(used & (refs < 0))
    first, cnt = M.decode_leaf(refs[li, ls])
    return refs, used, li, ls, first, cnt


def moments(tree, vertices):
    """(n_nodes, 4, 8) float64: N, c, r, A of every child slot; zeros for an unused slot."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)[tree.order]  # leaf order, as the corner table
    refs, used, li, ls, first, cnt = _leaf_slots(tree)
    out = np.zeros((tree.n_nodes, 4, 8))
    m = li.size
    A, N, G = np.zeros(m), np.zeros((m, 3)), np.zeros((m, 3))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(int(cnt.max()) if m else 0):
            on = k < cnt
            t = v[np.where(on, first + k, first)]
            av = 0.5 * CM._cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
            a = np.sqrt(CM._dot(av, av))
            g = ((t[:, 0] + t[:, 1]) + t[:, 2]) / 3.0
            ok = on & (a > 0.0) & np.isfinite(a)
            A = np.where(ok, A + a, A)
            N = np.where(ok[:, None], N + av, N)
            G = np.where(ok[:, None], G + a[:, None] * g, G)
        c = np.where((A > 0.0)[:, None], G / A[:, None], v[first, 0])
        r = np.zeros(m)
        for k in range(int(cnt.max()) if m else 0):
            on = k < cnt
            t = v[np.where(on, first + k, first)]
            for j in range(3):
                d = t[:, j] - c
                d = np.sqrt(CM._dot(d, d))
                r = np.where(on & (d > r), d, r)
    out[li, ls, 0:3], out[li, ls, 3:6], out[li, ls, 6], out[li, ls, 7] = N, c, r, A
    # inner slots, deepest level first: the child's used slots in slot order
    for lv in reversed(M._levels(tree)):
        pi, ps = np.nonzero(refs[lv] >= 0)
        pi = lv[pi]
        ch = refs[pi, ps]
        m = ch.size
        if not m:
            continue
        A, N, G, c0 = np.zeros(m), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3))
        seen = np.zeros(m, dtype=bool)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for k in range(4):
                u = used[ch, k]
                rec = out[ch, k]
                c0 = np.where((u & ~seen)[:, None], rec[:, 3:6], c0)
                seen |= u
                A = np.where(u, A + rec[:, 7], A)
                N = np.where(u[:, None], N + rec[:, 0:3], N)
                G = np.where(u[:, None], G + rec[:, 3:6] * rec[:, 7:8], G)
            c = np.where((A > 0.0)[:, None], G / A[:, None], c0)
            r = np.zeros(m)
            for k in range(4):
                u = used[ch, k]
                rec = out[ch, k]
                d = rec[:, 3:6] - c
                d = np.sqrt(CM._dot(d, d)) + rec[:, 6]
                r = np.where(u & (d > r), d, r)
        out[pi, ps, 0:3], out[pi, ps, 3:6], out[pi, ps, 6], out[pi, ps, 7] = N, c, r, A
    return out


def moment_scale(tree, table):
    """(n_nodes, 4): max(|c|) + r + sqrt(A) of each slot - the lengths a record's roundings scale with (areas: its square)."""
    return np.abs(table[:, :, 3:6]).max(axis=-1) + table[:, :, 6] + np.sqrt(np.abs(table[:, :, 7]))


def solid_angle(p, t):
    """Van Oosterom and Strackee: p (m, 3), t (m, 3, 3) -> (m,)."""
    a, b, c = t[:, 0] - p, t[:, 1] - p, t[:, 2] - p
    la, lb, lc = np.sqrt(CM._dot(a, a)), np.sqrt(CM._dot(b, b)), np.sqrt(CM._dot(c, c))
    num = CM._dot(a, CM._cross(b, c))
    den = la * lb * lc + CM._dot(a, b) * lc + CM._dot(b, c) * la + CM._dot(c, a) * lb
    return 2.0 * np.arctan2(num, den)


class Walk:
    """value (n,), and per query nodes, tris, far_inner, far_leaf; terms: (query (k,), value (k,), kind (k,))."""


def walk(tree, vertices, points, beta, table=None):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)[tree.order]
    table = moments(tree, vertices) if table is None else table
    refs = tree.nodes["ref"].astype(np.int64)
    n = p.shape[0]
    w = Walk()
    tq, tv, tk, vq = [], [], [], []

    def add(q, val, kind):
        tq.append(q), tv.append(val), tk.append(np.full(q.size, kind, dtype=np.int8))

    q, node = np.arange(n), np.zeros(n, dtype=np.int64)
    if tree.n_tris == 0:
        q = q[:0]
    while q.size:
        vq.append(q)
        nq, nn = [], []
        for s in range(4):
            r = refs[node, s]
            on = r != M.UNUSED
            if s > 0:
                on &= ~((r < 0) & (r == refs[node, s - 1]))  # the one-triangle root lists its leaf twice
            rec = table[node, s]
            d = rec[:, 3:6] - p[q]
            dd = CM._dot(d, d)
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                br = beta * rec[:, 6]
                far = on & (dd > br * br)
                term = CM._dot(rec[:, 0:3], d) / (dd * np.sqrt(dd))
            add(q[far & (r >= 0)], term[far & (r >= 0)], FAR_INNER)
            add(q[far & (r < 0)], term[far & (r < 0)], FAR_LEAF)
            near = on & ~far
            leaf = near & (r < 0)
            if leaf.any():
                first, cnt = M.decode_leaf(r[leaf])
                lq = np.repeat(q[leaf], cnt)
                pos = np.repeat(first, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                add(lq, solid_angle(p[lq], v[pos]), EXACT)
            inner = near & (r >= 0)
            nq.append(q[inner]), nn.append(r[inner])
        q, node = np.concatenate(nq), np.concatenate(nn)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    tq, tv, tk = cat(tq, np.int64), cat(tv, np.float64), cat(tk, np.int8)
    w.terms = (tq, tv, tk)
    w.nodes = np.bincount(cat(vq, np.int64), minlength=n)
    w.far_inner, w.far_leaf, w.tris = (np.bincount(tq[tk == k], minlength=n) for k in (FAR_INNER, FAR_LEAF, EXACT))
    # each query's terms, summed in extended precision (the contract leaves the order open; this sum is closer to the
    # exact one than any fp64 order): sorted by query, one sequential pass per segment
    S = np.zeros(n, dtype=np.longdouble)
    if tq.size:
        o = np.argsort(tq, kind="stable")
        sq = tq[o]
        start = np.flatnonzero(np.r_[True, sq[1:] != sq[:-1]])
        S[sq[start]] = np.add.reduceat(tv[o].astype(np.longdouble), start)
    w.value = (S / np.longdouble(FOUR_PI)).astype(np.float64)
    return w


# ---- shapes and queries
def open_sphere(n_lat=32, n_lon=48, cap=0.35):
    """A unit sphere tessellated by latitude and longitude, faces counter-clockwise seen from outside, with the polar cap
    above colatitude `cap` (radians) removed: 2 * n_lon * (n_lat - 1) - n_lon triangles around a round hole."""
    th = cap + (np.pi - cap) * np.arange(n_lat + 1) / n_lat  # colatitude from the rim of the hole to the south pole
    ph = 2.0 * np.pi * np.arange(n_lon + 1) / n_lon

    def pt(i, j):
        return np.array([np.sin(th[i]) * np.cos(ph[j % n_lon]), np.sin(th[i]) * np.sin(ph[j % n_lon]), np.cos(th[i])])

    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
            tris.append((a, b, c))
            tris.append((a, c, d))
    t = np.array(tris)
    area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    return M._scene("open_sphere", t[area > 1e-12])  # (the fan at the south pole: half its quads are degenerate)


def open_box():
    """The unit cube without its top (z = 1) face, each side 8 x 8 quads: 640 triangles, outward orientation."""
    k = 8
    g = np.arange(k + 1) / k
    tris = []

    def side(origin, du, dv):  # outward normal = du x dv
        o, du, dv = np.array(origin, float), np.array(du, float), np.array(dv, float)
        for i in range(k):
            for j in range(k):
                a, b = o + g[i] * du + g[j] * dv, o + g[i + 1] * du + g[j] * dv
                c, d = o + g[i + 1] * du + g[j + 1] * dv, o + g[i] * du + g[j + 1] * dv
                tris.extend([(a, b, c), (a, c, d)])

    side((0, 0, 0), (0, 1, 0), (1, 0, 0))  # bottom, normal -z
    side((0, 0, 0), (1, 0, 0), (0, 0, 1))  # y = 0, normal -y
    side((0, 1, 0), (0, 0, 1), (1, 0, 0))  # y = 1, normal +y
    side((0, 0, 0), (0, 0, 1), (0, 1, 0))  # x = 0, normal -x
    side((1, 0, 0), (0, 1, 0), (0, 0, 1))  # x = 1, normal +x
    return M._scene("open_box", np.array(tris))


def box_queries(vertices, n=4096, seed=5, factor=1.5):
    """n uniform points in the bounds scaled by `factor` about their centre."""
    p = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * factor
    return np.ascontiguousarray(c + (np.random.default_rng(seed).random((n, 3)) * 2.0 - 1.0) * h)
