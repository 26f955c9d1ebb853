"""fp64 model of the tree walk of Trav (pooraytracer_amd/csrc/prt_device.h): how much WORK a ray costs in a given tree.

The kernels' box tests are conservative, so nothing that only decides how many nodes a ray visits can change a hit; the
hit tests therefore say nothing about the sorting network of inner_step, the far-to-near push order, the tminf clamp of the
entry distance, tbestf = f32_up(t) after an accept, the size of the slab pad, the early stop of an any-hit traversal or the
place where tris_full is counted.  In K1 (k_trace, k_trace_surface) a lane's traversal touches only its own state (leaf
parking delays a leaf test, it does not change hit.t at the moment that lane tests the leaf), so a ray's counts of inner
node visits, triangle tests and full triangle tests are a function of (tree, ray) alone, and prt_get_counters' node_fetches /
tri_tests / tri_full of a count_work call are their sums over the batch whatever the scheduling, the chunking or K4's order.

walk() restates Trav for a batch of rays, every ray on its own, with no call into the library beyond a tree read from a
PRT_TEST_DUMP_BVH dump (tests/bvh_model.py).  It is vectorised over the rays (one numpy step = one round in which every ray
still under way executes ONE inner_step or ONE leaf_step), which changes nothing per ray.

What is restated
  slab_axis   per axis: id = 1 / (float)d, |id| clamped to 1e28; r = g0 - o; c = r id; pad = (E |id| + |c|) 2^-20;
              idq = gs id; entry plane of a child = its low grid index when id >= 0, its high one otherwise:
              t_entry(q) = q idq + c - pad, t_exit(q) = q idq + c + pad.  E = slab_scale(tree): nextafter((float)(65535 max
              grid_step)) (prt_api.cpp), not the dump header's coord_scale.
  box4        n = max(nx, ny, nz, tminf), f = min(fx, fy, fz, tbestf); tminf = f32_down(tmin), tbestf = f32_up(best).
  inner_step  a child is hit when n <= f; slots 2 and 3 also need ref != 0x80000000 (slots 0 and 1 are not checked); key =
              the bits of (float)n as an unsigned integer, 0xffffffff for a miss; the five compare-exchanges (0,1) (2,3)
              (0,2) (1,3) (1,2) with the kernel's strict `<`; hit children pushed far to near, the nearest becomes current
              (else pop).  A popped child is not tested again.
  test_leaf   the leaf's triangles in leaf order through tree.order against [tmin, best] inclusive: tris counted before the
              test, |n.d| < 1e-8 rejects, tris_full counted after the interval check, an accept sets best = t and tbestf =
              f32_up(t); an any-hit traversal ends after the leaf in which a triangle was accepted (the leaf's remaining
              triangles are still tested: test_leaf's loop has no break).

Robustness.  The model's numbers are not the kernel's: the kernel rounds to fp32 in the box test and to its `real` in the
triangle test.  Every decision is therefore taken with a band around the model's value, and a ray with a decision inside
its band is EXCLUDED from exact comparison (Walk.reason names the first such decision):

  box planes  slab_axis' comment: the roundings of r, 1/d (v_rcp_f32: 1 ulp = 2 units of 2^-24), gs id, r id and the fma sum
              to <= 6 2^-24 (|r| + E) |id| in t(q) = 0.375 pad.  Added here: the subtraction / addition c -+ pad (<= 2^-24
              (|c| + pad): 1 more unit) and the roundings inside pad (3 2^-24 pad): 7.2 units = 0.45 pad.  BAND = 0.5 pad,
              plus 2^-52 (|g0| + |o|) |id| for the fp64 subtraction g0 - o (a scene far from the origin).  BAND < pad, so
              a flat box (entry index == exit index on an axis) is still robustly entered: exit - entry = 2 pad.
  tminf       f32_down rounds twice (conversion, the multiply-subtract): 3 2^-24 |tmin|.
  tbestf      f32_up likewise, of the KERNEL's t of the accepted triangle, which is within the triangle margin dt of the
              model's: 3 2^-24 |best| + dt(best).
  child       robust when n <= f comes out the same at both ends of the bands.
  order       two hit children are robustly ordered when their entry bands are disjoint, or when both entries are
              provably the bit-identical float: both clamped to tminf, or both bound by the same axis at the same grid
              index (the kernel runs the same fmaf on the same operands), in each child with every other term's band
              below the binding one's.  The model's values are then equal as well, and the network is deterministic on equal
              keys.  All pairs of a node's hit children must be robustly ordered.
  triangles   tests/hit_certifier.py's first-order margins (evaluate(): dt, e_a, e_b, e_den for u = 2^-53 or 2^-24), on
              |n.d| against 1e-8, t against tmin and against the running best (margin dt + dt(best): the kernel's best is
              its own t) and the barycentrics.  A t within its margin of an end of the interval only widens the tri_full
              bracket when the barycentrics robustly reject the triangle (the coplanar partner of a quad: its t equals
              the running best to within rounding); if they would accept it the ray is excluded.

`faults`: planted mistakes, each a variant of the walk (test_traversal_model_cpu.py shows that the batches tell them apart).
"""
import dataclasses

import numpy as np

from pooraytracer_amd import scenes
from tests import bvh_model as M
from tests import hit_certifier as H

NOCUR = -0x80000000          # PRT_NOCUR == the ref of an unused slot
MISS = 0xFFFFFFFF
PAD_SCALE = 2.0 ** -20
BAND = 0.5                   # of the pad (module docstring)
U24 = 2.0 ** -24
F32_WIDEN = float(np.float32(2.4e-7))
ID_MAX = float(np.float32(1e28))
STACK = M.STACK_DEPTH + 8
REASONS = ("robust", "box", "order", "denom", "interval", "bary")
FAULTS = ("no_tbestf", "drop_last_ce", "push_reversed", "pad_x16", "no_any_stop", "no_tminf", "full_before_interval")
NETWORK = ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2))


def slab_scale(tree):
    """E of the pad as prt_scene_upload computes it from the grid."""
    e = np.float32(65535.0 * float(tree.step.max()))
    return float(np.nextafter(e, np.float32(np.inf)))


@dataclasses.dataclass
class Walk:
    nodes: np.ndarray      # inner nodes visited, per ray
    tris: np.ndarray       # triangles tested
    full_lo: np.ndarray    # bracket of the tests that went past the interval check
    full_hi: np.ndarray
    prim: np.ndarray       # triangle index of the hit (closest; any-hit: of the accepted one), -1 on a miss
    t: np.ndarray          # its t (tmax on a miss), float64
    reason: np.ndarray     # index into REASONS of the first non-robust decision, 0 for a robust ray

    @property
    def robust(self):
        return self.reason == 0

    @property
    def point(self):
        return self.full_lo == self.full_hi

    def totals(self, mask=None):
        m = self.robust if mask is None else mask
        return {"node_fetches": int(self.nodes[m].sum()), "tri_tests": int(self.tris[m].sum()),
                "tri_full_lo": int(self.full_lo[m].sum()), "tri_full_hi": int(self.full_hi[m].sum())}

    def excluded(self):
        return {REASONS[i]: int((self.reason == i).sum()) for i in range(1, len(REASONS)) if (self.reason == i).any()}


def round_rays(rays, u):
    """The rays as the kernel of unit roundoff u reads them: PrtRay is fp64 at the ABI, the fp32 kernels convert on load."""
    if u < 2.0 ** -40:
        return rays
    out = rays.copy()
    with np.errstate(over="ignore"):
        for k in ("o", "d", "tmin", "tmax"):
            out[k] = rays[k].astype(np.float32)
    return out


def records(vertices, u):
    """The triangle records for walk(), above the precision of the kernel of unit roundoff u (as certify() takes them)."""
    wide = np.longdouble if u < 2.0 ** -40 else np.float64
    return H.tri_records(np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3), wide)


def walk(tree, vertices, rays, any_hit=False, u=H.U64, E=None, faults=(), trace=None, rec=None):
    """The walk of every ray of `rays` (RAY_DTYPE) through `tree`.  E: the kernels' slab_scale (refit_info()["slab_scale"]
    of an uploaded scene; computed from the header otherwise).  `rec`: records(vertices, u), to share between calls.
    `trace`: a list that receives the visit trace (one ray only): ('node', index, [(ref, n, f, hit) per slot], the hit refs
    in visit order) and ('leaf', ref, [(triangle, t, verdict)])."""
    assert all(f in FAULTS for f in faults), faults
    assert trace is None or rays.shape[0] == 1
    wide = np.longdouble if u < 2.0 ** -40 else np.float64
    rays = round_rays(rays, u)
    N = rays.shape[0]
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    tmin = rays["tmin"].astype(np.float64)
    assert (tmin >= 0).all(), "the keys order like floats only for entry distances >= 0"
    E = slab_scale(tree) if E is None else float(E)
    rec = records(vertices, u) if rec is None else rec
    assert rec["D"].dtype == wide
    Q = tree.qboxes()                              # (nodes, slot, axis, lo/hi)
    REF = tree.nodes["ref"].astype(np.int64)
    order = tree.order

    # ---- slab_axis, per ray and axis
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        df = d.astype(np.float32).astype(np.float64)
        idv = 1.0 / df
        idv = np.where(np.abs(idv) <= ID_MAX, idv, np.copysign(ID_MAX, df))
        r = tree.origin[None, :] - o
        c = r * idv
        pad = (E * np.abs(idv) + np.abs(c)) * PAD_SCALE
        band = BAND * pad + 2.0 ** -52 * (np.abs(tree.origin)[None, :] + np.abs(o)) * np.abs(idv)
        if "pad_x16" in faults:
            pad = pad * 16.0
        idq = tree.step[None, :] * idv
        c_lo, c_hi = c - pad, c + pad
    neg = idv < 0
    tminf = tmin - np.abs(tmin) * F32_WIDEN
    tminf_band = 3.0 * U24 * np.abs(tmin)

    def f32_up(x):
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(x), x + np.abs(x) * F32_WIDEN, x)

    best = rays["tmax"].astype(wide)               # hit.t
    best_dt = np.zeros(N, dtype=wide)              # margin of the kernel's hit.t around the model's
    tbestf = f32_up(rays["tmax"].astype(np.float64))
    tbestf_band = np.where(np.isfinite(tbestf), 3.0 * U24 * np.abs(tbestf), 0.0)
    hit_pos = np.full(N, -1, dtype=np.int64)
    cur = np.zeros(N, dtype=np.int64)
    sp = np.zeros(N, dtype=np.int64)
    stack = np.zeros((N, STACK), dtype=np.int64)
    active = np.full(N, tree.n_tris != 0)
    nodes, tris = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    full_lo, full_hi = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    reason = np.zeros(N, dtype=np.int64)

    def flag(idx, code):
        idx = idx[reason[idx] == 0]
        reason[idx] = code

    def pop(idx):
        """cur <- top of the stack, or the end of the traversal."""
        empty = sp[idx] == 0
        done, more = idx[empty], idx[~empty]
        active[done] = False
        cur[done] = NOCUR
        sp[more] -= 1
        cur[more] = stack[more, sp[more]]

    def inner_step(I):
        node = cur[I]
        nodes[I] += 1
        q, ref = Q[node], REF[node].copy()                           # (m, 4, 3, 2), (m, 4)
        ng = neg[I][:, None, :]
        qe = np.where(ng, q[..., 1], q[..., 0]).astype(np.float64)   # entry / exit plane index: the rotation
        qx = np.where(ng, q[..., 0], q[..., 1]).astype(np.float64)
        tn = qe * idq[I][:, None, :] + c_lo[I][:, None, :]
        tf = qx * idq[I][:, None, :] + c_hi[I][:, None, :]
        b3 = np.broadcast_to(band[I][:, None, :], tn.shape)
        m = I.shape[0]
        # the four terms of n: x, y, z, tminf
        T = np.concatenate([tn, np.broadcast_to(tminf[I][:, None, None], (m, 4, 1))], axis=2)
        TB = np.concatenate([b3, np.broadcast_to(tminf_band[I][:, None, None], (m, 4, 1))], axis=2)
        if "no_tminf" in faults:
            T, TB = T[..., :3], TB[..., :3]
        n, n_lo, n_hi = T.max(2), (T - TB).max(2), (T + TB).max(2)
        F = np.concatenate([tf, np.broadcast_to(tbestf[I][:, None, None], (m, 4, 1))], axis=2)
        FB = np.concatenate([b3, np.broadcast_to(tbestf_band[I][:, None, None], (m, 4, 1))], axis=2)
        f, f_lo, f_hi = F.min(2), (F - FB).min(2), (F + FB).min(2)
        hit = n <= f
        used = ref != M.UNUSED
        checked = np.ones((m, 4), dtype=bool)
        checked[:, 2:] = used[:, 2:]                                 # an unused slot 2 / 3 is rejected by its ref
        hit &= checked
        sure = (n_hi <= f_lo) | (n_lo > f_hi)
        flag(I[(checked & ~sure).any(1)], 1)
        # the term that binds n, and whether it does so beyond rounding
        bind = T.argmax(2)
        rows = np.arange(m)[:, None], np.arange(4)[None, :]
        bind_lo = (T - TB)[rows[0], rows[1], bind]
        others = (T + TB).copy()
        others[rows[0], rows[1], bind] = -np.inf
        bind_sure = others.max(2) < bind_lo
        qe4 = np.concatenate([qe, np.zeros((m, 4, 1))], axis=2)
        ident = bind * 65536 + qe4[rows[0], rows[1], bind].astype(np.int64)
        for a in range(4):
            for b in range(a + 1, 4):
                both = hit[:, a] & hit[:, b]
                disjoint = (n_hi[:, a] < n_lo[:, b]) | (n_hi[:, b] < n_lo[:, a])
                same = bind_sure[:, a] & bind_sure[:, b] & (ident[:, a] == ident[:, b])
                flag(I[both & ~disjoint & ~same], 2)
        with np.errstate(over="ignore"):
            key = n.astype(np.float32).view(np.uint32).astype(np.int64)
        key = np.where(hit, key, MISS)
        k = [key[:, s].copy() for s in range(4)]
        rf = [ref[:, s].copy() for s in range(4)]
        for a, b in NETWORK[:4] if "drop_last_ce" in faults else NETWORK:
            sw = k[b] < k[a]
            k[a], k[b] = np.where(sw, k[b], k[a]), np.where(sw, k[a], k[b])
            rf[a], rf[b] = np.where(sw, rf[b], rf[a]), np.where(sw, rf[a], rf[b])
        for s in ((1, 2, 3) if "push_reversed" in faults else (3, 2, 1)):
            J = k[s] != MISS
            stack[I[J], sp[I[J]]] = rf[s][J]
            sp[I[J]] += 1
        assert (sp[I] < STACK).all(), "stack overflow"
        near = k[0] != MISS
        cur[I[near]] = rf[0][near]
        pop(I[~near])
        if trace is not None:
            trace.append(("node", int(node[0]), [(int(ref[0, s]), float(n[0, s]), float(f[0, s]), bool(hit[0, s])) for s in range(4)],
                          [int(rf[s][0]) for s in range(4) if k[s][0] != MISS]))

    def leaf_step(L):
        enc = (~cur[L]) & 0xFFFFFFFF
        first, cnt = enc >> 3, (enc & 7) + 1
        accepted = np.zeros(L.shape[0], dtype=bool)
        log = []
        for i in range(int(cnt.max())):
            sel = i < cnt
            S, pos = L[sel], first[sel] + i
            tri = order[pos]
            tris[S] += 1
            ev = H.evaluate(rec, tri, o[S], d[S], u)
            t, dt = ev["t"], ev["dt"]
            with np.errstate(invalid="ignore"):
                e_den = ev["e_den"] + H.DENOM_MIN * U24
                denom_ok = ev["nd"] >= H.DENOM_MIN
                flag(S[np.abs(ev["nd"] - H.DENOM_MIN) <= e_den], 3)
                lo_m, hi_m = dt, dt + best_dt[S]
                inside = denom_ok & (tmin[S] <= t) & (t <= best[S])
                near_end = denom_ok & ((np.abs(t - tmin[S]) <= lo_m) | (np.abs(t - best[S]) <= hi_m))
                al, be, ea, eb = ev["alpha"], ev["beta"], ev["e_a"], ev["e_b"]
                out = (al < -ea) | (be < -eb) | (al + be > 1 + ea + eb)
                acc_sure = (al > ea) & (be > eb) & (al + be < 1 - ea - eb)
                accept = inside & (al >= 0) & (be >= 0) & (al + be <= 1)
            if "full_before_interval" in faults:
                full_lo[S] += denom_ok
                full_hi[S] += denom_ok
            else:
                # past the interval check for certain / possibly; at an end of the interval only a triangle the
                # barycentrics robustly reject leaves the rest of the walk untouched
                full_lo[S] += inside & ~near_end
                full_hi[S] += inside | near_end
                flag(S[near_end & ~out], 4)
            flag(S[inside & ~near_end & ~out & ~acc_sure], 5)
            A = S[accept]
            best[A], best_dt[A] = t[accept], dt[accept]
            hit_pos[A] = pos[accept]
            if "no_tbestf" not in faults:
                tb = f32_up(t[accept].astype(np.float64))
                tbestf[A], tbestf_band[A] = tb, 3.0 * U24 * np.abs(tb) + dt[accept].astype(np.float64)
            accepted[sel] |= accept
            if trace is not None and sel[0]:
                log.append((int(tri[0]), float(t[0]), "accept" if accept[0] else "inside" if inside[0] else "out"))
        if trace is not None:
            trace.append(("leaf", int(cur[L[0]]), log))
        stop = accepted & (any_hit and "no_any_stop" not in faults)
        active[L[stop]] = False
        cur[L[stop]] = NOCUR
        pop(L[~stop])

    while active.any():
        I = np.flatnonzero(active & (cur >= 0))
        L = np.flatnonzero(active & (cur < 0) & (cur != NOCUR))
        if I.size:
            inner_step(I)
        if L.size:
            leaf_step(L)

    hit = hit_pos >= 0
    return Walk(nodes, tris, full_lo, full_hi, np.where(hit, order[np.maximum(hit_pos, 0)], -1),
                np.where(hit, best, rays["tmax"].astype(wide)).astype(np.float64), reason)


def format_trace(trace):
    lines = []
    for ev in trace:
        if ev[0] == "node":
            slots = " ".join(f"[{ref:#x} n {n:.9g} f {f:.9g} {'hit' if h else 'miss'}]" for ref, n, f, h in ev[2])
            lines.append(f"node {ev[1]}: {slots} -> order {[hex(r & 0xFFFFFFFF) for r in ev[3]]}")
        else:
            lines.append(f"leaf {ev[1] & 0xFFFFFFFF:#x}: " + " ".join(f"(tri {tri} t {t:.17g} {v})" for tri, t, v in ev[2]))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------- the fixed batches
N_RAYS = 4001                       # per batch: several waves and chunks, no multiple of 1024
EXCLUDED_MAX = 0.05                 # of a batch: the cap on the rays the model alone may exclude (a condition)
FAR = (1.0e6, -1.0e6, 1.0e6)
SCENES = {
    "cornell": lambda: scenes.cornell_box(ball_subdiv=3),                         # quads, shared planes, a ball in a box
    "mixed": lambda: scenes.mixed_materials(40, 40),
    "soup": lambda: scenes.triangle_soup(20_000, seed=5, with_light=False),       # a deep tree, real ordering decisions
    "cornell@1e6": lambda: M.translated(scenes.cornell_box(ball_subdiv=3), FAR),  # the pad relative to the grid origin
}
FAMILIES = ("inside", "around", "tmin0", "segments")
# (scene, family) of the batches walked through HOST-built trees; the GPU test adds device-built and refitted trees
HOST_BATCHES = [(s, f) for s in ("cornell", "mixed", "soup") for f in ("inside", "around")] + \
    [("cornell@1e6", "inside"), ("cornell", "tmin0"), ("soup", "tmin0"), ("mixed", "segments"), ("soup", "segments")]


def batch(name, family, n=N_RAYS):
    """The rays of one fixed batch.  inside: origins uniform in the scene's box, directions uniform, [1e-4, inf); around: in a
    box 30 % larger; tmin0: inside with tmin = 0 (the clamp is +0); segments: around, with a finite tmax between 0.3 and
    1.5 scene diagonals (reaching past several occluders: what an any-hit traversal stops in front of).  A translated
    scene gets the rays of the scene at the origin, translated with it."""
    base = name.split("@")[0]
    lo, hi = SCENES[base]().bounds()
    ext = hi - lo
    if family in ("around", "segments"):
        lo, hi = lo - 0.15 * ext, hi + 0.15 * ext
    rays = scenes.random_rays(n, lo, hi, seed=7 + FAMILIES.index(family), tmin=0.0 if family == "tmin0" else 1e-4)
    if family == "segments":
        rays["tmax"] = np.random.default_rng(3).uniform(0.3, 1.5, n) * float(np.linalg.norm(ext))
    if name != base:
        rays["o"] += np.asarray(FAR)
    return rays
