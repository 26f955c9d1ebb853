"""numpy restatement of the signed-distance contract (include/prt.h: prt_scene_topology_info, prt_scene_set_signed_queries,
prt_signed_distance; host pass in mesh_topology.cpp, kernels in pseudonormals.hip and closest_point.hip).

  topology          the weld (bitwise equal coordinates after -0.0 -> +0.0), vertex and edge ids in first-appearance order, the
                    PrtTopologyInfo counts
  pseudonormals     per triangle its unit normal and corner angles, per vertex the angle-weighted and per edge the plain sum
                    of the unit normals of its faces, in fp64, each sum in ascending prim order from 0.0 (np.add.at adds
                    one element after the other in index order); `equal_weight` replaces the angles by 1 - the variant the
                    tests show to be wrong
  per_triangle      those in prt_scene_pseudonormals' layout [n_tris][6][3], with the tests' tolerance per slot
  sign_of_records   contract item 2: the sign from a record (point, prim, feature), the vertices and per-triangle pseudonormals
  winding_number    the generalised winding number (Van Oosterom-Strackee solid angles): the ground truth of inside / outside
  tetrahedron, notched_pyramid   two closed shapes beside the scenes of tests/closest_point_model.py
"""
import numpy as np

from tests import closest_point_model as CM

NONE = 0xFFFFFFFF


def _first_appearance_ids(keys):
    """keys (m,) or (m, k) -> (ids (m,), count): equal keys share an id, ids ascend in order of first appearance."""
    if keys.shape[0] == 0:
        return np.zeros(0, np.int64), 0
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[np.asarray(inv).reshape(-1)], int(first.size)


def topology(vertices):
    """vertices (n, 3, 3) -> dict: vid (n, 3), eid (n, 3; NONE where the edge's ends welded; edges v0v1, v1v2, v2v0),
    n_vertices, n_edges, and `info`, the PrtTopologyInfo counts (without table_bytes)."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    n = v.shape[0]
    bits = np.ascontiguousarray((v.reshape(-1, 3) + 0.0)).view(np.uint64)  # -0.0 + 0.0 is +0.0
    vid, nv = _first_appearance_ids(bits)
    vid = vid.reshape(n, 3)
    u, w = vid, np.roll(vid, -1, axis=1)  # edge k: corner k -> corner k + 1
    valid = u != w
    key = (np.minimum(u, w).astype(np.uint64) << np.uint64(32)) | np.maximum(u, w).astype(np.uint64)
    ids, ne = _first_appearance_ids(key[valid])
    eid = np.full((n, 3), NONE, np.int64)
    eid[valid] = ids
    faces = np.bincount(ids, minlength=ne)
    forward = np.bincount(eid[valid & (u < w)], minlength=ne)
    with np.errstate(over="ignore", invalid="ignore"):
        nrm = CM._cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    degenerate = (~valid).any(axis=1) | (nrm == 0.0).all(axis=1)
    info = {"n_vertices": nv, "n_edges": ne, "boundary_edges": int((faces == 1).sum()), "nonmanifold_edges": int((faces >= 3).sum()),
            "inconsistent_edges": int(((faces == 2) & (forward != 1)).sum()), "degenerate_tris": int(degenerate.sum()),
            "max_valence": int(np.bincount(vid.reshape(-1)).max()) if n else 0}
    info["closed"] = int(info["boundary_edges"] == 0 and info["nonmanifold_edges"] == 0 and info["inconsistent_edges"] == 0)
    return {"vid": vid, "eid": eid, "n_vertices": nv, "n_edges": ne, "info": info}


def pseudonormals(vertices, topo=None, equal_weight=False):
    """dict: vn (n_vertices, 3), en (n_edges, 3) - unnormalised - and per feature the sum of |weights| and the number of
    list entries (vn_w, vn_k, en_w, en_k), which the tolerance of the GPU tests is made of."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    t = topo or topology(v)
    vid, eid = t["vid"], t["eid"]
    n = v.shape[0]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        nrm = CM._cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        nn = CM._dot(nrm, nrm)
        ok = (nn > 0.0) & np.isfinite(nn) & (eid != NONE).all(axis=1)
        nu = np.where(ok[:, None], nrm / np.sqrt(nn)[:, None], 0.0)
        ang = np.zeros((n, 3))
        for k in range(3):
            e1, e2 = v[:, (k + 1) % 3] - v[:, k], v[:, (k + 2) % 3] - v[:, k]
            c = CM._cross(e1, e2)
            ang[:, k] = np.arctan2(np.sqrt(CM._dot(c, c)), CM._dot(e1, e2))
        ang = np.where(ok[:, None], np.ones((n, 3)) if equal_weight else ang, 0.0)
    vn, en = np.zeros((t["n_vertices"], 3)), np.zeros((t["n_edges"], 3))
    flat_v = vid.reshape(-1)  # (prim, corner) order: every vertex's terms are added in ascending prim order
    np.add.at(vn, flat_v, (ang[:, :, None] * nu[:, None, :]).reshape(-1, 3))
    has = (eid != NONE).reshape(-1)
    flat_e = eid.reshape(-1)[has]
    np.add.at(en, flat_e, np.repeat(nu, 3, axis=0)[has])
    return {"vn": vn, "en": en, "topology": t,
            "vn_w": np.bincount(flat_v, weights=np.abs(ang).reshape(-1), minlength=t["n_vertices"]),
            "vn_k": np.bincount(flat_v, minlength=t["n_vertices"]),
            "en_w": np.bincount(flat_e, weights=np.repeat(ok.astype(np.float64), 3)[has], minlength=t["n_edges"]),
            "en_k": np.bincount(flat_e, minlength=t["n_edges"])}


def per_triangle(pn):
    """(P, tol): P (n, 6, 3) in prt_scene_pseudonormals' layout - slots edge v0v1, v1v2, v2v0, vertex v0, v1, v2, zeros for a
    slot without an id - and tol (n, 6), the per-component tolerance (valence + 16) 2^-50 sum|weights| of each slot: a few
    ulps per term for atan2, the normalisation and the product, one rounding per addition, with a fourfold margin."""
    t = pn["topology"]
    vid, eid = t["vid"], t["eid"]
    has = eid != NONE
    e = np.where(has, eid, 0)
    P = np.concatenate([np.where(has[:, :, None], pn["en"][e], 0.0), pn["vn"][vid]], axis=1)
    tol = np.concatenate([np.where(has, (pn["en_k"][e] + 16) * pn["en_w"][e], 0.0), (pn["vn_k"][vid] + 16) * pn["vn_w"][vid]],
                         axis=1) * 2.0 ** -50
    return P, tol


def sign_of_records(p, point, prim, feature, vertices, P):
    """Contract item 2 for records with prim / feature (-1: a miss): s = dot(N, p - point) as x*x + y*y + z*z, N the
    winner's cross(v1 - v0, v2 - v0) at a face and P[prim, feature - 1] elsewhere; +1, -1, or 0 (s == 0, NaN, a miss)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    hit = prim >= 0
    t = np.where(hit, prim, 0)
    with np.errstate(over="ignore", invalid="ignore"):
        face_n = CM._cross(v[t, 1] - v[t, 0], v[t, 2] - v[t, 0])
        N = np.where((feature == 0)[:, None], face_n, P[t, np.clip(feature - 1, 0, 5)])
        s = CM._dot(N, p - point)
    return np.where(hit & (s > 0), 1, np.where(hit & (s < 0), -1, 0)).astype(np.int32)


def model_sign(points, vertices, equal_weight=False):
    """The whole model on the CPU: brute-force closest point, then the sign rule with the model's own pseudonormals.
    Returns (sign, brute-force record)."""
    r = CM.brute_force(points, vertices)
    P, _ = per_triangle(pseudonormals(vertices, equal_weight=equal_weight))
    return sign_of_records(points, r["point"], r["prim"], r["feature"], vertices, P), r


def winding_number(points, vertices, chunk=512):
    """Generalised winding number of each point: the sum of the signed solid angles of all triangles (Van Oosterom and
    Strackee 1983) over 4 pi.  ~1 inside a closed mesh whose faces are counter-clockwise seen from outside, ~0 outside."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros(p.shape[0])
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, None, :]
        a, b, c = (v[None] - q)[:, :, 0], (v[None] - q)[:, :, 1], (v[None] - q)[:, :, 2]
        la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
        num = CM._dot(a, CM._cross(b, c))
        den = la * lb * lc + CM._dot(a, b) * lc + CM._dot(b, c) * la + CM._dot(c, a) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def inside_truth(points, vertices):
    """-1 inside, +1 outside, from the winding number (a closed, outward-oriented mesh)."""
    return np.where(winding_number(points, vertices) > 0.5, -1, 1).astype(np.int32)


# ---- shapes
def _scene(name, tris):
    from tests import bvh_model as M
    return M._scene(name, np.ascontiguousarray(tris, dtype=np.float64))


def tetrahedron_vertices(reverse_face=None):
    x = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    if reverse_face is not None:
        f[reverse_face] = f[reverse_face][::-1]
    return x[f]


def tetrahedron():
    """The regular tetrahedron, faces counter-clockwise seen from outside (4 triangles)."""
    return _scene("tetrahedron", tetrahedron_vertices())


def tetrahedron_inside(points):
    """Analytic truth: -1 inside, +1 outside (below every face plane)."""
    v = tetrahedron_vertices()
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    h = ((points[:, None, :] - v[None, :, 0]) * n[None]).sum(-1)
    return np.where((h < 0).all(axis=1), -1, 1).astype(np.int32)


def notched_pyramid_vertices(m=64, h=2.0, notch=0.5):
    n = notch
    poly = [(0.0, 0.0), (2.0, 0.0), (2.0, n), (n, n), (n, 2.0), (0.0, 2.0)]
    ring = []
    for i, a in enumerate(poly):
        b = poly[(i + 1) % len(poly)]
        pieces = m if i in (2, 3) else 1  # the third and fourth edges: the two sides of the notch
        for j in range(pieces):
            s = j / pieces
            ring.append((a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1]), 0.0))
    ring = np.array(ring)
    apex, bottom = np.array([n / 2, n / 2, h]), np.array([n / 2, n / 2, 0.0])
    tris = []
    for i in range(ring.shape[0]):
        a, b = ring[i], ring[(i + 1) % ring.shape[0]]
        tris.append((apex, a, b))
        tris.append((bottom, b, a))
    return np.array(tris)


def notched_pyramid(m=64, h=2.0, notch=0.5):
    """A pyramid over an L-shaped base: across the notch the two fans of m thin faces meet the apex at an acute dihedral
    angle, with very unequal corner angles - where the plane-side sign and an equal-weight normal sum go wrong."""
    return _scene("notched_pyramid", notched_pyramid_vertices(m, h, notch))


def apex_queries(n=4096, seed=7, h=2.0, notch=0.5, radius=0.2):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.array([notch / 2, notch / 2, h]) + d * (radius * rng.random((n, 1)) ** (1.0 / 3.0))


def box_queries(vertices, n=4096, seed=11):
    """Uniform in the bounds padded by 10 % of the extent (closest_point_model.queries' `box` class)."""
    return CM.queries(vertices, n, seed)["box"][0]
