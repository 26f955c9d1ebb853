"""fp64 model of the traversal tree (4-wide, 16-bit quantised DNode boxes) that either BVH builder produces.

It reads the file the dev-hooks library writes under PRT_TEST_DUMP_BVH=<file> (prt_api.cpp, dump_bvh) and checks it against
the scene's fp64 vertices without calling into the library:

  * the leaf order is a permutation, every leaf ref decodes to 1..PRT_LEAF_MAX triangles in range, every triangle sits in
    exactly one leaf and every node is reached exactly once from the root;
  * used slots come first; an unused slot has ref 0x80000000 and the inverted range 0x0000ffff on all three axes;
  * every triangle's box (the scene setup's: edges thinner than 1e-4 padded, AABB.cpp), widened by the margin prim_boxes
    adds (1e-9 extent + 256 eps scale), lies inside its leaf's box dequantised in fp64 as the kernels read it
    (grid_origin + q * grid_step); every child box lies inside its parent's, give or take one grid step;
  * the stack need (tree_stack_need's rule) is <= PRT_STACK_DEPTH and equals what the library recorded.

Also: a canonical form (depth-first in child order: per node its dequantised child boxes, per leaf its set of triangles),
equal for two builds of one scene whatever the node numbering, and the SAH cost of the wide tree (node 1.0, triangle 1.5,
the builders' constants).  Adversarial scene generators for the builders live here too, not in scenes.py (bench.py imports
that one).
"""
import struct

import numpy as np

from pooraytracer_amd import _abi, scenes

MAGIC, VERSION = 0x48564250, 1
LEAF_MAX = 4
STACK_DEPTH = 40
UNUSED = -0x80000000
INVERTED = 0x0000FFFF
COST_NODE, COST_TRI = 1.0, 1.5
EPS = np.finfo(np.float64).eps
HEADER = struct.Struct("<IIQQIIiI3f3ffI")
NODE = np.dtype([("bx", "<u4", 4), ("by", "<u4", 4), ("bz", "<u4", 4), ("ref", "<i4", 4)])
assert HEADER.size == 72 and NODE.itemsize == 64


class BVHCheckError(AssertionError):
    """A tree invariant does not hold; the message names it."""


class Tree:
    """One dumped tree: header fields, `nodes` (structured DNode array), `order` (leaf position -> triangle index)."""

    def __init__(self, n_tris, built_on_device, depth, stack_need, origin, step, coord_scale, nodes, order):
        self.n_tris, self.built_on_device, self.depth, self.stack_need = n_tris, built_on_device, depth, stack_need
        self.origin = np.asarray(origin, dtype=np.float32).astype(np.float64)
        self.step = np.asarray(step, dtype=np.float32).astype(np.float64)
        self.coord_scale = coord_scale
        self.nodes = nodes
        self.order = order

    @property
    def n_nodes(self):
        return int(self.nodes.shape[0])

    def copy(self):
        return Tree(self.n_tris, self.built_on_device, self.depth, self.stack_need, self.origin, self.step, self.coord_scale,
                    self.nodes.copy(), self.order.copy())

    def qboxes(self):
        """(n_nodes, 4, 3, 2) grid indices: [node, slot, axis, lo/hi]."""
        w = np.stack([self.nodes["bx"], self.nodes["by"], self.nodes["bz"]], axis=-1)  # (n, 4, 3)
        return np.stack([w & 0xFFFF, w >> 16], axis=-1).astype(np.int64)

    def boxes(self):
        """(n_nodes, 4, 3, 2) world boxes, dequantised in fp64 as prt_device.h does: origin + q * step."""
        q = self.qboxes().astype(np.float64)
        return self.origin[None, None, :, None] + q * self.step[None, None, :, None]


def read_dump(path):
    with open(path, "rb") as f:
        raw = f.read()
    (magic, version, n_tris, n_nodes, on_dev, depth, need, node_bytes, ox, oy, oz, sx, sy, sz, cs, _z) = HEADER.unpack_from(raw, 0)
    if magic != MAGIC or version != VERSION or node_bytes != NODE.itemsize:
        raise ValueError(f"{path}: not a version-{VERSION} BVH dump")
    off = HEADER.size
    nodes = np.frombuffer(raw, dtype=NODE, count=n_nodes, offset=off).copy()
    off += n_nodes * NODE.itemsize
    order = np.frombuffer(raw, dtype="<u4", count=n_tris, offset=off).astype(np.int64)
    if off + 4 * n_tris != len(raw):
        raise ValueError(f"{path}: {len(raw)} bytes, expected {off + 4 * n_tris}")
    return Tree(n_tris, on_dev, depth, need, (ox, oy, oz), (sx, sy, sz), cs, nodes, order)


def decode_leaf(ref):
    enc = (~np.asarray(ref, dtype=np.int64)) & 0xFFFFFFFF
    return enc >> 3, (enc & 7) + 1


def tri_boxes(vertices):
    """fp64 triangle boxes as the scene setup makes them (scene_setup.cpp edge_interval: per edge v0-v1 and v0-v2, an
    axis extent below 1e-4 is padded by 5e-5 on each side), and the margin prim_boxes widens them by."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)

    def edge(a, b):
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        thin = hi - lo < 0.0001
        return np.where(thin, lo - 0.0001 / 2.0, lo), np.where(thin, hi + 0.0001 / 2.0, hi)

    l0, h0 = edge(v[:, 0], v[:, 1])
    l1, h1 = edge(v[:, 0], v[:, 2])
    lo, hi = np.minimum(l0, l1), np.maximum(h0, h1)
    scale = max(1.0, float(np.abs(lo).max()), float(np.abs(hi).max())) if len(v) else 1.0
    extent = max(1.0, float((hi.max(0) - lo.min(0)).max())) if len(v) else 1.0
    delta = 1e-9 * extent + 256.0 * EPS * scale
    return lo, hi, delta, scale


def _levels(tree):
    """Breadth-first levels of node indices from the root, checking that inner refs are in range and every node is
    reached exactly once.  Returns the list of levels."""
    refs = tree.nodes["ref"].astype(np.int64)
    seen = np.zeros(tree.n_nodes, dtype=np.int64)
    seen[0] = 1
    levels, cur = [], np.array([0], dtype=np.int64)
    while cur.size:
        levels.append(cur)
        if len(levels) > tree.n_nodes + 1:
            raise BVHCheckError("node reached twice (the tree has a cycle)")
        r = refs[cur].reshape(-1)
        kids = r[r >= 0]
        if (kids >= tree.n_nodes).any():
            raise BVHCheckError(f"node index out of range: {int(kids.max())} >= {tree.n_nodes} nodes")
        np.add.at(seen, kids, 1)
        if (seen[kids] > 1).any():
            raise BVHCheckError(f"node reached twice from the root: node {int(kids[seen[kids] > 1][0])}")
        cur = kids
    if (seen == 0).any():
        raise BVHCheckError(f"node not reached from the root: {int((seen == 0).sum())} of {tree.n_nodes} nodes")
    return levels


def stack_need(tree, levels=None):
    """tree_stack_need (bvh_build.cpp): need(node) = (used children - 1) + max over inner children of need(child)."""
    levels = _levels(tree) if levels is None else levels
    refs = tree.nodes["ref"].astype(np.int64)
    need = np.zeros(tree.n_nodes, dtype=np.int64)
    for lv in reversed(levels):
        r = refs[lv]
        used = (r != UNUSED).sum(axis=1)
        kid = np.where(r >= 0, need[np.clip(r, 0, None)], 0)
        need[lv] = np.maximum(used - 1, 0) + kid.max(axis=1)
    return int(need[0])


def check_tree(tree, vertices, info=None):
    """Every invariant of the module docstring; raises BVHCheckError naming the first one broken.  `info` (optional):
    Scene.bvh_info() of the scene, whose n_nodes and depth must agree.  Returns a small report."""
    n = tree.n_tris
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 3)
    if v.shape[0] != n:
        raise BVHCheckError(f"dump holds {n} triangles, the scene {v.shape[0]}")
    if tree.n_nodes < 1:
        raise BVHCheckError("no nodes")
    if not np.array_equal(np.sort(tree.order), np.arange(n)):
        raise BVHCheckError("leaf order is not a permutation of 0..n_tris-1")
    refs = tree.nodes["ref"].astype(np.int64)
    used = refs != UNUSED
    # slots fill from the front (the traversal reads the refs of slots 2 and 3 only)
    if (used[:, 1:] & ~used[:, :-1]).any():
        bad = int(np.argwhere(used[:, 1:] & ~used[:, :-1])[0, 0])
        raise BVHCheckError(f"unused slot before a used one in node {bad}")
    q = tree.qboxes()
    inv = np.stack([tree.nodes["bx"], tree.nodes["by"], tree.nodes["bz"]], axis=-1) == INVERTED  # (n, 4, 3)
    if (~used[..., None] & ~inv).any():
        bad = int(np.argwhere(~used[..., None] & ~inv)[0, 0])
        raise BVHCheckError(f"unused slot without the inverted box 0x0000ffff in node {bad}")
    nused = used.sum(axis=1)
    if n >= 2 and (nused < 2).any():
        raise BVHCheckError(f"node with fewer than two children: node {int(np.argmin(nused))}")
    levels = _levels(tree)

    # leaves: 1..LEAF_MAX triangles in range, every leaf position (= every triangle) in exactly one leaf
    leaf = used & (refs < 0)
    li, ls = np.nonzero(leaf)
    first, cnt = decode_leaf(refs[li, ls])
    if n == 1 and li.size == 2 and refs[0, 0] == refs[0, 1]:  # the one-triangle root lists its leaf twice
        li, ls, first, cnt = li[:1], ls[:1], first[:1], cnt[:1]
    if (cnt < 1).any() or (cnt > LEAF_MAX).any() or (first + cnt > n).any():
        raise BVHCheckError("leaf ref decodes to a triangle range out of bounds")
    pos = np.repeat(first, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    cover = np.bincount(pos, minlength=n)
    if (cover > 1).any():
        raise BVHCheckError(f"triangle in two leaves: triangle {int(tree.order[np.argmax(cover > 1)])}")
    if (cover == 0).any():
        raise BVHCheckError(f"triangle in no leaf: {int((cover == 0).sum())} triangles, e.g. {int(tree.order[np.argmax(cover == 0)])}")

    # geometry, in fp64: leaf boxes hold their triangles (widened by prim_boxes' margin), children sit in their parent
    box = tree.boxes()
    lo, hi, delta, scale = tri_boxes(v)
    tol = 8.0 * EPS * max(scale, float(np.abs(box[used]).max()))  # roundings of the dequantisation itself
    leaf_of_pos = np.repeat(np.arange(li.size), cnt)
    tri = tree.order[pos]
    blo, bhi = box[li, ls, :, 0][leaf_of_pos], box[li, ls, :, 1][leaf_of_pos]
    out = ((lo[tri] - delta) < blo - tol) | ((hi[tri] + delta) > bhi + tol)
    if out.any():
        k = int(np.argwhere(out.any(axis=1))[0, 0])
        a = int(np.argmax(out[k]))
        raise BVHCheckError(f"triangle outside its leaf box: triangle {int(tri[k])} axis {a}: "
                            f"[{lo[tri[k], a] - delta!r}, {hi[tri[k], a] + delta!r}] vs leaf [{blo[k, a]!r}, {bhi[k, a]!r}]")
    inner = used & (refs >= 0)
    pi, ps = np.nonzero(inner)
    child = refs[pi, ps]
    slack = 1.0001 * tree.step
    cused = used[child]
    clo = np.where(cused[..., None], box[child, :, :, 0], np.inf)
    chi = np.where(cused[..., None], box[child, :, :, 1], -np.inf)
    if ((clo < box[pi, ps, None, :, 0] - slack).any() or (chi > box[pi, ps, None, :, 1] + slack).any()):
        raise BVHCheckError("child box outside its parent's by more than one grid step")

    need = stack_need(tree, levels)
    if need > STACK_DEPTH:
        raise BVHCheckError(f"stack need {need} exceeds PRT_STACK_DEPTH {STACK_DEPTH}")
    if need != tree.stack_need:
        raise BVHCheckError(f"stack need {need} differs from the {tree.stack_need} the library recorded")
    if tree.depth != len(levels):
        raise BVHCheckError(f"depth {tree.depth} recorded, the tree has {len(levels)} levels of nodes")
    if info is not None:
        if int(info["n_nodes"]) != tree.n_nodes or int(info["depth"]) != tree.depth:
            raise BVHCheckError(f"bvh_info (n_nodes {info['n_nodes']}, depth {info['depth']}) disagrees with the dump "
                                f"({tree.n_nodes}, {tree.depth})")
        if int(info["built_on_device"]) != tree.built_on_device:
            raise BVHCheckError("bvh_info and the dump disagree on the builder")
    return {"stack_need": need, "levels": len(levels), "leaves": int(li.size), "nodes": tree.n_nodes}


def canonical(tree):
    """Depth-first walk in child order: per inner node ('n', its children's dequantised boxes), per leaf ('l', its box, the
    sorted triangle indices).  Independent of node numbering."""
    box = tree.boxes()
    refs = tree.nodes["ref"]
    out, st = [], [0]
    while st:
        i = st.pop()
        r = refs[i]
        k = int((r != UNUSED).sum())
        out.append(("n", box[i, :k].tobytes()))
        for s in range(k):
            if r[s] < 0:
                f, c = decode_leaf(r[s])
                out.append(("l", box[i, s].tobytes(), tuple(sorted(tree.order[int(f):int(f + c)].tolist()))))
        st.extend(int(r[s]) for s in range(k - 1, -1, -1) if r[s] >= 0)
    return out


def sah_cost(tree):
    """SAH cost of the wide tree from its dequantised boxes: 1.0 per node visit, 1.5 per triangle test, each weighted by the
    half area of the box that gates it over the half area of the root's box (the union of the root's children)."""
    box = tree.boxes()
    refs = tree.nodes["ref"].astype(np.int64)
    used = refs != UNUSED
    ext = np.maximum(box[..., 1] - box[..., 0], 0.0)
    area = ext[..., 0] * ext[..., 1] + ext[..., 1] * ext[..., 2] + ext[..., 2] * ext[..., 0]
    r0 = box[0][used[0]]
    e = r0[:, :, 1].max(0) - r0[:, :, 0].min(0)
    root = max(e[0] * e[1] + e[1] * e[2] + e[2] * e[0], 1e-300)
    _, cnt = decode_leaf(np.where(refs < 0, refs, -1))
    cost = np.where(used & (refs >= 0), COST_NODE * area, 0.0) + np.where(used & (refs < 0), COST_TRI * cnt * area, 0.0)
    return COST_NODE + float(cost.sum()) / root


# ------------------------------------------------------------------------------------------------- adversarial scenes
_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.5], [0.25, 1.0, 0.75]])  # binary fractions: fp32-exact vertices


def _scene(name, verts):
    b = scenes._Builder(name)
    m = b.material(scenes.Material("White", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    b.mesh(name, m, np.asarray(verts, dtype=np.float64).reshape(-1, 3, 3))
    lo, hi = b.v[0].reshape(-1, 3).min(0), b.v[0].reshape(-1, 3).max(0)
    c = 0.5 * (lo + hi)
    cam = scenes.Camera(32, 32, 40.0, eye=tuple(c + np.array([0.0, 0.0, 3.0]) * max(1.0, float((hi - lo).max()))), look_at=tuple(c))
    return b.build(cam)


def identical(n=3000):
    """n copies of one triangle: every Morton key equal, every candidate split ties."""
    return _scene(f"identical{n}", np.broadcast_to(_TRI, (n, 3, 3)))


def clusters(k=6, per=400):
    """k clusters of identical triangles."""
    off = np.array([[3.0 * i, 1.5 * (i % 2), -2.0 * (i % 3)] for i in range(k)])
    return _scene("clusters", (_TRI[None] * 0.5 + off[:, None, None, :]).repeat(per, axis=0))


def _soup(n, seed, extent=0.01):
    rng = np.random.default_rng(seed)
    return rng.random((n, 1, 3)) + (rng.random((n, 3, 3)) - 0.5) * extent


def soup(n, seed=11):
    return _scene(f"soup{n}", _soup(n, seed))


def flat(n=4000):
    """A flat scene: every vertex at z = 0 (zero extent on one axis)."""
    v = _soup(n, 3, extent=0.05)
    v[..., 2] = 0.0
    return _scene("flat", v)


def walls(per=1500):
    """Axis-aligned zero-thickness walls: x = 0, y = 0, z = 0 and x = 1."""
    rng = np.random.default_rng(5)
    out = []
    for axis, at in ((0, 0.0), (1, 0.0), (2, 0.0), (0, 1.0)):
        v = _soup(per, int(rng.integers(1 << 30)), extent=0.04)
        v[..., axis] = at
        out.append(v)
    return _scene("walls", np.concatenate(out))


def geometric(n=2000):
    """Positions in a geometric progression over 12 decades: the 17-bit Morton cells collapse near the origin."""
    c = 10.0 ** (-12.0 * np.arange(n) / n)
    return _scene("geometric", c[:, None, None] * (0.1 * _TRI[None] + np.array([1.0, 0.7, 0.4])[None, None, :]))


def mixed_sizes(n=3000, walls=16):
    """Wall-sized triangles among tiny ones."""
    rng = np.random.default_rng(8)
    big = rng.random((walls, 3, 3)) * 1.2 - 0.1
    return _scene("mixed_sizes", np.concatenate([_soup(n, 9, extent=0.002), big]))


def large_soup(n=1_200_000, outliers=64):
    """More triangles than k_centroid_bounds covers in one pass (2048 blocks x 256 = 524,288), with far outliers at the end
    of the description order: only a second grid-stride pass sees them."""
    v = _soup(n, 21)
    rng = np.random.default_rng(22)
    far = rng.uniform(-1.0, 1.0, (outliers, 1, 3))
    far = 40.0 * far / np.abs(far).max(axis=-1, keepdims=True)
    v[-outliers:] = far + (rng.random((outliers, 3, 3)) - 0.5) * 0.05
    return _scene("large_soup", v)


def translated(data, by=(1.0e6, -1.0e6, 1.0e6)):
    import copy
    out = copy.copy(data)
    out.name = data.name + "@1e6"
    out.vertices = data.vertices + np.asarray(by, dtype=np.float64)
    return out


SIZES = (2, 3, 4, 5, 16, 17, 18, 1024, 1025, 4096, 4097)
GENERATORS = {
    "identical": identical,
    "clusters": clusters,
    "flat": flat,
    "walls": walls,
    "geometric": geometric,
    "mixed_sizes": mixed_sizes,
    **{f"soup{n}": (lambda n=n: soup(n)) for n in SIZES},
}
