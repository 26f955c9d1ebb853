"""CPU tests of the fp64 tree model (tests/bvh_model.py) on host-built trees: every adversarial scene's tree passes the
checker, and each broken invariant is reported by name.  The trees come from the dev-hooks library's PRT_TEST_DUMP_BVH
dump at prt_scene_create (no GPU needed)."""
import numpy as np
import pytest

from pooraytracer_amd import api, scenes
from tests import bvh_model as M


def host_tree(data, tmp_path, monkeypatch):
    path = str(tmp_path / "tree.bin")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    with api.dev_hooks():
        sc = api.Scene(data)
    return M.read_dump(path), sc.bvh_info()


@pytest.mark.parametrize("name", sorted(M.GENERATORS) + ["cornell"])
@pytest.mark.parametrize("moved", [False, True], ids=["origin", "at1e6"])
def test_host_tree_passes_the_checker(prt_lib, tmp_path, monkeypatch, name, moved):
    data = scenes.cornell_box(ball_subdiv=4, width=48, height=48) if name == "cornell" else M.GENERATORS[name]()
    if moved:
        data = M.translated(data)
    tree, info = host_tree(data, tmp_path, monkeypatch)
    assert tree.built_on_device == 0 and tree.n_tris == data.n_tris
    rep = M.check_tree(tree, data.vertices, info)
    assert rep["stack_need"] <= M.STACK_DEPTH
    # the canonical form is a function of the tree alone
    assert M.canonical(tree) == M.canonical(M.read_dump(str(tmp_path / "tree.bin")))
    assert M.sah_cost(tree) >= M.COST_NODE


def test_host_tree_of_the_large_soup_passes_the_checker(prt_lib, tmp_path, monkeypatch):
    data = M.large_soup()
    tree, info = host_tree(data, tmp_path, monkeypatch)
    M.check_tree(tree, data.vertices, info)


def test_host_rebuild_in_update_vertices_is_dumped(prt_lib, tmp_path, monkeypatch):
    data = M.flat()
    tree0, _ = host_tree(data, tmp_path, monkeypatch)
    v = data.vertices * np.array([1.0, 2.0, 1.0]) + np.array([0.0, 0.0, 0.5])
    with api.dev_hooks():
        sc = api.Scene(data)
        sc.update_vertices(v)
    tree1 = M.read_dump(str(tmp_path / "tree.bin"))
    M.check_tree(tree1, v, sc.bvh_info())
    with pytest.raises(M.BVHCheckError, match="outside its leaf box"):
        M.check_tree(tree0, v)  # the tree of the old positions does not hold the new ones


# ---------------------------------------------------------------------------------------------------------- mutants
def _leaf_slots(t):
    refs = t.nodes["ref"]
    return [(int(i), int(s)) for i, s in zip(*np.nonzero((refs != M.UNUSED) & (refs < 0)))]


def _nused(t):
    return (t.nodes["ref"] != M.UNUSED).sum(axis=1)


def shrink_leaf_box(t, v):
    i, s = _leaf_slots(t)[0]
    lo, hi = t.nodes["bx"][i, s] & 0xFFFF, t.nodes["bx"][i, s] >> 16
    assert hi > lo
    t.nodes["bx"][i, s] = lo | ((hi - 1) << 16)


def duplicate_triangle(t, v):
    for i, s in _leaf_slots(t):
        f, c = M.decode_leaf(t.nodes["ref"][i, s])
        if c < M.LEAF_MAX and f + c < t.n_tris:
            t.nodes["ref"][i, s] = ~np.int32((int(f) << 3) | int(c))  # one more triangle: the next leaf's first
            return
    raise AssertionError("no leaf to extend")


def drop_leaf(t, v):
    for i, s in _leaf_slots(t):
        k = int(_nused(t)[i])
        if k >= 3:
            for f in ("bx", "by", "bz", "ref"):
                row = t.nodes[f][i].copy()
                t.nodes[f][i, s:3] = row[s + 1:4]
                t.nodes[f][i, k - 1] = M.UNUSED if f == "ref" else M.INVERTED
            return
    raise AssertionError("no node with three children")


def used_after_unused(t, v):
    i = int(np.argmax(_nused(t) == 3))
    assert _nused(t)[i] == 3
    for f in ("bx", "by", "bz", "ref"):
        t.nodes[f][i, 3], t.nodes[f][i, 2] = t.nodes[f][i, 2], (M.UNUSED if f == "ref" else M.INVERTED)


def unused_box_not_inverted(t, v):
    i = int(np.argmax(_nused(t) < 4))
    assert _nused(t)[i] < 4
    t.nodes["by"][i, 3] = 0x00010000


def swap_far_triangles(t, v):
    c = np.asarray(v).reshape(-1, 3, 3).mean(axis=1)
    far = int(np.argmax(((c[t.order] - c[t.order[0]]) ** 2).sum(-1)))
    t.order[0], t.order[far] = t.order[far], t.order[0]


MUTANTS = {
    "leaf_box_one_step_tight": (shrink_leaf_box, "triangle outside its leaf box"),
    "triangle_in_two_leaves": (duplicate_triangle, "triangle in two leaves"),
    "leaf_dropped": (drop_leaf, "triangle in no leaf"),
    "used_slot_after_unused": (used_after_unused, "unused slot before a used one"),
    "unused_slot_box_not_inverted": (unused_box_not_inverted, "unused slot without the inverted box"),
    "far_triangles_swapped": (swap_far_triangles, "triangle outside its leaf box"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_checker_reports_each_broken_invariant(prt_lib, tmp_path, monkeypatch, mutant):
    data = M.soup(4097)
    tree, info = host_tree(data, tmp_path, monkeypatch)
    M.check_tree(tree, data.vertices, info)
    fn, msg = MUTANTS[mutant]
    bad = tree.copy()
    fn(bad, data.vertices)
    with pytest.raises(M.BVHCheckError, match=msg):
        M.check_tree(bad, data.vertices)


def _quantise(v, origin, step, up):
    q = np.ceil((v - origin) / step) if up else np.floor((v - origin) / step)
    q = np.clip(q, 0, 65535)
    if up:
        while (bad := (q < 65535) & (origin + q * step < v)).any():
            q[bad] += 1
    else:
        while (bad := (q > 0) & (origin + q * step > v)).any():
            q[bad] -= 1
    return q.astype(np.uint32)


def chain_tree(vertices, per_node=3):
    """A tree that is right in every respect but depth: a chain of 4-wide nodes, each with `per_node` one-triangle leaves
    and the next node in its last slot.  Stack need = 3 per node."""
    lo, hi, delta, _ = M.tri_boxes(vertices)
    n = lo.shape[0]
    k = (n - 1) // per_node
    assert k * per_node + 1 == n
    origin = np.float32(lo.min(0) - 2 * delta).astype(np.float64)
    origin = np.where(origin > lo.min(0) - 2 * delta, np.nextafter(origin.astype(np.float32), np.float32(-np.inf)), origin)
    step = ((hi.max(0) + delta - origin) / 65535.0).astype(np.float32)
    step = np.where(origin + 65535.0 * step.astype(np.float64) < hi.max(0) + delta, np.nextafter(step, np.float32(np.inf)), step)
    step = step.astype(np.float64)
    qlo = _quantise(lo - delta, origin, step, False)
    qhi = _quantise(hi + delta, origin, step, True)
    nodes = np.zeros(k, dtype=M.NODE)
    for j in range(k):
        last = j == k - 1
        tris = list(range(j * per_node, (j + 1) * per_node)) + ([n - 1] if last else [])
        for s, tri in enumerate(tris):
            for a, f in enumerate(("bx", "by", "bz")):
                nodes[f][j, s] = qlo[tri, a] | (qhi[tri, a] << 16)
            nodes["ref"][j, s] = ~np.int32(tri << 3)
        if not last:  # the rest of the chain: the box of every later triangle
            for a, f in enumerate(("bx", "by", "bz")):
                nodes[f][j, 3] = qlo[(j + 1) * per_node:, a].min() | (qhi[(j + 1) * per_node:, a].max() << 16)
            nodes["ref"][j, 3] = j + 1
    t = M.Tree(n, 0, k, 0, origin, step, 1.0, nodes, np.arange(n))
    t.stack_need = M.stack_need(t)
    return t


def test_checker_reports_a_stack_need_beyond_the_bound(prt_lib):
    def line(n):
        x = np.arange(n, dtype=np.float64)
        return (M._TRI[None] * 0.5 + np.stack([x, 0 * x, 0 * x], -1)[:, None, :])

    ok = line(3 * 13 + 1)  # 13 nodes: need 39
    t = chain_tree(ok)
    assert M.check_tree(t, ok)["stack_need"] == 39
    deep = line(3 * 14 + 1)  # 14 nodes: need 42
    with pytest.raises(M.BVHCheckError, match="stack need 42 exceeds PRT_STACK_DEPTH 40"):
        M.check_tree(chain_tree(deep), deep)


def test_checker_rejects_a_shifted_grid(prt_lib, tmp_path, monkeypatch):
    """The dequantisation itself is checked: a grid origin one step too high moves every box off its triangles."""
    data = M.translated(M.soup(1024))
    tree, _ = host_tree(data, tmp_path, monkeypatch)
    bad = tree.copy()
    bad.origin = bad.origin + bad.step
    with pytest.raises(M.BVHCheckError, match="outside its leaf box"):
        M.check_tree(bad, data.vertices)
