"""GPU tests (-m gpu) of the in-place geometry update (prt_scene_refit, include/prt.h; kernels in bvh_refit.hip): the refitted
tree against the fp64 tree model (tests/bvh_model.py), the refitted scene's hits and frames against a fresh scene made
from the new positions, the device-pointer entry, the refusals, and the ordering against calls in flight.

Scenes: the adversarial generators of bvh_model at their default sizes, one and two triangles, and a small cornell box
(whose light must stay put: a motion there moves every triangle that belongs to no light mesh).  Both builders.
Motions: the affine map of test_moving_geometry_rebuilds_a_valid_tree, a per-vertex sinusoidal displacement of 10 % of the
extent, a translation by 1e6 (the grid has to move), and back to the start (the boxes have to shrink again).

Tolerances are the project's: hits 1e-12 max(1, t) (test_gpu_parity.compare_hits), fp32 tier 2 (test_gpu_f32), frames 1e-9.
The share of rays whose t is bit-identical to the fresh scene's is printed (the records are meant to be bit-equal).

Shallow second tree: `geometric` (2,000 triangles, stack need 37) is the generator whose host-built tree carries the
32-entry collapse the fp32 kernels traverse; test_hits_on_a_scene_with_a_shallow_second_tree runs it in fp32.
"""
import copy

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from tests import bvh_model as M
from tests.test_gpu_device_bvh import EPS32, TIE_BOUND, TIE_BOUND_DEFAULT, aimed_rays, min_altitude, representatives, settle_ties
from tests.test_gpu_f32 import trace
from tests.test_gpu_parity import compare_images

pytestmark = pytest.mark.gpu

_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.5], [0.25, 1.0, 0.75]])


def _cornell():
    return scenes.cornell_box(ball_subdiv=2, width=32, height=32)


SCENES = {
    "clusters": M.clusters,
    "flat": M.flat,
    "identical": M.identical,
    "soup3000": lambda: M.soup(3000),
    "mixed_sizes": M.mixed_sizes,
    "one_triangle": lambda: M._scene("one", _TRI[None]),
    "two_triangles": lambda: M._scene("two", np.stack([_TRI, _TRI * 0.5 + np.array([2.0, 0.5, -1.0])])),
    "cornell": _cornell,
}
BUILDERS = [pytest.param(False, id="host"), pytest.param(True, id="device")]


def movable(data):
    """Mask of the triangles that belong to no light mesh (emitters do not move under a refit)."""
    mask = np.ones(data.n_tris, dtype=bool)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = False
    return mask


def affine(v):
    return v * np.array([1.5, 0.75, 1.0]) + np.array([0.25, -0.5, 2.0])


def sine(v, amount=0.1):
    p = v.reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    k = 7.0 / max(ext, 1e-300)
    return v + amount * ext * np.sin(k * v[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3]))


def far(v):
    return v + np.array([1.0e6, -1.0e6, 1.0e6])


def moved(data, fn):
    """The scene's vertices with `fn` applied to every triangle that may move."""
    mask = movable(data)
    v = data.vertices.copy()
    v[mask] = fn(data.vertices[mask])
    return v


def with_vertices(data, v):
    out = copy.copy(data)
    out.vertices = v
    return out


def upload_dumped(data, device_bvh, tmp_path, monkeypatch, tag="start"):
    path = str(tmp_path / f"{tag}.bin")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    return sc, M.read_dump(path)


def refit_dumped(sc, v, tmp_path, monkeypatch, tag, how="host"):
    path = str(tmp_path / f"{tag}.bin")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    if how == "host":
        sc.refit(v)
    else:
        import torch
        d = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        torch.cuda.synchronize()
        sc.refit_device(d.data_ptr())
        torch.cuda.synchronize()
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    return M.read_dump(path), open(path, "rb").read()


def check_refitted(tree, start, v, info):
    """The model's invariants for the new vertices, the untouched topology, exact inner unions, tight leaves."""
    M.check_tree(tree, v, info)
    assert np.array_equal(tree.nodes["ref"], start.nodes["ref"]), "a refit changed node refs"
    assert np.array_equal(tree.order, start.order), "a refit changed the leaf order"
    refs = tree.nodes["ref"].astype(np.int64)
    used = refs != M.UNUSED
    q = tree.qboxes()
    # every inner slot is the exact integer union of its child's used slots
    pi, ps = np.nonzero(used & (refs >= 0))
    child = refs[pi, ps]
    cu = used[child][..., None]
    lo = np.where(cu, q[child, :, :, 0], 1 << 20).min(axis=1)
    hi = np.where(cu, q[child, :, :, 1], -1).max(axis=1)
    assert np.array_equal(q[pi, ps, :, 0], lo) and np.array_equal(q[pi, ps, :, 1], hi), "inner slot is not its child's union"
    # no leaf slot is looser than 2 grid steps beyond its triangles' widened fp64 boxes: one step for the outward
    # quantisation, one for the fp32 outward rounding relative to the origin (below 1e-3 of a step)
    tlo, thi, delta, _ = M.tri_boxes(v)
    box = tree.boxes()
    li, ls = np.nonzero(used & (refs < 0))
    first, cnt = M.decode_leaf(refs[li, ls])
    for k in range(1, M.LEAF_MAX + 1):
        sel = cnt == k
        if not sel.any():
            continue
        tri = tree.order[first[sel, None] + np.arange(k)[None, :]]  # (leaves, k)
        ulo, uhi = (tlo[tri] - delta).min(axis=1), (thi[tri] + delta).max(axis=1)
        blo, bhi = box[li[sel], ls[sel], :, 0], box[li[sel], ls[sel], :, 1]
        assert (blo >= ulo - 2.0 * tree.step).all() and (bhi <= uhi + 2.0 * tree.step).all(), "a leaf box did not shrink to its triangles"


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_refitted_tree_against_the_model(dev_lib, tmp_path, monkeypatch, name, device_bvh):
    """affine, then the sinusoidal displacement, then 1e6 away, then back to the start: after each refit the dumped tree
    passes the model's checks for the new vertices with the topology untouched, inner slots exact and leaf slots tight."""
    data = SCENES[name]()
    sc, start = upload_dumped(data, device_bvh, tmp_path, monkeypatch)
    info0 = sc.bvh_info()
    steps = [("affine", moved(data, affine)), ("sine", moved(data, sine)), ("far", moved(data, far)), ("back", data.vertices.copy())]
    for i, (tag, v) in enumerate(steps):
        tree, _ = refit_dumped(sc, v, tmp_path, monkeypatch, tag)
        check_refitted(tree, start, v, sc.bvh_info())
        ri = sc.refit_info()
        assert ri["refits"] == i + 1 and ri["host_stale"] == 0
        assert np.array_equal(np.float32(ri["grid_origin"]), np.float32(tree.origin)) and np.array_equal(np.float32(ri["grid_step"]), np.float32(tree.step))
        # sah_ratio is the model's SAH cost of this tree over that of the tree as built
        want = M.sah_cost(tree) / M.sah_cost(start)
        assert abs(ri["sah_ratio"] - want) <= 1e-9 * want, (ri["sah_ratio"], want)
        print(f"[refit] {name} {'device' if device_bvh else 'host'} {tag}: sah_ratio {ri['sah_ratio']:.4f} "
              f"records {ri['records_ms']:.3f} ms boxes {ri['boxes_ms']:.3f} ms")
    back = sc.refit_info()
    assert abs(back["sah_ratio"] - 1.0) <= 1e-6  # the start geometry again: the start boxes again
    info = sc.bvh_info()
    for f in ("n_nodes", "depth", "render_variant", "texture_bytes", "stack_need", "built_on_device"):
        assert info[f] == info0[f], f
    sc.close()


def scene_rays(v, seed=4):
    rays, _ = aimed_rays(v, seed=seed)
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    pad = 0.25 * np.maximum(hi - lo, 1e-3)
    return np.concatenate([rays, scenes.random_rays(2000, lo - pad, hi + pad, seed=seed + 1)])


def trace_dev(sc, rays, precision=_abi.PRECISION_F64, sort=False):
    import torch
    rays = np.ascontiguousarray(rays, dtype=_abi.RAY_DTYPE)
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
    d_h = torch.zeros((rays.shape[0], 4), dtype=torch.float64, device="cuda")
    d_o = torch.full((rays.shape[0],), 7, dtype=torch.uint8, device="cuda")
    sc.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr(), precision=precision, sort=sort)
    sc.trace_occluded_device(d_r.data_ptr(), rays.shape[0], d_o.data_ptr(), precision=precision, sort=sort)
    torch.cuda.synchronize()
    return d_h.cpu().numpy().view(_abi.HIT_DTYPE).reshape(-1), d_o.cpu().numpy()


def assert_same_hits(g, ref, rays, v, label):
    """t, alpha, beta within 1e-12 max(1, t); prim and front equal after settle_ties' treatment of exact ties."""
    rep = representatives(v)
    g, ref, ties = settle_ties(g, ref, rays, v, rep)
    assert np.array_equal(g["prim"] >= 0, ref["prim"] >= 0), label
    hit = ref["prim"] >= 0
    tol = 1e-12 * np.maximum(1.0, ref["t"][hit])
    for f in ("t", "alpha", "beta"):
        assert (np.abs(g[f][hit] - ref[f][hit]) <= tol).all(), (label, f, float(np.abs(g[f][hit] - ref[f][hit]).max()))
    assert np.array_equal(g["prim"][hit], ref["prim"][hit]) and np.array_equal(g["front"][hit], ref["front"][hit]), label
    same = hit & (g["prim"] == ref["prim"])
    share = float((g["t"][same] == ref["t"][same]).mean()) if same.any() else 1.0
    print(f"[refit] {label}: {int(hit.sum())} hits, {ties} ties, t bit-identical on {100.0 * share:.4f} % of equal prims")
    return share


def fp32_scale(rays, tri, t):
    """Largest magnitude the fp32 kernel rounds on the way to a hit: the origin's and the vertices' coordinates, and t."""
    return np.maximum(np.maximum(np.abs(rays["o"]).max(-1), np.abs(tri).reshape(-1, 9).max(-1)), np.abs(t))


def ray_meets(rays, tri, t):
    """Per ray, in fp64: the ray meets its triangle's plane within 1e-5 max(1, t) of `t`, at a point inside the triangle or
    within a slack of its rim.  The slack, in barycentric units, is tier 2's 2e-3 on alpha and beta plus what the fp32
    kernel cannot resolve: it sees origin, direction and vertices rounded to fp32, so the point is known to about
    eps32 * (largest of the origin's and the vertices' coordinates and t) per rounding, 16 roundings allowed for, and a
    barycentric coordinate moves by that length over the triangle's smallest altitude (`geometric` has triangles of 1e-9
    beside coordinates of 1e3: fp32 cannot tell where inside such a triangle a ray passes, only that it is there)."""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.cross(e1, e2)
    nn, dn = (n * n).sum(-1), (rays["d"] * n).sum(-1)
    ok = (nn > 0) & (dn != 0)
    nn, dn = np.where(ok, nn, 1.0), np.where(ok, dn, 1.0)
    tp = ((tri[:, 0] - rays["o"]) * n).sum(-1) / dn
    w = rays["o"] + tp[:, None] * rays["d"] - tri[:, 0]
    b1, b2 = (np.cross(w, e2) * n).sum(-1) / nn, (np.cross(e1, w) * n).sum(-1) / nn
    slack = 2e-3 + 16.0 * EPS32 * fp32_scale(rays, tri, t) / np.maximum(min_altitude(tri), 1e-300)
    inside = np.minimum(np.minimum(b1, b2), 1.0 - b1 - b2) >= -slack
    return ok & inside & (np.abs(tp - t) <= 1e-5 * np.maximum(1.0, np.abs(t)))


def assert_same_hits_tier2(g, ref, rays, v, label, scene):
    """Tier 2 (test_gpu_f32): for all but 1e-4 of the rays, |dt| <= 1e-5 max(1, t) and the same primitive or a neighbour
    at the same t; alpha and beta within 2e-3 on the same primitive.

    test_gpu_f32.check_hits_tier2 also caps the share of neighbours at 1 %, a figure for random rays.  Six in seven of
    aimed_rays' rays go through a vertex or an edge midpoint, where two trees of different topology over one scene
    name different primitives at one t on 2 % of the rays already in fp64 (TIE_BOUND in test_gpu_device_bvh), and the
    refitted tree keeps the old topology while the fresh scene builds a new one.  So each differing pair is verified in
    fp64 (ray_meets: each scene's primitive is met by the ray at the other's t, to what fp32 resolves), and one that is
    not counts against the same 1e-4 as a miss or a far t.  The share of verified neighbours is capped as well, at
    test_gpu_device_bvh's bound on exact ties between two topologies for these rays on this scene (TIE_BOUND, 1e-3 where
    it names none): that guards against a refit that mislabels primitives wholesale.  Pairs with a triangle fp32 does
    not resolve (smallest altitude below the 16 roundings of ray_meets: `geometric`'s small decades, which all sit on
    one fp32 point) are left out of that share: which of them a kernel names is a matter of traversal order."""
    n = ref.shape[0]
    tris = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    flip = (g["prim"] >= 0) != (ref["prim"] >= 0)
    both = (g["prim"] >= 0) & (ref["prim"] >= 0)
    dt = np.abs(np.where(both, g["t"], 0.0) - np.where(both, ref["t"], 0.0))
    far_t = both & (dt > 1e-5 * np.maximum(1.0, ref["t"]))
    diff = np.nonzero(both & ~far_t & (g["prim"] != ref["prim"]))[0]
    twin = ray_meets(rays[diff], tris[g["prim"][diff]], ref["t"][diff]) & ray_meets(rays[diff], tris[ref["prim"][diff]], g["t"][diff])
    ta, tb = tris[g["prim"][diff]], tris[ref["prim"][diff]]
    resolved = (min_altitude(ta) >= 16.0 * EPS32 * fp32_scale(rays[diff], ta, ref["t"][diff])) & \
               (min_altitude(tb) >= 16.0 * EPS32 * fp32_scale(rays[diff], tb, ref["t"][diff]))
    cap = TIE_BOUND.get(scene, TIE_BOUND_DEFAULT)
    same = both & ~far_t & (g["prim"] == ref["prim"])
    dab = max(float(np.abs(g[f][same] - ref[f][same]).max()) if same.any() else 0.0 for f in ("alpha", "beta"))
    print(f"[refit] fp32 {label}: {n} rays, {int(flip.sum())} flips, {int(far_t.sum())} far, {diff.size} neighbours of which "
          f"{int((~twin).sum())} unverified and {int(resolved.sum())} between resolved triangles (cap {cap * n:.0f}), alpha/beta within {dab:.2e}, t bit-identical on {100.0 * float((g['t'] == ref['t']).mean()):.4f} %")
    assert flip.sum() + far_t.sum() + (~twin).sum() <= 1e-4 * n, (label, int(flip.sum()), int(far_t.sum()), int((~twin).sum()), n)
    assert resolved.sum() <= cap * n, (label, int(resolved.sum()), n)
    assert dab <= 2e-3, (label, dab)


MOTIONS = {"affine": affine, "sine": sine, "far": far}


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_hits_equal_a_fresh_scene(dev_lib, tmp_path, monkeypatch, name, device_bvh):
    """After each motion (and after the way back from 1e6) the refitted scene answers rays as api.Scene(new data) does:
    closest hits within the hit tolerance, the any-hit bytes equal on every ray; as given and sorted."""
    data = SCENES[name]()
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    for tag, v in [(k, moved(data, fn)) for k, fn in MOTIONS.items()] + [("back", data.vertices.copy())]:
        sc.refit(v)
        fresh = api.Scene(with_vertices(data, v)).upload(0)
        rays = scene_rays(v)
        for sort in (False, True):
            (g, go), (r, ro) = trace_dev(sc, rays, sort=sort), trace_dev(fresh, rays, sort=sort)
            assert np.array_equal(go, ro), f"{tag}: occlusion bytes differ on {int((go != ro).sum())} rays"
            assert np.array_equal(go, (g["prim"] >= 0).astype(np.uint8))
            assert_same_hits(g, r, rays, v, f"{name} {tag} sort={sort}")
        fresh.close()
    sc.close()


@pytest.mark.parametrize("tables_first", [False, True], ids=["tables_after", "tables_before"])
@pytest.mark.parametrize("name", ["soup3000", "cornell"])
def test_fp32_hits_equal_a_fresh_scene(dev_lib, name, tables_first):
    """PRT_PRECISION_F32 on the refitted scene against PRT_PRECISION_F32 on a fresh scene, tier 2; with the fp32 tables made
    before the refit (they are re-derived on the device) and after it (they are derived from the refitted records)."""
    data = SCENES[name]()
    sc = api.Scene(data).upload(0)
    if tables_first:
        trace(sc, scene_rays(data.vertices)[:64], _abi.PRECISION_F32)
        assert sc.bvh_info()["render_variant"] >> 8
    v = moved(data, sine)
    sc.refit(v)
    fresh = api.Scene(with_vertices(data, v)).upload(0)
    rays = scene_rays(v)
    (g, go), (r, ro) = trace_dev(sc, rays, precision=_abi.PRECISION_F32), trace_dev(fresh, rays, precision=_abi.PRECISION_F32)
    assert_same_hits_tier2(g, r, rays, v, f"{name} tables_first={tables_first}", name)
    assert (go != ro).sum() <= 1e-4 * rays.shape[0]
    sc.close()
    fresh.close()


@pytest.mark.parametrize("tables_first", [False, True], ids=["tables_after", "tables_before"])
def test_hits_on_a_scene_with_a_shallow_second_tree(dev_lib, tables_first):
    """`geometric` (2,000 triangles over 12 decades): its host-built tree needs 37 stack entries, so the scene carries the
    32-entry collapse that the fp32 kernels traverse.  Both node arrays follow the refit: fp64 hits (full tree) within the
    hit tolerance and fp32 hits (shallow tree) at tier 2, against a fresh scene."""
    data = M.geometric()
    sc = api.Scene(data).upload(0)
    assert sc.bvh_info()["stack_need"] > 32 and sc.bvh_info()["built_on_device"] == 0
    if tables_first:
        trace(sc, scene_rays(data.vertices)[:64], _abi.PRECISION_F32)
    v = affine(data.vertices)
    sc.refit(v)
    fresh = api.Scene(with_vertices(data, v)).upload(0)
    rays = scene_rays(v)
    (g, go), (r, ro) = trace_dev(sc, rays), trace_dev(fresh, rays)
    assert np.array_equal(go, ro)
    assert_same_hits(g, r, rays, v, "geometric affine")
    (g, go), (r, ro) = trace_dev(sc, rays, precision=_abi.PRECISION_F32), trace_dev(fresh, rays, precision=_abi.PRECISION_F32)
    assert_same_hits_tier2(g, r, rays, v, f"geometric tables_first={tables_first}", "geometric")
    assert (go != ro).sum() <= 1e-4 * rays.shape[0]
    sc.close()
    fresh.close()


def test_first_fp32_call_waits_for_a_refit_on_a_side_stream(dev_lib):
    """refit_device on a non-blocking stream, then at once the scene's first PRT_PRECISION_F32 call on the null stream: the
    float tables are derived from the records the refit is writing, so their conversion has to wait for its end.  A
    60,000-triangle soup, so that the writing phases take a while; the fp32 hits are a fresh scene's at tier 2."""
    import torch
    data = M.soup(60_000)
    v = moved(data, sine)
    rays = scene_rays(v)
    sc = api.Scene(data).upload(0)
    side = torch.cuda.Stream()
    d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    torch.cuda.synchronize()
    sc.refit_device(d_v.data_ptr(), stream=side.cuda_stream)
    g, go = trace_dev(sc, rays, precision=_abi.PRECISION_F32)
    fresh = api.Scene(with_vertices(data, v)).upload(0)
    r, ro = trace_dev(fresh, rays, precision=_abi.PRECISION_F32)
    assert_same_hits_tier2(g, r, rays, v, "soup60000 side stream", "soup60000")
    assert (go != ro).sum() <= 1e-4 * rays.shape[0]
    sc.close()
    fresh.close()


@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_device_pointers(dev_lib, tmp_path, monkeypatch, device_bvh):
    """refit_device from a float64 torch tensor: the same dump byte for byte and the same hits as refit from the same
    numbers; afterwards the host geometry is stale (upload refused) until update_vertices replaces every position."""
    data = _cornell()
    v = moved(data, sine)
    a, _ = upload_dumped(data, device_bvh, tmp_path, monkeypatch, "a")
    b, _ = upload_dumped(data, device_bvh, tmp_path, monkeypatch, "b")
    _, raw_a = refit_dumped(a, v, tmp_path, monkeypatch, "ra", how="host")
    _, raw_b = refit_dumped(b, v, tmp_path, monkeypatch, "rb", how="device")
    assert raw_a == raw_b
    rays = scene_rays(v)
    (ga, oa), (gb, ob) = trace_dev(a, rays), trace_dev(b, rays)
    assert np.array_equal(ga, gb) and np.array_equal(oa, ob)
    assert b.refit_info()["host_stale"] == 1 and a.refit_info()["host_stale"] == 0
    with pytest.raises(api.PrtError) as e:
        b.upload(0)
    assert e.value.code == _abi.PRT_E_INVALID and "stale" in str(e.value)
    (gb2, _) = trace_dev(b, rays)
    assert np.array_equal(gb2, gb)  # the refused upload left the scene resident
    b.update_vertices(v)
    assert b.refit_info()["host_stale"] == 0
    b.upload(0)
    fresh = api.Scene(with_vertices(data, v)).upload(0)
    assert_same_hits(trace_dev(b, rays)[0], trace_dev(fresh, rays)[0], rays, v, "after update_vertices")
    # a host refit leaves host triangles a later upload can use
    a.upload(0)
    assert_same_hits(trace_dev(a, rays)[0], trace_dev(fresh, rays)[0], rays, v, "upload after a host refit")
    for s in (a, b, fresh):
        s.close()


RENDER = dict(spp=4, max_depth=5, seed=11)


def ball_moved(data, by=(-0.25, 0.15, -0.1)):
    v = data.vertices.copy()
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    m = data.mesh_names.index("ball")
    v[first[m]:first[m + 1]] += np.asarray(by)
    return v


def test_frames_equal_a_fresh_scene(dev_lib):
    """cornell 32x32, spp 4, depth 5, the ball's triangles moved: render() of the refitted scene equals the fresh scene's
    frame within 1e-9 on every pixel.  The scene and motion have no tie pixel: the fresh scene's frame is the same from a
    host-built and from a device-built tree (two different topologies), which is checked first."""
    data = _cornell()
    v = ball_moved(data)
    new = with_vertices(data, v)
    fresh_h, fresh_d = api.Scene(new).upload(0), api.Scene(new, device_bvh=True).upload(0)
    want = fresh_h.render(**RENDER)
    compare_images(fresh_d.render(**RENDER), want, max_bad=0)
    for device_bvh in (False, True):
        sc = api.Scene(data, device_bvh=device_bvh).upload(0)
        info0 = sc.bvh_info()
        assert sc.refit_info()["refits"] == 0
        old = sc.render(**RENDER)
        assert np.abs(old - want).max() > 1e-3  # the motion is visible
        sc.refit(v)
        assert sc.refit_info()["refits"] == 1
        compare_images(sc.render(**RENDER), want, max_bad=0)
        sc.refit(data.vertices)
        assert sc.refit_info()["refits"] == 2
        compare_images(sc.render(**RENDER), old, max_bad=0)
        info = sc.bvh_info()
        for f in ("n_nodes", "depth", "render_variant", "texture_bytes"):
            assert info[f] == info0[f], f
        sc.close()
    fresh_h.close()
    fresh_d.close()


def test_refusals_change_nothing(dev_lib):
    """A moved emitter vertex, a NaN, a coordinate of 1e19: PRT_E_INVALID; a scene that is not uploaded: PRT_E_NO_DEVICE.
    After each refusal the frame and 2,000 random-ray hits are bit-equal to those before, and an accumulator made earlier
    still accepts add(); after a successful refit it refuses add() until reset()."""
    data = _cornell()
    with pytest.raises(api.PrtError) as e:
        api.Scene(data).refit(data.vertices.copy())
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    with pytest.raises(api.PrtError) as e:
        api.Scene(data).refit_device(4096)
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc = api.Scene(data).upload(0)
    lo, hi = data.bounds()
    rays = scenes.random_rays(2000, lo, hi, seed=3)
    frame0, hits0 = sc.render(**RENDER), sc.trace_closest(rays)
    gen_info = sc.refit_info()
    acc = api.Accumulator(sc, max_depth=5, seed=11)
    acc.add(1)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    light = first[data.mesh_names.index("light")]
    ball = first[data.mesh_names.index("ball")]
    bad = []
    v = ball_moved(data)
    v[light + 1, 2, 0] = np.nextafter(v[light + 1, 2, 0], 1.0)  # one ulp on one light vertex
    bad.append(("light", v))
    for what, x in (("nan", np.nan), ("inf", np.inf), ("1e19", 1e19)):
        v = ball_moved(data)
        v[ball + 5, 1, 2] = x
        bad.append((what, v))
    for what, v in bad:
        for how in ("host", "device"):
            with pytest.raises(api.PrtError) as e:
                if how == "host":
                    sc.refit(v)
                else:
                    import torch
                    d = torch.from_numpy(v).cuda()
                    torch.cuda.synchronize()
                    sc.refit_device(d.data_ptr())
            assert e.value.code == _abi.PRT_E_INVALID, (what, how)
            if what == "light":
                assert "prt_scene_update_vertices" in str(e.value)
            assert np.array_equal(sc.render(**RENDER), frame0), (what, how)
            assert np.array_equal(sc.trace_closest(rays), hits0), (what, how)
            assert sc.refit_info() == gen_info
            acc.add(1)  # the generation was not bumped
    sc.refit(ball_moved(data))
    with pytest.raises(api.PrtError) as e:
        acc.add(1)
    assert e.value.code == _abi.PRT_E_INVALID
    acc.reset().add(2)
    fresh = api.Scene(with_vertices(data, ball_moved(data))).upload(0)
    compare_images(acc.image(), fresh.render(spp=2, max_depth=5, seed=11), max_bad=0)
    acc.close()
    sc.close()
    fresh.close()


def test_ordering_against_calls_in_flight(dev_lib):
    """render_device on stream A, refit_device on stream B, render_device on stream A into a second buffer: the first frame
    is the old geometry's, the second the new geometry's (both against fresh scenes, 1e-9)."""
    import torch
    # 256 x 256 at spp 64 keeps the first render busy for far longer than the refit's host work takes, and a refit to the
    # start positions beforehand leaves this one nothing to allocate: the first render is in flight when the refit is issued
    data = scenes.cornell_box(ball_subdiv=2, width=256, height=256)
    v = ball_moved(data)
    params = dict(spp=64, max_depth=5, seed=11)
    sc = api.Scene(data).upload(0)
    sc.refit(data.vertices)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    cam = data.camera
    f0 = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
    f1 = torch.zeros_like(f0)
    d_v = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    sc.render_device(f0.data_ptr(), None, stream=sa.cuda_stream, **params)
    sc.refit_device(d_v.data_ptr(), stream=sb.cuda_stream)
    sc.render_device(f1.data_ptr(), None, stream=sa.cuda_stream, **params)
    torch.cuda.synchronize()
    old, new = api.Scene(data).upload(0), api.Scene(with_vertices(data, v)).upload(0)
    compare_images(f0.cpu().numpy(), old.render(**params), max_bad=0)
    compare_images(f1.cpu().numpy(), new.render(**params), max_bad=0)
    for s in (sc, old, new):
        s.close()
