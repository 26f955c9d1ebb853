"""The node visit's push tail and its 32-bit node offset (Trav::inner_step), where the other scenes do not reach.

inner_step counts the children that are hit, forms ONE address from the new top of the stack and stores the far children at
fixed distances below it, each under its own condition.  What can go wrong with that shows only where the stack is used up
to the entries the launch reserved for it and where every number of hit children occurs, with and without unused slots — on
the suite's other scenes a ray rarely hits more than two children of a node and the stack stays far from its end.  So:

  the scene   250 thin slivers nested inside each other along x (every one inside the span of a longer one) and a quad light:
              a ray along x passes through the boxes of most nodes at every level.  test_the_scene_reaches_the_stacks_bound
              asserts on the DUMPED tree that a ray of the batch reaches a stack depth within 3 entries of tree_stack_need,
              which is what a launch reserves (PrtBvhInfo.stack_need), and that node visits with 0, 1, 2, 3 and 4 hit children
              all occur, among them visits of nodes whose slot 3, and whose slots 2 and 3, are unused;
  K1          4,096 rays (half along x through the bundle, half from around the scene), closest and any-hit: hits, node
              fetches and triangle tests equal the fp64 model of the walk (tests/traversal_model.py), compared as
              test_gpu_traversal_work.py compares them (the rays every decision of which is robust, at most 5 % excluded);
  K3          16 x 16 at spp 2 through the lean kernel: the oracle's frame and ray counts; the counting run gives the
              same frame, and its node fetches, triangle tests and full tests are those of ITS OWN ray stream
              (PRT_TUNE_DUMP_RAYS) replayed through K1 — exactly, all rays — while K1 equals the model on the stream's robust rays;
  thresholds  all of it again at the dev-hook settings KEEP 0 / LEAF_BATCH 1 and CHAIN_MIN 65 (no lane chained in the wave loop);
  the limit   a tree that claims 2^26 + 1 nodes (PRT_TEST_CLAIM_NODES: nothing of that size is allocated) is refused with
              PRT_E_LIMIT when the scene is created, on the CPU; one that claims 2^26 is accepted; the shipped library reads
              no hook.  The same claim behind the device builder is refused at upload and at rebuild, and both leave the scene
              as it was.  (build_bvh's and validate_nodes' own checks see real trees only: nothing of 4 GB is built here.)
"""
import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from pooraytracer_amd.scenes import Material
from tests import bvh_model as M
from tests import hit_certifier as H
from tests import traversal_model as T
from tests.test_gpu_kernel_matrix import PERMS, VALID, _close, _render_counting, variant
from tests.test_gpu_parity import assert_ray_counts, compare_images
from tests.test_gpu_traversal_work import COUNTERS, _explain, _launch, _mismatch
from tests.test_gpu_wave_loop import THRESHOLDS, _set

F64 = _abi.PRECISION_F64
N_SLIVERS, N_RAYS, N_TRACED = 250, 4096, 64
RENDER_KW = dict(spp=2, max_depth=8, seed=11)
MAX_NODES = 1 << 26


def nest_scene():
    """Slivers of half-length 1.0 down to 0.35 along x, about 0.15 wide, their centres within 0.06 of the x axis, slightly
    tilted out of each other's planes; a quad light above them; the camera looks down the x axis into the bundle."""
    rng = np.random.default_rng(5)
    n = N_SLIVERS
    b = scenes._Builder("visit-tail")
    white = b.material(Material("White", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    light = b.material(Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=(14.0, 13.0, 11.0)))
    half = np.linspace(1.0, 0.35, n)
    rng.shuffle(half)
    cy, cz = rng.uniform(-0.06, 0.06, n), rng.uniform(-0.06, 0.06, n)
    w = rng.uniform(0.05, 0.09, n)
    tilt = rng.uniform(-0.04, 0.04, n)
    tris = np.empty((n, 3, 3))
    tris[:, 0] = np.stack([-half, cy - w, cz - tilt], 1)
    tris[:, 1] = np.stack([half, cy - w, cz + tilt], 1)
    tris[:, 2] = np.stack([rng.uniform(-0.2, 0.2, n) * half, cy + w, cz + rng.uniform(-0.03, 0.03, n)], 1)
    b.mesh("nest", white, tris)
    b.mesh("light", light, *scenes.quad((-0.4, 0.6, -0.4), (0.4, 0.6, -0.4), (0.4, 0.6, 0.4), (-0.4, 0.6, 0.4)))
    return b.build(scenes.Camera(16, 16, 12.0, eye=(-2.5, 0.02, 0.01), look_at=(0.0, 0.0, 0.0)))


def nest_rays(data):
    """The first half along the long axis through the bundle, in both directions; the second from a box 30 % larger than the scene."""
    rng = np.random.default_rng(3)
    lo, hi = data.bounds()
    rays = scenes.random_rays(N_RAYS, lo - 0.15 * (hi - lo), hi + 0.15 * (hi - lo), seed=3)
    k = N_RAYS // 2
    o = np.stack([np.full(k, -1.6), rng.uniform(-0.1, 0.1, k), rng.uniform(-0.08, 0.08, k)], 1)
    d = np.stack([np.ones(k), rng.uniform(-0.03, 0.03, k), rng.uniform(-0.03, 0.03, k)], 1)
    d[::2] *= -1
    o[::2, 0] *= -1
    rays["o"][:k] = o
    rays["d"][:k] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return rays


def visit_stats(tree, vertices, rays):
    """Of the visit traces of `rays` (one model walk each): node visits by number of hit children, the same for nodes with
    one and with two unused slots, and the deepest stack — a visit with h hits leaves h - 1 entries more (it descends into the
    nearest), a visit without a hit and every leaf pop one."""
    hist, one_unused, two_unused, deepest = np.zeros(5, int), np.zeros(5, int), np.zeros(5, int), 0
    for i in range(rays.shape[0]):
        trace, sp = [], 0
        T.walk(tree, vertices, rays[i:i + 1], False, H.U64, trace=trace)
        for ev in trace:
            if ev[0] == "node":
                h = len(ev[3])
                hist[h] += 1
                unused = sum(s[0] == M.UNUSED for s in ev[2])
                one_unused[h] += unused == 1
                two_unused[h] += unused == 2
                sp += h - 1 if h else -1
            else:
                sp -= 1
            deepest = max(deepest, sp)
    return hist, one_unused, two_unused, deepest


_DATA = {}


def _data():
    if not _DATA:
        _DATA["data"] = nest_scene()
        _DATA["rays"] = nest_rays(_DATA["data"])
    return _DATA["data"], _DATA["rays"]


def _resident(tmp_path, monkeypatch):
    """(the scene on the GPU, the tree its kernels walk): host-built, validated, dumped, checked against the vertices."""
    data, _ = _data()
    path = str(tmp_path / "tree.bin")
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    sc = api.Scene(data).upload(0)
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    tree = M.read_dump(path)
    M.check_tree(tree, data.vertices, sc.bvh_info())
    return sc, tree


def _walks(tree, rays, key):
    """The model's closest and any-hit walks of a batch, computed once per batch (the tree is the same in every test: the host
    builder is deterministic; asserted through the node count)."""
    if key not in _DATA:
        data, _ = _data()
        rec = T.records(data.vertices, H.U64)
        _DATA[key] = (tree.n_nodes, {a: T.walk(tree, data.vertices, rays, a, H.U64, rec=rec) for a in (False, True)})
    assert _DATA[key][0] == tree.n_nodes
    return _DATA[key][1]


def _check_k1(sc, tree, rays, walks, what):
    """K1's hits and work on the robust rays of `rays` against the model; returns the (closest, occluded) counters of ALL rays."""
    data, _ = _data()
    E = sc.refit_info()["slab_scale"]
    assert E == T.slab_scale(tree)
    n = rays.shape[0]
    for any_hit, kind in ((False, "closest"), (True, "occluded")):
        w = walks[any_hit]
        idx = np.flatnonzero(w.robust)
        assert n - idx.size <= T.EXCLUDED_MAX * n, (what, w.excluded())
        prim, t, c = _launch(sc, kind, rays[idx], F64)
        print(f"[visit tail] {what} {kind}: {n} rays, excluded {n - idx.size} {w.excluded()}, nodes/ray {w.nodes[idx].mean():.3f}, "
              + ", ".join(f"{k} {c[k]}" for k in COUNTERS))
        bad = _mismatch(c, w, idx)
        if bad:
            pytest.fail(_explain(sc, kind, rays, F64, H.U64, w, idx, tree, data.vertices, E, f"{what}, {kind}: {bad}"))
        assert c["rays_shadow" if any_hit else "rays_closest"] == idx.size
        if any_hit:
            assert np.array_equal(prim, (w.prim[idx] >= 0).astype(np.int64)), what
        else:
            assert np.array_equal(prim, w.prim[idx]), what
            hit = prim >= 0
            assert hit.any() and (~hit).any()
            assert (np.abs(t[hit] - w.t[idx][hit]) <= H.SAME_TOL[H.U64] * np.maximum(1.0, w.t[idx][hit])).all(), what
            assert np.isinf(t[~hit]).all()


@pytest.mark.gpu
def test_the_scene_reaches_the_stacks_bound(gpu, dev_lib, tmp_path, monkeypatch):
    data, rays = _data()
    sc, tree = _resident(tmp_path, monkeypatch)
    need = M.stack_need(tree)
    assert need == sc.bvh_info()["stack_need"] == tree.stack_need  # what a launch reserves per lane
    w = _walks(tree, rays, "batch")[False]
    busiest = np.argsort(-w.nodes, kind="stable")[:N_TRACED]
    hist, one_unused, two_unused, deepest = visit_stats(tree, data.vertices, rays[np.concatenate([busiest, np.arange(N_RAYS - 8, N_RAYS)])])
    print(f"\n[visit tail] {data.n_tris} triangles, {tree.n_nodes} nodes, stack need {need}, deepest stack of a traced ray {deepest}; "
          f"visits by hit children {hist.tolist()}, slot 3 unused {one_unused.tolist()}, slots 2 and 3 unused {two_unused.tolist()}")
    assert need - 3 <= deepest <= need
    assert (hist > 0).all(), hist
    assert (one_unused[:4] > 0).all() and (two_unused[:3] > 0).all(), (one_unused, two_unused)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
def test_k1_walks_the_nest_as_the_model_does(gpu, dev_lib, tmp_path, monkeypatch, thresholds):
    _, rays = _data()
    _set(monkeypatch, THRESHOLDS[thresholds])
    sc, tree = _resident(tmp_path, monkeypatch)
    _check_k1(sc, tree, rays, _walks(tree, rays, "batch"), thresholds)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thresholds", list(THRESHOLDS))
def test_k3_renders_the_nest_and_does_the_work_of_its_rays(gpu, dev_lib, tmp_path, monkeypatch, thresholds):
    data, _ = _data()
    _set(monkeypatch, THRESHOLDS[thresholds])
    sc, tree = _resident(tmp_path, monkeypatch)
    if "oracle" not in _DATA:
        _DATA["oracle"] = oracle.Oracle(data).render(nthreads=8, **RENDER_KW)
    ref, ref_cnt = _DATA["oracle"]
    assert ref.max() > 0 and ref_cnt["rays_shadow"] > 0
    img = sc.render(**RENDER_KW)
    cnt = sc.counters()
    assert variant(sc) & VALID and variant(sc) & _abi.VARIANT_PERM_MASK == PERMS["lean"]
    assert compare_images(img, ref) == 0
    assert_ray_counts(cnt, ref_cnt)
    # the counting run, its rays written out in the order its waves start them
    path = str(tmp_path / "rays.bin")
    monkeypatch.setenv("PRT_TUNE_DUMP_RAYS", f"{1 << 20},{path}")
    cimg, ccnt = _render_counting(sc, **RENDER_KW)
    monkeypatch.delenv("PRT_TUNE_DUMP_RAYS")
    assert _close(cimg, img, 1e-12)
    assert (ccnt["rays_closest"], ccnt["rays_shadow"]) == (cnt["rays_closest"], cnt["rays_shadow"])
    stream = np.fromfile(path, dtype=_abi.RAY_DTYPE)
    shadow = stream["tmin"] > 5e-4  # (0.001 against 0.0001)
    assert (int((~shadow).sum()), int(shadow.sum())) == (ccnt["rays_closest"], ccnt["rays_shadow"])
    # K3's work is the work of its rays: the stream through K1, every ray of it
    k1 = {k: 0 for k in ("node_fetches", "tri_tests", "tri_full")}
    for kind, part in (("closest", stream[~shadow]), ("occluded", stream[shadow])):
        _, _, c = _launch(sc, kind, part, F64)
        for k in k1:
            k1[k] += c[k]
    print(f"\n[visit tail] {thresholds}: K3 " + ", ".join(f"{k} {ccnt[k]}" for k in COUNTERS) + f"; its {stream.shape[0]} rays through K1 {k1}")
    assert {k: ccnt[k] for k in k1} == k1
    # ... and K1 walks them as the model does (shadow rays are segments: the any-hit walk; the others the closest-hit walk)
    for any_hit, kind, part in ((False, "closest", stream[~shadow]), (True, "occluded", stream[shadow])):
        w = T.walk(tree, data.vertices, part, any_hit, H.U64, E=sc.refit_info()["slab_scale"])
        idx = np.flatnonzero(w.robust)
        assert part.shape[0] - idx.size <= T.EXCLUDED_MAX * part.shape[0], (kind, w.excluded())
        _, _, c = _launch(sc, kind, part[idx], F64)
        bad = _mismatch(c, w, idx)
        if bad:
            pytest.fail(_explain(sc, kind, part, F64, H.U64, w, idx, tree, data.vertices, sc.refit_info()["slab_scale"], f"{thresholds}, K3's {kind} rays: {bad}"))
    sc.close()


def test_a_tree_beyond_the_node_limit_is_refused(prt_lib, monkeypatch):
    """On the CPU: the host builder's tree of a small scene, claimed to have 2^26 + 1 nodes, never becomes a scene."""
    data, _ = _data()
    with api.dev_hooks():
        monkeypatch.setenv("PRT_TEST_CLAIM_NODES", str(MAX_NODES + 1))
        with pytest.raises(api.PrtError) as e:
            api.Scene(data)
        assert e.value.code == _abi.PRT_E_LIMIT and "2^26" in str(e.value) and str(MAX_NODES + 1) in str(e.value), str(e.value)
        monkeypatch.setenv("PRT_TEST_CLAIM_NODES", str(MAX_NODES))
        api.Scene(data).close()
    # the shipped library reads no hook: the claim that the dev-hooks library has just refused means nothing to it
    monkeypatch.setenv("PRT_TEST_CLAIM_NODES", str(MAX_NODES + 1))
    api.Scene(data).close()


@pytest.mark.gpu
def test_the_device_builders_trees_meet_the_same_limit(gpu, dev_lib, monkeypatch):
    """The guards behind the device builder, at upload and at rebuild: a tree that claims 2^26 + 1 nodes is refused with
    PRT_E_LIMIT before it is adopted; the failed upload leaves nothing resident, the failed rebuild leaves the scene as it
    was (its hits are the ones from before)."""
    data, rays = _data()
    over = str(MAX_NODES + 1)
    sc = api.Scene(data, device_bvh=True)  # (nothing is built at create: no tree to claim anything about)
    monkeypatch.setenv("PRT_TEST_CLAIM_NODES", over)
    with pytest.raises(api.PrtError) as e:
        sc.upload(0)
    assert e.value.code == _abi.PRT_E_LIMIT and "prt_scene_upload" in str(e.value) and over in str(e.value), str(e.value)
    monkeypatch.delenv("PRT_TEST_CLAIM_NODES")
    sc.upload(0)  # the scene is back in the not-uploaded state, and uploads
    before = sc.trace_closest(rays[:512])
    monkeypatch.setenv("PRT_TEST_CLAIM_NODES", over)
    with pytest.raises(api.PrtError) as e:
        sc.rebuild(data.vertices)
    assert e.value.code == _abi.PRT_E_LIMIT and "prt_scene_rebuild" in str(e.value) and over in str(e.value), str(e.value)
    monkeypatch.delenv("PRT_TEST_CLAIM_NODES")
    after = sc.trace_closest(rays[:512])
    assert np.array_equal(before["prim"], after["prim"]) and np.array_equal(before["t"], after["t"])
    sc.rebuild(data.vertices)
    sc.close()
