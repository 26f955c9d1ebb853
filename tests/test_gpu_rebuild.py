"""GPU tests (-m gpu) of the device-side rebuild of a resident scene (prt_scene_rebuild*, include/prt.h; kernels in
bvh_refit.hip, the builder in bvh_build_gpu.hip): the rebuilt tree against the fp64 tree model, the rebuilt scene's hits,
surface records and frames against a fresh scene made from the new positions, what the rebuild restores after a refit
has decayed the tree, the refusals and injected failures, and the ordering against calls in flight.

Scenes: the adversarial generators of bvh_model at their default sizes, one and two triangles, a small cornell box and
the multi-material textured box (whose lights stay put: a motion moves every triangle that belongs to no light mesh).
Both start builders.  Tolerances are the project's: hits 1e-12 max(1, t), fp32 tier 2, frames 1e-9 on every pixel.
"""
import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes
from tests import bvh_model as M
from tests.test_gpu_f32 import check_image_tier2, oracle_tier2_reference, trace
from tests.test_gpu_parity import compare_images
from tests.test_gpu_refit import (BUILDERS, MOTIONS, RENDER, SCENES, _cornell, affine, assert_same_hits, assert_same_hits_tier2,
                                  ball_moved, check_refitted, movable, moved, refit_dumped, scene_rays, sine, trace_dev,
                                  upload_dumped, with_vertices)

pytestmark = pytest.mark.gpu
F32 = _abi.PRECISION_F32


def rebuild_dumped(sc, v, tmp_path, monkeypatch, tag, how="host"):
    path = str(tmp_path / f"{tag}.bin")
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    if how == "host":
        sc.rebuild(v)
    else:
        import torch
        d = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        torch.cuda.synchronize()
        sc.rebuild_device(d.data_ptr())
        torch.cuda.synchronize()
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    return M.read_dump(path)


def rebuild_how(sc, v, how):
    if how == "host":
        sc.rebuild(v)
    else:
        import torch
        d = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        torch.cuda.synchronize()
        sc.rebuild_device(d.data_ptr())
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1
TREE_SCENES = dict(SCENES, geometric=M.geometric)


@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", list(TREE_SCENES))
def test_rebuilt_tree_is_a_valid_tree_of_the_new_vertices(dev_lib, tmp_path, monkeypatch, name, device_bvh):
    """affine, the sinusoidal displacement, 1e6 away: after rebuild and after rebuild_device the dumped tree passes the
    model's checks for the new vertices; bvh_info names the device builder and agrees with the dump.  One triangle takes
    the refit path (PRT_OK, a valid tree)."""
    data = TREE_SCENES[name]()
    sc, start = upload_dumped(data, device_bvh, tmp_path, monkeypatch)
    n = data.n_tris
    for tag, fn in MOTIONS.items():
        v = moved(data, fn)
        for how in ("host", "device"):
            tree = rebuild_dumped(sc, v, tmp_path, monkeypatch, f"{tag}_{how}", how)
            info = sc.bvh_info()
            M.check_tree(tree, v, info)
            assert info["stack_need"] == tree.stack_need
            ri = sc.refit_info()
            assert ri["host_stale"] == (1 if how == "device" else 0)
            assert np.array_equal(np.float32(ri["grid_origin"]), np.float32(tree.origin)) and np.array_equal(np.float32(ri["grid_step"]), np.float32(tree.step))
            if n >= 2:
                assert info["built_on_device"] == 1 and tree.built_on_device == 1
                assert ri["sah_ratio"] == 1.0
                assert info["build_ms"] > 0.0
            else:
                assert np.array_equal(tree.nodes["ref"], start.nodes["ref"])
    sc.close()


@pytest.mark.parametrize("tables_first", [False, True], ids=["tables_after", "tables_before"])
def test_rebuild_drops_the_shallow_second_tree(dev_lib, tmp_path, monkeypatch, tables_first):
    """`geometric`: the host-built tree needs more than 32 stack entries, so the scene carries the 32-entry collapse the fp32
    kernels traverse (made resident by the first fp32 call or by the first refit).  The rebuild drops it: fp32 hits
    afterwards are those of the new tree (tier 2 against a fresh scene), fp64 hits within the hit tolerance, and a refit
    after the rebuild works on the new tree alone."""
    data = M.geometric()
    sc = api.Scene(data).upload(0)
    assert sc.bvh_info()["stack_need"] > 32 and sc.bvh_info()["built_on_device"] == 0
    if tables_first:
        trace(sc, scene_rays(data.vertices)[:64], F32)
        assert sc.bvh_info()["render_variant"] >> 8
    else:
        sc.refit(data.vertices.copy())  # (the refit makes the collapse resident too)
    v = affine(data.vertices)
    tree = rebuild_dumped(sc, v, tmp_path, monkeypatch, "rebuilt")
    info = sc.bvh_info()
    M.check_tree(tree, v, info)
    assert info["built_on_device"] == 1 and info["stack_need"] == tree.stack_need
    fresh = api.Scene(with_vertices(data, v), device_bvh=True).upload(0)
    rays = scene_rays(v)
    (g, go), (r, ro) = trace_dev(sc, rays), trace_dev(fresh, rays)
    assert np.array_equal(go, ro)
    assert_same_hits(g, r, rays, v, "geometric rebuilt")
    (g, go), (r, ro) = trace_dev(sc, rays, precision=F32), trace_dev(fresh, rays, precision=F32)
    assert_same_hits_tier2(g, r, rays, v, f"geometric rebuilt tables_first={tables_first}", "geometric")
    assert (go != ro).sum() <= 1e-4 * rays.shape[0]
    v2 = sine(v, 0.01)
    refitted, _ = refit_dumped(sc, v2, tmp_path, monkeypatch, "refit_after")
    check_refitted(refitted, tree, v2, sc.bvh_info())
    fresh2 = api.Scene(with_vertices(data, v2), device_bvh=True).upload(0)
    (g, _), (r, _) = trace_dev(sc, rays, precision=F32), trace_dev(fresh2, rays, precision=F32)
    assert_same_hits_tier2(g, r, rays, v2, "geometric refit after rebuild", "geometric")
    for s in (sc, fresh, fresh2):
        s.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", ["soup3000", "mixed_sizes", "clusters", "two_triangles", "cornell"])
def test_hits_equal_a_fresh_scene(dev_lib, monkeypatch, name, device_bvh):
    """After each motion the rebuilt scene answers 2,000 aimed and 2,000 random rays as a fresh device-built scene of the new
    positions does: closest hits within the hit tolerance, the any-hit bytes equal on every ray; as given and sorted; the
    host form and the device form in turn."""
    data = SCENES[name]()
    monkeypatch.setenv("PRT_VALIDATE_BVH", "1")
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    for i, (tag, fn) in enumerate(MOTIONS.items()):
        v = moved(data, fn)
        rebuild_how(sc, v, ("host", "device")[i % 2])
        fresh = api.Scene(with_vertices(data, v), device_bvh=True).upload(0)
        rays = scene_rays(v)
        for sort in (False, True):
            (g, go), (r, ro) = trace_dev(sc, rays, sort=sort), trace_dev(fresh, rays, sort=sort)
            assert np.array_equal(go, ro), f"{tag}: occlusion bytes differ on {int((go != ro).sum())} rays"
            assert np.array_equal(go, (g["prim"] >= 0).astype(np.uint8))
            assert_same_hits(g, r, rays, v, f"rebuild {name} {tag} sort={sort}")
        fresh.close()
    sc.close()


@pytest.mark.parametrize("tables_first", [False, True], ids=["tables_after", "tables_before"])
@pytest.mark.parametrize("device_bvh", BUILDERS)
@pytest.mark.parametrize("name", ["soup3000", "cornell"])
def test_fp32_hits_equal_a_fresh_scene(dev_lib, name, device_bvh, tables_first):
    """PRT_PRECISION_F32 on the rebuilt scene against PRT_PRECISION_F32 on a fresh scene, tier 2; with the fp32 tables made
    before the rebuild (re-converted, their tree replaced) and after it (derived from the rebuilt records)."""
    data = SCENES[name]()
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    if tables_first:
        trace(sc, scene_rays(data.vertices)[:64], F32)
        assert sc.bvh_info()["render_variant"] >> 8
    v = moved(data, sine)
    rebuild_how(sc, v, "device" if tables_first else "host")
    assert bool(sc.bvh_info()["render_variant"] >> 8) == tables_first
    fresh = api.Scene(with_vertices(data, v), device_bvh=True).upload(0)
    rays = scene_rays(v)
    (g, go), (r, ro) = trace_dev(sc, rays, precision=F32), trace_dev(fresh, rays, precision=F32)
    assert_same_hits_tier2(g, r, rays, v, f"rebuild {name} tables_first={tables_first}", name)
    assert (go != ro).sum() <= 1e-4 * rays.shape[0]
    (g, go), (r, ro) = trace_dev(sc, rays, precision=F32, sort=True), trace_dev(fresh, rays, precision=F32, sort=True)
    assert_same_hits_tier2(g, r, rays, v, f"rebuild {name} tables_first={tables_first} sorted", name)
    sc.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("device_bvh", BUILDERS)
def test_shading_records_went_to_the_right_leaves(dev_lib, device_bvh, how):
    """trace_surface on the multi-material, textured box after a rebuild against a fresh scene's: prim, material,
    material_type, uv, albedo and tangent equal, position and normal within the hit tolerance.  (The intersection records
    are rewritten from the vertices; uv, material and prim only get where they belong through the permutation.)"""
    data = scenes.mixed_materials()
    mask = movable(data)  # ... and the Debug material emits as well: its patch is a light mesh
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DEBUG:
            mask[first[m]:first[m + 1]] = False
    v = data.vertices.copy()
    v[mask] = sine(data.vertices[mask], 0.02)
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    assert len({int(m) for m in data.mesh_material}) > 2
    rebuild_how(sc, v, how)
    fresh = api.Scene(with_vertices(data, v), device_bvh=True).upload(0)
    rays = scene_rays(v)
    g, r = sc.trace_surface(rays), fresh.trace_surface(rays)
    assert np.array_equal(g["prim"] >= 0, r["prim"] >= 0)
    hit = r["prim"] >= 0
    tol = 1e-12 * np.maximum(1.0, np.where(hit, r["t"], 0.0))
    assert (np.abs(g["t"][hit] - r["t"][hit]) <= tol[hit]).all()
    other = hit & (g["prim"] != r["prim"])
    print(f"[rebuild] surface {how}: {int(hit.sum())} hits, {int(other.sum())} on another primitive, t bit-identical on "
          f"{100.0 * float((g['t'][hit] == r['t'][hit]).mean()):.4f} %")
    assert (g["t"][other] == r["t"][other]).all()  # another primitive only on an exact tie in t (test_gpu_parity.compare_hits)
    assert other.sum() <= 0.02 * hit.sum()
    same = hit & ~other
    assert len(np.unique(r["material"][same])) > 2 and (np.abs(r["uv"][same]) > 0).any()
    for f in ("prim", "material", "material_type", "uv", "albedo", "tangent", "front"):
        assert np.array_equal(g[f][same], r[f][same]), f
    for f in ("position", "normal"):
        assert (np.abs(g[f][same] - r[f][same]) <= tol[same, None]).all(), f
    sc.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ 4
def test_frames_equal_a_fresh_scene(dev_lib):
    """cornell 32x32, spp 4, depth 5, the ball moved: the rebuilt scene's fp64 frame equals the fresh scene's within 1e-9 on
    every pixel, its fp32 frame is within tier 2 of the oracle's; an accumulator made before the rebuild refuses add() until
    reset() and then matches the fresh scene."""
    data = _cornell()
    v = ball_moved(data)
    new = with_vertices(data, v)
    fresh = api.Scene(new, device_bvh=True).upload(0)
    want = fresh.render(**RENDER)
    ref32, sigma32 = oracle_tier2_reference(new, RENDER["spp"], max_depth=RENDER["max_depth"], seed=RENDER["seed"])
    for device_bvh in (False, True):
        for how in ("host", "device"):
            sc = api.Scene(data, device_bvh=device_bvh).upload(0)
            old = sc.render(**RENDER)
            assert np.abs(old - want).max() > 1e-3  # the motion is visible
            acc = api.Accumulator(sc, max_depth=5, seed=11)
            acc.add(1)
            rebuild_how(sc, v, how)
            compare_images(sc.render(**RENDER), want, max_bad=0)
            img32, fresh32 = sc.render(precision=F32, **RENDER), fresh.render(precision=F32, **RENDER)
            tol32 = 3.0 * sigma32 / np.sqrt(RENDER["spp"]) + 1e-3 * np.maximum(1.0, np.abs(ref32))
            print(f"[rebuild] fp32 frame: {int((np.abs(img32 - ref32) > tol32).any(-1).sum())} pixels outside tier 2 (the fresh scene's: "
                  f"{int((np.abs(fresh32 - ref32) > tol32).any(-1).sum())}), equal to the fresh scene's bit for bit: {np.array_equal(img32, fresh32)}")
            check_image_tier2(img32, ref32, sigma32, RENDER["spp"])
            with pytest.raises(api.PrtError) as e:
                acc.add(1)
            assert e.value.code == _abi.PRT_E_INVALID
            acc.reset().add(2)
            compare_images(acc.image(), fresh.render(spp=2, max_depth=5, seed=11), max_bad=0)
            # and back: the start geometry through a second rebuild
            rebuild_how(sc, data.vertices.copy(), how)
            compare_images(sc.render(**RENDER), old, max_bad=0)
            acc.close()
            sc.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ 5
def scrambled(data, seed=17):
    """Triangle i takes the vertices of triangle perm[i]: the same set of triangles, every one somewhere else."""
    perm = np.random.default_rng(seed).permutation(data.n_tris)
    return np.ascontiguousarray(data.vertices[perm])


def test_rebuild_restores_what_a_refit_lost(dev_lib, tmp_path, monkeypatch):
    """soup(3000), scrambled.  The refitted tree's multi-triangle leaves span unrelated places: sah_ratio > 1.  A rebuild of
    the same positions: sah_ratio 1.0, a smaller model SAH cost, fewer node fetches for the same rays, the same hits; the
    same SAH cost as update_vertices' tree of the same positions (same builder, boxes meant to be bit-equal: 1e-9 relative,
    summation order).  A refit after the rebuild runs on the new parents and counters."""
    data = M.soup(3000)
    v = scrambled(data)
    rays = scene_rays(v)[:2000]
    sc, _ = upload_dumped(data, False, tmp_path, monkeypatch)
    refitted, _ = refit_dumped(sc, v, tmp_path, monkeypatch, "refitted")
    ratio = sc.refit_info()["sah_ratio"]
    assert ratio > 1.0
    hits_refit = sc.trace_closest(rays, count_work=True)
    fetches_refit = sc.counters()["node_fetches"]
    refits = sc.refit_info()["refits"]
    rebuilt = rebuild_dumped(sc, v, tmp_path, monkeypatch, "rebuilt")
    M.check_tree(rebuilt, v, sc.bvh_info())
    ri = sc.refit_info()
    assert ri["sah_ratio"] == 1.0 and ri["refits"] == refits
    hits_rebuilt = sc.trace_closest(rays, count_work=True)
    fetches_rebuilt = sc.counters()["node_fetches"]
    cost_refit, cost_rebuilt = M.sah_cost(refitted), M.sah_cost(rebuilt)
    print(f"[rebuild] scramble: sah_ratio after the refit {ratio:.1f}; model SAH cost {cost_refit:.1f} -> {cost_rebuilt:.2f}; "
          f"node fetches of 2,000 rays {fetches_refit} -> {fetches_rebuilt}")
    assert cost_rebuilt < cost_refit
    assert fetches_rebuilt < fetches_refit
    assert_same_hits(hits_rebuilt, hits_refit, rays, v, "scramble: rebuilt against refitted")
    # update_vertices of the same positions on a second scene: the same builder on the host's boxes
    path = str(tmp_path / "updated.bin")
    other = api.Scene(data).upload(0)
    monkeypatch.setenv("PRT_TEST_DUMP_BVH", path)
    other.update_vertices(v)
    monkeypatch.delenv("PRT_TEST_DUMP_BVH")
    updated = M.read_dump(path)
    cost_updated = M.sah_cost(updated)
    print(f"[rebuild] scramble: model SAH cost of update_vertices' tree {cost_updated!r}, of the rebuilt tree {cost_rebuilt!r}; "
          f"canonical forms equal: {M.canonical(updated) == M.canonical(rebuilt)}")
    assert abs(cost_rebuilt - cost_updated) <= 1e-9 * cost_updated
    assert_same_hits(hits_rebuilt, other.trace_closest(rays), rays, v, "scramble: rebuilt against update_vertices")
    # a refit after the rebuild
    v2 = sine(v, 0.01)
    again, _ = refit_dumped(sc, v2, tmp_path, monkeypatch, "refit_after")
    check_refitted(again, rebuilt, v2, sc.bvh_info())
    ri = sc.refit_info()
    assert ri["refits"] == refits + 1
    want = M.sah_cost(again) / cost_rebuilt
    assert abs(ri["sah_ratio"] - want) <= 1e-9 * want, (ri["sah_ratio"], want)
    fresh = api.Scene(with_vertices(data, v2), device_bvh=True).upload(0)
    rays2 = scene_rays(v2)[:2000]
    assert_same_hits(sc.trace_closest(rays2), fresh.trace_closest(rays2), rays2, v2, "scramble: refit after the rebuild")
    for s in (sc, other, fresh):
        s.close()


# ------------------------------------------------------------------------------------------------ 6
def _state(sc, rays):
    return sc.render(**RENDER), sc.trace_closest(rays), sc.refit_info(), sc.bvh_info()


def _assert_unchanged(sc, rays, before, label):
    frame, hits, ri, bi = _state(sc, rays)
    assert np.array_equal(frame, before[0]), label
    assert np.array_equal(hits, before[1]), label
    assert ri == before[2], label
    assert bi == before[3], label


def test_refusals_change_nothing(dev_lib):
    """A light vertex moved by one ulp, a NaN, 1e19, through the host call and through the device pointer: PRT_E_INVALID, and
    the frame, 2,000 hits, refit_info() and bvh_info() are bit-equal to before; an accumulator made earlier still accepts
    add()."""
    import torch
    data = _cornell()
    sc = api.Scene(data).upload(0)
    sc.refit(data.vertices.copy())  # (the refit's working arrays exist: refit_info's times are those of this refit throughout)
    lo, hi = data.bounds()
    rays = scenes.random_rays(2000, lo, hi, seed=3)
    before = _state(sc, rays)
    acc = api.Accumulator(sc, max_depth=5, seed=11)
    acc.add(1)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    light, ball = first[data.mesh_names.index("light")], first[data.mesh_names.index("ball")]
    bad = []
    v = ball_moved(data)
    v[light + 1, 2, 0] = np.nextafter(v[light + 1, 2, 0], 1.0)
    bad.append(("light", v))
    for what, x in (("nan", np.nan), ("1e19", 1e19)):
        v = ball_moved(data)
        v[ball + 5, 1, 2] = x
        bad.append((what, v))
    for what, v in bad:
        for how in ("host", "device"):
            with pytest.raises(api.PrtError) as e:
                if how == "host":
                    sc.rebuild(v)
                else:
                    d = torch.from_numpy(v).cuda()
                    torch.cuda.synchronize()
                    sc.rebuild_device(d.data_ptr())
            assert e.value.code == _abi.PRT_E_INVALID, (what, how)
            if what == "light":
                assert "prt_scene_update_vertices" in str(e.value)
            _assert_unchanged(sc, rays, before, (what, how))
            acc.add(1)  # the generation was not bumped
    acc.close()
    sc.close()


@pytest.mark.parametrize("how", ["host", "device"])
def test_injected_allocation_failures_change_nothing(dev_lib, monkeypatch, how):
    """PRT_TEST_FAIL_REBUILD=k for every k the call makes: PRT_E_OOM and the same bit-equality; then a rebuild without the
    hook succeeds and the scene is the fresh scene's.  With the fp32 tables resident, so that they are checked as well."""
    data = _cornell()
    v = ball_moved(data)
    sc = api.Scene(data).upload(0)
    sc.refit(data.vertices.copy())
    lo, hi = data.bounds()
    rays = scenes.random_rays(2000, lo, hi, seed=3)
    frame32 = sc.render(precision=F32, **RENDER)
    before = _state(sc, rays)
    acc = api.Accumulator(sc, max_depth=5, seed=11)
    acc.add(1)
    failed = 0
    for k in range(64):
        monkeypatch.setenv("PRT_TEST_FAIL_REBUILD", str(k))
        try:
            rebuild_how(sc, v, how)
        except api.PrtError as e:
            assert e.code == _abi.PRT_E_OOM and "PRT_TEST_FAIL_REBUILD" in str(e), (k, str(e))
            failed += 1
            _assert_unchanged(sc, rays, before, k)
            assert np.array_equal(sc.render(precision=F32, **RENDER), frame32), k
            acc.add(1)
            continue
        finally:
            monkeypatch.delenv("PRT_TEST_FAIL_REBUILD")
        break  # k is past the call's last allocation: this rebuild went through
    else:
        pytest.fail("the rebuild still fails at its 64th allocation")
    print(f"[rebuild] {failed} allocations of a rebuild failed in turn")
    assert failed >= 6  # the boxes, the builder's run, the shading records, the inverse order, parents, counters
    fresh = api.Scene(with_vertices(data, v), device_bvh=True).upload(0)
    compare_images(sc.render(**RENDER), fresh.render(**RENDER), max_bad=0)
    rebuild_how(sc, data.vertices.copy(), how)  # without the hook
    compare_images(sc.render(**RENDER), before[0], max_bad=0)
    for s in (acc, sc, fresh):
        s.close()


# ------------------------------------------------------------------------------------------------ 7
def test_ordering_against_calls_in_flight(dev_lib):
    """render_device on stream A, rebuild_device on stream B, render_device on stream A into a second buffer: the first frame
    is the old geometry's, the second the new geometry's (both against fresh scenes, 1e-9)."""
    import torch
    # 256 x 256 at spp 64 keeps the first render busy for far longer than the rebuild's read-only part takes: the first
    # render is in flight when the rebuild is issued
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
    sc.rebuild_device(d_v.data_ptr(), stream=sb.cuda_stream)
    sc.render_device(f1.data_ptr(), None, stream=sa.cuda_stream, **params)
    torch.cuda.synchronize()
    old, new = api.Scene(data).upload(0), api.Scene(with_vertices(data, v), device_bvh=True).upload(0)
    compare_images(f0.cpu().numpy(), old.render(**params), max_bad=0)
    compare_images(f1.cpu().numpy(), new.render(**params), max_bad=0)
    for s in (sc, old, new):
        s.close()
