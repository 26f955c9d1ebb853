"""K3's one-pass vertex (-m gpu).  In the lean and the CookTorrance permutation the pass that consumes a closest hit shades the whole
path vertex — light pick, the light's contribution as if visible (kept as a pending term), roulette, Scatter (the direction
kept aside) — and a lane whose shadow ray has returned is chained onto its continuation ray inside the wave's traversal loop
once PRT_TUNE_CHAIN_MIN lanes wait for it, or by the next pass (65: always by the next pass).  Draws, operations and their
order are those of the two-pass flow, which the Phong and the textured permutations keep:

  * the chain threshold is schedule only: frames, ray counts, counted work, progressive and adaptive results are identical
    bit for bit under every setting, alone and combined with the other thresholds, in both precisions;
  * per sample, radiance and path signature are the oracle's for every way a vertex can end, and the test shows on the
    oracle's own traces that each way occurs among its samples;
  * scenes without lights, and with light sampling off, keep the flow that scatters in the same pass.
"""
import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api
from tests.test_gpu_kernel_matrix import (DEPTH, F32, F64, SPP, VALID, _data, _render_counting, _seed, matrix_scene, variant,
                                          variant_name)
from tests.test_gpu_parity import assert_ray_counts, compare_images

pytestmark = pytest.mark.gpu
NEE, VISIBLE, ROULETTE, SCATTER = _abi.TRACE_NEE, _abi.TRACE_VISIBLE, _abi.TRACE_ROULETTE, _abi.TRACE_SCATTER

# ------------------------------------------------------------------------------------------ 1. schedule only
CHAIN_SCENES = [("lean", "quad"), ("lean", "sphere"), ("ct", "quad"), ("tex", "quad"), ("phong", "quad")]
TWO_PASS = ("phong", "tex")  # Phong: its Eval draws; textured: measured slower with the one-pass vertex, so it keeps two
HOOKS = ("CHAIN_MIN", "KEEP", "CACHED_MIN")
CHAIN_SETTINGS = ([{"CHAIN_MIN": c} for c in (1, 8, 64, 65)]
                  + [{"CHAIN_MIN": c, "KEEP": k, "CACHED_MIN": m} for c in (1, 8, 64, 65) for k, m in ((0, 1), (63, 65), (0, 65), (63, 1))])


def _set(monkeypatch, setting):
    for k in HOOKS:
        monkeypatch.delenv(f"PRT_TUNE_{k}", raising=False)
    for k, v in setting.items():
        assert k in HOOKS and {"CHAIN_MIN": 1 <= v <= 65, "KEEP": 0 <= v <= 64, "CACHED_MIN": 1 <= v <= 65}[k], (k, v)
        monkeypatch.setenv(f"PRT_TUNE_{k}", str(v))


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("perm,lighting", CHAIN_SCENES)
def test_chain_threshold_is_schedule_only(gpu, dev_lib, monkeypatch, perm, lighting, precision):
    """PRT_TUNE_CHAIN_MIN 1 / 8 / 64 / 65, alone and with KEEP 0 / 63 and CACHED_MIN 1 / 65: the frame, samples and ray
    counts, the counting run's frame and node / triangle work, one Accumulator pass and two AdaptiveAccumulator steps are
    those of the default setting bit for bit.  The counting runs' rounds and refills differ between settings: the hook acts
    (on the Phong and the textured scene through KEEP / CACHED_MIN only — the two-pass flow has nothing to chain)."""
    data = _data(perm, lighting)
    _set(monkeypatch, {})
    sc = api.Scene(data).upload(gpu)
    kw = dict(spp=SPP, max_depth=DEPTH, seed=_seed(perm, lighting), precision=precision)
    ray_keys = ("samples", "rays_closest", "rays_shadow")
    work_keys = ray_keys + ("node_fetches", "tri_tests", "tri_full")

    def run():
        img = sc.render(**kw)
        cnt = sc.counters()
        cimg, ccnt = _render_counting(sc, **kw)
        with api.Accumulator(sc, max_depth=DEPTH, seed=kw["seed"], precision=precision) as acc:
            acc.add(5)
            prog = acc.image()
        with api.AdaptiveAccumulator(sc, rel_tol=0.05, abs_tol=1e-3, min_spp=8, max_spp=64, batch=4, max_depth=DEPTH,
                                     seed=kw["seed"], precision=precision) as ad:
            ad.step(8)
            ad.step(8)
            adapt = ad.export()
        return img, cnt, cimg, ccnt, prog, adapt

    img0, cnt0, cimg0, ccnt0, prog0, adapt0 = run()
    assert variant(sc, precision) & VALID
    assert cnt0["rays_closest"] > 0 and cnt0["rays_shadow"] > 0 and ccnt0["node_fetches"] > 0
    sched = {(): (ccnt0["inner_rounds"], ccnt0["refills"])}
    for setting in CHAIN_SETTINGS:
        _set(monkeypatch, setting)
        img, cnt, cimg, ccnt, prog, adapt = run()
        _set(monkeypatch, {})
        where = (perm, lighting, variant_name(variant(sc, precision)), setting)
        assert np.array_equal(img.view(np.uint64), img0.view(np.uint64)), where
        assert [cnt[k] for k in ray_keys] == [cnt0[k] for k in ray_keys], where
        assert np.array_equal(cimg.view(np.uint64), cimg0.view(np.uint64)), where
        assert [ccnt[k] for k in work_keys] == [ccnt0[k] for k in work_keys], where
        assert np.array_equal(prog.view(np.uint64), prog0.view(np.uint64)), where + ("progressive",)
        for k in ("sums", "moments", "counts"):
            assert np.array_equal(adapt[k], adapt0[k]) and adapt[k].tobytes() == adapt0[k].tobytes(), where + ("adaptive", k)
        sched[tuple(sorted(setting.items()))] = (ccnt["inner_rounds"], ccnt["refills"])
    print(f"\n{perm}/{lighting} precision {precision}: (inner rounds, refills) per setting: {sched}")
    assert len(set(sched.values())) > 1, sched
    alone = {sched[(("CHAIN_MIN", c),)] for c in (1, 8, 64, 65)}
    if perm in TWO_PASS:  # the two-pass flow: the chain threshold has nothing to act on
        assert len(alone) == 1, alone
    else:
        assert len(alone) > 1, alone
    sc.close()


# ------------------------------------------------------------------------------------------ 2. every way a vertex can end
# Pixels and seeds chosen on the CPU with the oracle so that every kind below occurs (the test re-derives that from the
# oracle's traces and fails if one is missing).  Depth 1 and 2 exhaust the depth at vertices that have a pending shadow ray.
SAMPLE_RUNS = {"lean": [dict(max_depth=DEPTH, spp=6), dict(max_depth=1, spp=4), dict(max_depth=2, spp=4)],
               "ct": [dict(max_depth=DEPTH, spp=6), dict(max_depth=1, spp=4), dict(max_depth=2, spp=4)]}
KINDS = ("nee_occluded", "nee_visible_roulette_ends", "nee_visible_continues", "nee_refused", "depth_exhausted_pending",
         "mirror_then_emitter")
WANT = {"lean": set(KINDS), "ct": set(KINDS) - {"mirror_then_emitter"}}  # (the CookTorrance scene has no mirror)


MIRROR_PIXELS = [(15, 9), (6, 10), (16, 10), (3, 19), (33, 26)]  # lean scene, its seed, depth 8: a mirror bounce ends on the light


def _pixels(data):
    """A fixed 12 x 10 lattice over the 40 x 32 image (walls, floor, every ball, the light and its penumbra) and the pixels
    above."""
    cam = data.camera
    xs = np.linspace(1, cam.width - 2, 12).astype(int)
    ys = np.linspace(1, cam.height - 2, 10).astype(int)
    return np.array([(x, y) for y in ys for x in xs] + MIRROR_PIXELS, dtype=np.int32)


def vertex_kinds(data, traces, max_depth):
    """Which of KINDS occur in the path signatures `traces` (n_pixels, count, TRACE_WORDS) of runs at `max_depth`."""
    tri_mesh = np.searchsorted(data.mesh_first_tri.astype(np.int64), np.arange(data.n_tris), side="right") - 1
    mat_type = np.array([m.type for m in data.materials])[data.mesh_material[tri_mesh]]
    found = set()
    for t in traces.reshape(-1, traces.shape[-1]):
        n = int(t[0])
        for v in range(min(n, _abi.TRACE_VERTS)):
            prim, fl = int(t[1 + 2 * v]), int(t[2 + 2 * v])
            if prim < 0:
                continue
            ty = mat_type[prim]
            nxt = int(t[1 + 2 * (v + 1)]) if v + 1 < min(n, _abi.TRACE_VERTS) else None
            if fl & NEE:
                if not fl & VISIBLE:
                    found.add("nee_occluded")
                elif not fl & ROULETTE:
                    found.add("nee_visible_roulette_ends")
                elif fl & SCATTER and nxt is not None:
                    found.add("nee_visible_continues")
                if fl & ROULETTE and fl & SCATTER and v == max_depth:
                    assert nxt is None
                    found.add("depth_exhausted_pending")
            elif ty == _abi.MAT_MIRROR:
                if fl & SCATTER and nxt is not None and nxt >= 0 and mat_type[nxt] == _abi.MAT_DIFFUSE_LIGHT:
                    found.add("mirror_then_emitter")
            elif ty != _abi.MAT_DIFFUSE_LIGHT:
                found.add("nee_refused")  # a lit, light-sampling material and no shadow ray: the geometric test said no
    return found


@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_every_vertex_ending_matches_the_oracle_per_sample(gpu, perm):
    data = _data(perm, "quad")
    px = _pixels(data)
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    found = set()
    for run in SAMPLE_RUNS[perm]:
        kw = dict(seed=_seed(perm, "quad"), **run)
        o, ot = orc.render_samples(px, trace=True, **kw)
        found |= vertex_kinds(data, ot, run["max_depth"])
        g, gt = sc.render_samples(px, trace=True, **kw)
        gp = sc.render_samples(px, **kw)  # the production instantiation
        same = (gt == ot).all(-1)
        assert same.all(), (run, int((~same).sum()))
        assert (np.abs(g - o) / np.maximum(1.0, np.abs(o))).max() <= 1e-9, run
        assert (np.abs(gp - o) / np.maximum(1.0, np.abs(o))).max() <= 1e-9, run
    sc.close()
    assert found == WANT[perm], sorted(WANT[perm] - found)


# ------------------------------------------------------------------------------------------ 3. no lights, lights off
def _without_light(data):
    import dataclasses
    keep = [i for i, n in enumerate(data.mesh_names) if n != "light"]
    first = data.mesh_first_tri.astype(np.int64)
    tris = np.concatenate([np.arange(first[i], first[i + 1]) for i in keep])
    sizes = [int(first[i + 1] - first[i]) for i in keep]
    return dataclasses.replace(data, name=data.name + "-dark", vertices=data.vertices[tris], texcoords=data.texcoords[tris],
                               normals=data.normals[tris], mesh_first_tri=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64),
                               mesh_material=data.mesh_material[keep], mesh_names=[data.mesh_names[i] for i in keep])


@pytest.mark.parametrize("case", ["no_light_mesh", "sample_lights_off"])
def test_vertices_without_a_shadow_ray_keep_their_flow(gpu, case):
    """No vertex takes a shadow ray: the frame is the oracle's to 1e-9, no shadow ray is counted, and the closest-hit rays
    are the oracle's (exactly, where both trace one camera ray per sample and the oracle does not peek: jitter, lights off)."""
    data = matrix_scene("lean", "quad")
    kw = dict(spp=SPP, max_depth=DEPTH, seed=_seed("lean", "quad"), background=(0.3, 0.4, 0.5))
    if case == "no_light_mesh":
        data = _without_light(data)
    else:
        kw["sample_lights"] = False
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    for jitter in (False, True):
        ref, ref_cnt = orc.render(nthreads=8, pixel_jitter=jitter, **kw)
        img = sc.render(pixel_jitter=jitter, **kw)
        cnt = sc.counters()
        assert compare_images(img, ref) == 0, (case, jitter)
        assert cnt["rays_shadow"] == 0 == ref_cnt["rays_shadow"], (case, jitter)
        assert_ray_counts(cnt, ref_cnt)
        if jitter and case == "sample_lights_off":
            assert cnt["rays_closest"] == ref_cnt["rays_closest"], (case, cnt, ref_cnt)
        cimg, ccnt = _render_counting(sc, pixel_jitter=jitter, **kw)
        assert np.array_equal(cimg, img), (case, jitter)
        assert (ccnt["rays_closest"], ccnt["rays_shadow"]) == (cnt["rays_closest"], cnt["rays_shadow"])
    sc.close()
