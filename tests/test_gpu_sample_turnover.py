"""K3's sample turnover (-m gpu).  In the one-pass permutations (lean, CookTorrance; not fp32 lean) a lane walks a pass in path order: a
returned shadow ray that ends its sample and a traced ray that left the scene are settled at the top of the pass, the next
sample of the item starts at once from the parked camera hit, and the shading blocks consume that hit in the same pass.  Only
the order of blocks inside a pass changed — draws, expressions and the order of terms into an item's sum did not:

  * frames and ray counters are those of the commit before the reorder, bit for bit (tests/golden/sample_turnover_parent.npz:
    the 40 x 32 lean and CookTorrance matrix scenes, quad light, fp64 and fp32, spp 1 / 2 / 7, depth 6, rendered on an MI355X
    by commit e1bdde2, "Shade a K3 path vertex in one pass and chain its rays in the wave loop"; the "_items" entries are the
    spp 7 frames dealt as one work item per pixel, sample_chunks=1 — a frame this small is otherwise dealt sample by sample
    and no sample would turn over inside an item).
    The CookTorrance entries were rendered again when ct_sample_wm stopped forming sqrt(1 - p.x^2) and pz by cancellation
    (tests/test_gpu_device_math.py holds its error below 1e-11): same ray counters, the same draws and paths, and of the
    3,840 values per frame 227 .. 435 moved by at most 2.3e-14 relative in fp64, 391 .. 1,330 by at most 2.6e-5 in fp32
    (rounding of the new expressions); the lean entries are still e1bdde2's, bit for bit.
    The fp32 lean kernels keep the old order of the pass (with the new one the compiler contracts their Scatter arithmetic
    differently and 133 / 228 / 539 of the 3,840 values left the fixture by up to 5.4e-7 relative), so
    for them this is a regression check of an unchanged kernel;
  * per sample, radiance and path signature are the oracle's for every way a sample can end, in a closed and in an open box,
    and the test shows on the oracle's own traces that each way occurs; whole frames of the same scenes (items of several
    samples: the turnover inside an item) are the oracle's to 1e-9;
  * KEEP / CHAIN_MIN / CACHED_MIN are schedule only, in the open box as well;
  * the flows the reorder does not serve (pixel jitter, no light sampling, no lights, items that end mid-pixel, a tile
    share) give the oracle's frame.
"""
import dataclasses
import os

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, distributed, scenes
from tests.test_gpu_kernel_matrix import DEPTH, F32, F64, VALID, _data, _render_counting, _seed, matrix_scene, variant, variant_name
from tests.test_gpu_parity import compare_images

pytestmark = pytest.mark.gpu
NEE, VISIBLE, ROULETTE, SCATTER = _abi.TRACE_NEE, _abi.TRACE_VISIBLE, _abi.TRACE_ROULETTE, _abi.TRACE_SCATTER
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_turnover_parent.npz")
BACKGROUND = (0.3, 0.4, 0.5)
# the matrix scenes' eye, looking up: the quad light under the ceiling is in view
UP_CAMERA = scenes.Camera(40, 32, 60.0, eye=(0.0173, 0.0091, 0.95), look_at=(0.0, 0.9, -0.2))


def _without(data, *names):
    """`data` without the meshes called `names`."""
    keep = [i for i, n in enumerate(data.mesh_names) if n not in names]
    first = data.mesh_first_tri.astype(np.int64)
    tris = np.concatenate([np.arange(first[i], first[i + 1]) for i in keep])
    sizes = [int(first[i + 1] - first[i]) for i in keep]
    return dataclasses.replace(data, name=data.name + "-without-" + "-".join(names), vertices=data.vertices[tris],
                               texcoords=data.texcoords[tris], normals=data.normals[tris],
                               mesh_first_tri=np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64),
                               mesh_material=data.mesh_material[keep], mesh_names=[data.mesh_names[i] for i in keep])


_OPEN = {}


def open_scene(perm):
    """The matrix scene without its right wall: camera rays and bounces leave the box through it."""
    if perm not in _OPEN:
        _OPEN[perm] = _without(matrix_scene(perm, "quad"), "right")
    return _OPEN[perm]


def _bounded_ray_counts(gpu_cnt, cpu_cnt):
    """The GPU traces no ray the oracle does not.  (No lower bound as in test_gpu_parity.assert_ray_counts: the camera ray of
    an item of several samples is traced once, the oracle counts it per sample, and in the open box many samples are only
    that ray.)"""
    assert 0 < gpu_cnt["rays_closest"] <= cpu_cnt["rays_closest"]
    assert gpu_cnt["rays_shadow"] <= cpu_cnt["rays_shadow"]


# ------------------------------------------------------------------------------------------ 1. the parent's frames
@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_frames_and_ray_counts_are_the_parents(gpu, perm, precision):
    g = np.load(GOLDEN)
    sc = api.Scene(_data(perm, "quad")).upload(gpu)
    # (a frame this small is dealt one sample per work item; "items": the fixture's spp 7 frames dealt one item per pixel)
    for spp, chunks in ((1, 0), (2, 0), (7, 0), (7, 1)):
        img = sc.render(spp=spp, max_depth=6, seed=_seed(perm, "quad"), precision=precision, sample_chunks=chunks)
        cnt = sc.counters()
        key = f"{perm}_{'f64' if precision == F64 else 'f32'}_spp{spp}" + ("_items" if chunks else "")
        assert np.array_equal(np.ascontiguousarray(img).view(np.uint64), g[key + "_bits"]), key
        assert [cnt["rays_closest"], cnt["rays_shadow"], cnt["samples"]] == [int(x) for x in g[key + "_counters"]], key
    assert variant(sc, precision) & VALID
    sc.close()


# ------------------------------------------------------------------------------------------ 2. every way a sample can end
# Runs chosen on the CPU with the oracle so that every kind below occurs (the test re-derives that from the oracle's traces
# and fails if one is missing).  prt_render_samples makes one work item per sample, so each of them is also the last sample
# of its item; the frames of test_open_box_frames_match_the_oracle cover the turnover inside an item.
KINDS = ("shadow_last_occluded", "shadow_last_visible", "bounce_miss", "camera_miss", "emitter_seen_by_camera",
         "emitter_over_mirror", "roulette_fails_without_light_sample", "depth_exhausted_shadow_pending",
         "camera_vertex_ends_sample")
SAMPLE_RUNS = [dict(max_depth=DEPTH, spp=6), dict(max_depth=1, spp=4), dict(max_depth=2, spp=4), dict(max_depth=DEPTH, spp=2, camera=UP_CAMERA)]
WANT = {("lean", "closed"): set(KINDS) - {"bounce_miss", "camera_miss"}, ("lean", "open"): set(KINDS),
        ("ct", "closed"): set(KINDS) - {"bounce_miss", "camera_miss", "emitter_over_mirror"},
        ("ct", "open"): set(KINDS) - {"emitter_over_mirror"}}  # (the CookTorrance scene has no mirror)
MIRROR_PIXELS = [(15, 9), (6, 10), (16, 10), (3, 19), (33, 26)]  # lean scene, its seed: a mirror bounce ends on the light


def _pixels(data):
    """A fixed 12 x 10 lattice over the 40 x 32 image (walls, floor, ceiling, every ball, the light, the opening) and the
    pixels above."""
    cam = data.camera
    xs = np.linspace(1, cam.width - 2, 12).astype(int)
    ys = np.linspace(0, cam.height - 1, 10).astype(int)
    return np.array([(x, y) for y in ys for x in xs] + MIRROR_PIXELS, dtype=np.int32)


def sample_endings(data, traces, max_depth):
    """Which of KINDS end the samples whose path signatures are `traces` (n_pixels, count, TRACE_WORDS), runs at `max_depth`."""
    tri_mesh = np.searchsorted(data.mesh_first_tri.astype(np.int64), np.arange(data.n_tris), side="right") - 1
    mat_type = np.array([m.type for m in data.materials])[data.mesh_material[tri_mesh]]
    found = set()
    for t in traces.reshape(-1, traces.shape[-1]):
        n = int(t[0])
        assert 1 <= n <= _abi.TRACE_VERTS
        v = n - 1  # the vertex that ended the sample
        prim, fl = int(t[1 + 2 * v]), int(t[2 + 2 * v])
        if prim < 0:
            kind = "camera_miss" if v == 0 else "bounce_miss"
        elif mat_type[prim] == _abi.MAT_DIFFUSE_LIGHT:
            kind = "emitter_seen_by_camera" if v == 0 else None
            if v > 0 and mat_type[int(t[1 + 2 * (v - 1)])] == _abi.MAT_MIRROR:
                kind = "emitter_over_mirror"
        elif fl & NEE:
            kind = "shadow_last_visible" if fl & VISIBLE else "shadow_last_occluded"
            if fl & ROULETTE and fl & SCATTER and v == max_depth:
                found.add("depth_exhausted_shadow_pending")
        else:
            kind = None if fl & ROULETTE else "roulette_fails_without_light_sample"
        if kind:
            found.add(kind)
        if v == 0 and (prim < 0 or not fl & NEE):
            found.add("camera_vertex_ends_sample")  # without a shadow ray: the fresh sample ends inside the shading blocks
    return found


@pytest.mark.parametrize("box", ["closed", "open"])
@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_every_sample_ending_matches_the_oracle_per_sample(gpu, perm, box):
    data = _data(perm, "quad") if box == "closed" else open_scene(perm)
    px = _pixels(data)
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    found = set()
    for run in SAMPLE_RUNS:
        kw = dict(seed=_seed(perm, "quad"), background=BACKGROUND, **run)
        o, ot = orc.render_samples(px, trace=True, **kw)
        found |= sample_endings(data, ot, run["max_depth"])
        g, gt = sc.render_samples(px, trace=True, **kw)
        gp = sc.render_samples(px, **kw)  # the production instantiation
        same = (gt == ot).all(-1)
        assert same.all(), (run, int((~same).sum()))
        assert (np.abs(g - o) / np.maximum(1.0, np.abs(o))).max() <= 1e-9, run
        assert (np.abs(gp - o) / np.maximum(1.0, np.abs(o))).max() <= 1e-9, run
    sc.close()
    assert found >= WANT[(perm, box)], sorted(WANT[(perm, box)] - found)


@pytest.mark.parametrize("perm", ["lean", "ct"])
def test_open_box_frames_match_the_oracle(gpu, perm):
    """Items of one and of several samples (spp 1: every sample the last of its item; spp 5: the turnover inside an item) in
    the open box, non-zero background: the oracle's frame to 1e-9 and its ray counts."""
    data = open_scene(perm)
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    for spp, cam in ((1, None), (5, None), (5, UP_CAMERA)):  # (UP_CAMERA: items whose every sample ends at the camera vertex)
        kw = dict(spp=spp, max_depth=DEPTH, seed=_seed(perm, "quad"), background=BACKGROUND, camera=cam)
        ref, ref_cnt = orc.render(nthreads=8, **kw)
        img = sc.render(sample_chunks=1, **kw)  # one item per pixel (a frame this small is dealt sample by sample otherwise)
        assert compare_images(img, ref) == 0, (perm, spp, cam is not None)
        _bounded_ray_counts(sc.counters(), ref_cnt)
    sc.close()


# ------------------------------------------------------------------------------------------ 3. schedule only
HOOKS = ("KEEP", "CHAIN_MIN", "CACHED_MIN")
SETTINGS = ([{"KEEP": k} for k in (0, 63)] + [{"CHAIN_MIN": c} for c in (1, 65)] + [{"CACHED_MIN": m} for m in (1, 65)]
            + [{"KEEP": k, "CHAIN_MIN": c, "CACHED_MIN": m} for k in (0, 63) for c in (1, 65) for m in (1, 65)])


def _set(monkeypatch, setting):
    for k in HOOKS:
        monkeypatch.delenv(f"PRT_TUNE_{k}", raising=False)
    for k, v in setting.items():
        monkeypatch.setenv(f"PRT_TUNE_{k}", str(v))


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("perm,box", [("lean", "closed"), ("lean", "open"), ("ct", "closed"), ("ct", "open")])
def test_thresholds_are_schedule_only(gpu, dev_lib, monkeypatch, perm, box, precision):
    """PRT_TUNE_KEEP 0 / 63, CHAIN_MIN 1 / 65 and CACHED_MIN 1 / 65, alone and combined: the frame, samples and ray counts, the
    counting run's frame and node / triangle work, one Accumulator pass and two AdaptiveAccumulator steps are those of the
    default setting bit for bit, while the counting runs' refills differ: the hooks act."""
    data = _data(perm, "quad") if box == "closed" else open_scene(perm)
    _set(monkeypatch, {})
    sc = api.Scene(data).upload(gpu)
    kw = dict(spp=5, max_depth=DEPTH, seed=_seed(perm, "quad"), precision=precision, background=BACKGROUND)
    ray_keys = ("samples", "rays_closest", "rays_shadow")
    work_keys = ray_keys + ("node_fetches", "tri_tests", "tri_full")

    def run():
        # one item per pixel: its samples turn over inside the item (a frame this small is dealt sample by sample otherwise)
        img = sc.render(sample_chunks=1, **kw)
        cnt = sc.counters()
        cimg, ccnt = _render_counting(sc, sample_chunks=1, **kw)
        with api.Accumulator(sc, max_depth=DEPTH, seed=kw["seed"], precision=precision, background=BACKGROUND) as acc:
            acc.add(5)
            prog = acc.image()
        with api.AdaptiveAccumulator(sc, rel_tol=0.05, abs_tol=1e-3, min_spp=8, max_spp=64, batch=4, max_depth=DEPTH,
                                     seed=kw["seed"], precision=precision, background=BACKGROUND) as ad:
            ad.step(8)
            ad.step(8)
            adapt = ad.export()
        return img, cnt, cimg, ccnt, prog, adapt

    img0, cnt0, cimg0, ccnt0, prog0, adapt0 = run()
    assert variant(sc, precision) & VALID
    assert cnt0["rays_closest"] > 0 and cnt0["rays_shadow"] > 0 and ccnt0["node_fetches"] > 0
    refills = {(): ccnt0["refills"]}
    for setting in SETTINGS:
        _set(monkeypatch, setting)
        img, cnt, cimg, ccnt, prog, adapt = run()
        _set(monkeypatch, {})
        where = (perm, box, variant_name(variant(sc, precision)), setting)
        assert np.array_equal(img.view(np.uint64), img0.view(np.uint64)), where
        assert [cnt[k] for k in ray_keys] == [cnt0[k] for k in ray_keys], where
        assert np.array_equal(cimg.view(np.uint64), cimg0.view(np.uint64)), where
        assert [ccnt[k] for k in work_keys] == [ccnt0[k] for k in work_keys], where
        assert np.array_equal(prog.view(np.uint64), prog0.view(np.uint64)), where + ("progressive",)
        for k in ("sums", "moments", "counts"):
            assert np.array_equal(adapt[k], adapt0[k]) and adapt[k].tobytes() == adapt0[k].tobytes(), where + ("adaptive", k)
        refills[tuple(sorted(setting.items()))] = ccnt["refills"]
    print(f"\n{perm}/{box} precision {precision}: refills per setting: {refills}")
    for hook, lo, hi in (("KEEP", 0, 63), ("CHAIN_MIN", 1, 65), ("CACHED_MIN", 1, 65)):
        assert refills[((hook, lo),)] != refills[((hook, hi),)], (hook, refills)
    sc.close()


# ------------------------------------------------------------------------------------------ 4. the flows beside the new one
BYPASS = {"pixel_jitter": dict(pixel_jitter=True), "sample_lights_off": dict(sample_lights=False), "no_light_mesh": {},
          "item_ends_mid_pixel": dict(spp=70), "tile_share": dict(rank=1, nranks=3, tile_size=8)}


@pytest.mark.parametrize("perm", ["lean", "ct"])
@pytest.mark.parametrize("case", list(BYPASS))
def test_bypassing_flows_match_the_oracle(gpu, case, perm):
    """Jittered camera rays (every sample traces its own), light sampling off and a scene without lights (no shadow ray ever
    returns), spp above the chunk cap (a pixel is several items) and a third of the tiles: the oracle's frame to 1e-9."""
    data = open_scene(perm)
    chunks = {} if case == "item_ends_mid_pixel" else dict(sample_chunks=1)  # one item per pixel, or the launch's own chunks
    if case == "no_light_mesh":
        data = _without(data, "light")
    kw = dict(spp=4, max_depth=DEPTH, seed=_seed(perm, "quad"), background=BACKGROUND)
    kw.update(BYPASS[case])
    share = {k: kw.pop(k) for k in ("rank", "nranks", "tile_size") if k in kw}
    sc = api.Scene(data).upload(gpu)
    ref, ref_cnt = oracle.Oracle(data).render(nthreads=8, **kw)
    img = sc.render(**kw, **share, **chunks)
    cnt = sc.counters()
    if share:
        cam = data.camera
        own = distributed.owned_mask(cam.width, cam.height, share["tile_size"], share["rank"], share["nranks"])
        assert 0 < own.sum() < own.size and not img[~own].any()
        assert compare_images(img[own][None], ref[own][None]) == 0, (case, perm)
        assert cnt["samples"] == int(own.sum()) * kw["spp"]
    else:
        assert compare_images(img, ref) == 0, (case, perm)
        _bounded_ray_counts(cnt, ref_cnt)
        assert cnt["samples"] == data.camera.width * data.camera.height * kw["spp"]
    if case in ("sample_lights_off", "no_light_mesh"):
        assert cnt["rays_shadow"] == 0
    sc.close()
