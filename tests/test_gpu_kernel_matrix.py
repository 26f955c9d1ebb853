"""The render kernel K3 variant by variant (-m gpu).  k_render<COUNT, FEAT, LLDS, PAD> is one compilation per material
permutation (lean, TEX, PHONG, CT, ALL; + PRT_FEAT_EXTRA for scenes with light tables or plain texel arrays) x shading
tables in LDS or not x packed or padded triangle records: 40 production and 20 counting instantiations per precision, each
with its own registers, LDS and park layout.  A small scene family selects each of them explicitly (the dev-hooks library's
PRT_TUNE_NO_LDS / PRT_TUNE_TRI_STRIDE / PRT_TUNE_TEX_BUDGET), PrtBvhInfo.render_variant says which one ran, and:

  * every fp64 production and counting variant gives the oracle's frame to 1e-9 per pixel, its ray counts, and the other
    variants' frame of the same scene to 1e-12; the tests assert that every reachable variant ran;
  * every fp32 production variant is within the second tolerance tier of the oracle (test_gpu_f32.py);
  * the wave scheduling thresholds (PRT_TUNE_KEEP / CACHED_MIN / LEAF_BATCH / INNER_MIN / SCRAMBLE) decide only WHEN a wave
    refills or tests its parked leaves; a lane's traversal and its random streams do not depend on them, so the frame, the ray
    counts and the counting run's node / triangle work are identical bit for bit under every setting, in both precisions.
"""
import itertools

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from pooraytracer_amd.scenes import Material
from tests.test_gpu_f32 import check_image_tier2, oracle_tier2_reference
from tests.test_gpu_parity import assert_ray_counts, compare_images

pytestmark = pytest.mark.gpu
F64, F32 = _abi.PRECISION_F64, _abi.PRECISION_F32
LLDS, PAD, EXTRA, VALID = _abi.VARIANT_LLDS, _abi.VARIANT_PAD, _abi.VARIANT_EXTRA, _abi.VARIANT_VALID
PERMS = {"lean": 0, "tex": 1, "phong": 2, "ct": 4, "all": 7}   # scene family -> the permutation it selects (PRT_FEAT_*)
LIGHTINGS = ("quad", "sphere")                                 # 2-triangle quad light; emissive icosphere (light tables)
SPP, DEPTH = 8, 8

# Production variants no scene of the family can launch, {variant: reason}.  fp64: size_kernels renders without the LDS
# tables when they would cost the production kernel a resident block, which could make a +llds variant unreachable; on
# gfx950 the occupancy query keeps the tables of every permutation here, so all 40 run.  fp32: the kernels keep their tables
# whatever they cost in occupancy.
UNREACHABLE_F64 = {}
UNREACHABLE_F32 = {}


def matrix_scene(perm, lighting, width=40, height=32):
    """A closed Lambertian box with objects whose materials select permutation `perm`, lit by a quad or an icosphere."""
    b = scenes._Builder(f"matrix-{perm}-{lighting}")
    white = b.material(Material("White", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    red = b.material(Material("Red", _abi.MAT_LAMBERTIAN, kd=(0.63, 0.065, 0.05)))
    green = b.material(Material("Green", _abi.MAT_LAMBERTIAN, kd=(0.14, 0.45, 0.091)))
    light = b.material(Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=(14.0, 13.0, 11.0)))
    b.mesh("floor", white, *scenes.quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)))
    b.mesh("ceiling", white, *scenes.quad((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)))
    b.mesh("back", white, *scenes.quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)))
    b.mesh("left", red, *scenes.quad((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)))
    b.mesh("right", green, *scenes.quad((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)))
    b.mesh("front", white, *scenes.quad((1, -1, 1), (-1, -1, 1), (-1, 1, 1), (1, 1, 1)))
    mats = []
    if perm in ("lean", "all"):
        mats.append(Material("Mirror", _abi.MAT_MIRROR))
    if perm == "lean":
        mats.append(Material("Ball", _abi.MAT_LAMBERTIAN, kd=(0.5, 0.5, 0.8)))
    if perm in ("tex", "all"):
        b.textures.append(scenes._wood_texture(32))
        mats.append(Material("Wood", _abi.MAT_LAMBERTIAN, kd=(0.5, 0.35, 0.2), texture=0))
    if perm in ("phong", "all"):
        mats.append(Material("PhongLo", _abi.MAT_PHONG, kd=(0.5, 0.5, 0.3), ks=(0.3, 0.3, 0.3), ns=5.0))
        mats.append(Material("PhongHi", _abi.MAT_PHONG, kd=(0.2, 0.3, 0.4), ks=(0.5, 0.5, 0.5), ns=60.0))
    if perm in ("ct", "all"):
        mats.append(Material("GoldIso", _abi.MAT_COOKTORRANCE, kd=(0.8, 0.6, 0.2), eta=(0.1, 0.5, 1.5), k=(4.0, 0.02, 0.3),
                             alpha_x=0.3, alpha_y=0.3))
        mats.append(Material("GoldAniso", _abi.MAT_COOKTORRANCE, kd=(0.8, 0.6, 0.2), eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2),
                             alpha_x=0.08, alpha_y=0.5))
    spots = [(-0.55, -0.72, -0.35), (0.5, -0.72, -0.3), (0.0, -0.74, 0.15), (-0.45, -0.2, -0.7), (0.55, -0.15, -0.65),
             (0.05, -0.3, -0.5)]
    for i, m in enumerate(mats):
        v, uv, n = scenes.icosphere(2, radius=0.26, center=spots[i])
        b.mesh(f"ball{i}", b.material(m), v, uv, n)
    if lighting == "quad":
        b.mesh("light", light, *scenes.quad((-0.3, 0.995, -0.3), (0.3, 0.995, -0.3), (0.3, 0.995, 0.3), (-0.3, 0.995, 0.3)))
    else:
        v, uv, n = scenes.icosphere(2, radius=0.16, center=(0.1, 0.35, -0.5))
        b.mesh("light", light, v, uv, n)
    return b.build(scenes.Camera(width, height, 60.0, eye=(0.0173, 0.0091, 0.95), look_at=(0.0, -0.2, 0.0)))


SCENES = [(perm, lighting) for perm in PERMS for lighting in LIGHTINGS]
_DATA = {}


def _data(perm, lighting):
    if (perm, lighting) not in _DATA:
        _DATA[(perm, lighting)] = matrix_scene(perm, lighting)
    return _DATA[(perm, lighting)]


def _seed(perm, lighting):
    return 3 + 2 * list(PERMS).index(perm) + LIGHTINGS.index(lighting)


def variant(sc, precision=F64):
    """The PRT_VARIANT_* byte of the production K3 instantiation `sc` launches in `precision` (0: none chosen yet)."""
    return (sc.bvh_info()["render_variant"] >> (8 * precision)) & 0xFF


def variant_name(v):
    perm = {p: n for n, p in PERMS.items()}[v & _abi.VARIANT_PERM_MASK]
    return perm + "".join(f"+{k}" for k, bit in (("llds", LLDS), ("pad", PAD), ("extra", EXTRA)) if v & bit)


def all_variants():
    return {VALID | p | (LLDS if l else 0) | (PAD if d else 0) | (EXTRA if x else 0)
            for p in PERMS.values() for l, d, x in itertools.product((0, 1), repeat=3)}


def coverage_table(title, ran, unreachable, flags=(LLDS, PAD, EXTRA)):
    cols = [sum(c) for c in itertools.product(*[(0, f) for f in flags])]
    head = ["base" if c == 0 else "+".join(n for n, f in (("llds", LLDS), ("pad", PAD), ("extra", EXTRA)) if c & f) for c in cols]
    lines = [title, f"{'':6}" + "".join(f"{h:>18}" for h in head)]
    for name, p in PERMS.items():
        row = []
        for c in cols:
            v = VALID | p | c
            row.append("ran" if v in ran else "unreachable" if v in unreachable else "MISSING")
        lines.append(f"{name:6}" + "".join(f"{r:>18}" for r in row))
    for v, why in sorted(unreachable.items()):
        lines.append(f"  unreachable {variant_name(v)}: {why}")
    print("\n" + "\n".join(lines))


def _upload(monkeypatch, data, no_lds, stride, tex_budget0=False):
    """Upload `data` from the dev-hooks library with the LDS tables on or off, records at `stride` bytes and, with
    tex_budget0, the textures as plain texel arrays.  The hooks stay set: the fp32 tables are sized on the first fp32 call."""
    monkeypatch.setenv("PRT_TUNE_NO_LDS", str(no_lds))
    monkeypatch.setenv("PRT_TUNE_TRI_STRIDE", str(stride))
    if tex_budget0:
        monkeypatch.setenv("PRT_TUNE_TEX_BUDGET", "0")
    else:
        monkeypatch.delenv("PRT_TUNE_TEX_BUDGET", raising=False)
    return api.Scene(data).upload(0)


def _configs(perm):
    """(no_lds, tex_budget0) of the production runs of a scene of permutation `perm` at one record stride."""
    return [(n, t) for t in ((False, True) if PERMS[perm] & 1 else (False,)) for n in (0, 1)]


def _check_variant(sc, v, perm, lighting, no_lds, stride, tex_budget0, precision):
    info = sc.bvh_info()
    where = (perm, lighting, no_lds, stride, tex_budget0, variant_name(v))
    assert v & VALID and v & _abi.VARIANT_PERM_MASK == PERMS[perm], where
    assert bool(v & PAD) == (stride == 128), where
    assert bool(v & EXTRA) == (lighting == "sphere" or tex_budget0), where
    if no_lds:
        assert not v & LLDS, where
    if precision == F64:  # the fp64 tables PrtBvhInfo reports are the ones the kernel stages
        assert bool(v & LLDS) == bool(info["lds_materials"] or info["lds_light_nodes"] or info["lds_light_tris"]), where
        assert info["tri_stride"] == stride, where
        assert info["texture_layouts"] == (0 if not PERMS[perm] & 1 else 2 if tex_budget0 else 1), where


def _render_counting(sc, **kw):
    import torch
    cam = sc.data.camera
    d = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
    sc.render_device(d.data_ptr(), None, count_work=True, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy(), sc.counters()


def _close(a, b, rel):
    return bool((np.abs(a - b) <= rel * np.maximum(1.0, np.abs(b))).all())


# What the fp64 matrix cases ran (filled by test_fp64_variant_matches_the_oracle, read by test_fp64_variant_coverage), the
# oracle's frames and each scene's first frame (computed once per scene and jitter setting).
_RAN, _RAN_COUNT, _CASES_DONE = set(), set(), set()
_REFS, _FIRST = {}, {}
MATRIX_CASES = [(perm, lighting, stride) for perm, lighting in SCENES for stride in (96, 128)]


@pytest.mark.parametrize("perm,lighting,stride", MATRIX_CASES)
def test_fp64_variant_matches_the_oracle(gpu, dev_lib, monkeypatch, perm, lighting, stride):
    """One scene with packed or padded records x LDS tables on / off (x texel arrays for textured scenes), with and without
    pixel jitter: the reported variant, the oracle's frame to 1e-9 per pixel, its ray counts, the scene's other variants to
    1e-12; the counting instantiation of each to the oracle and to its production frame."""
    data = _data(perm, lighting)
    seed = _seed(perm, lighting)
    for no_lds, tb0 in _configs(perm):
        sc = _upload(monkeypatch, data, no_lds, stride, tb0)
        v = variant(sc)
        assert variant(sc, F32) == 0  # no fp32 tables before the first fp32 call
        _check_variant(sc, v, perm, lighting, no_lds, stride, tb0, F64)
        for j in (False, True):
            kw = dict(spp=SPP, max_depth=DEPTH, seed=seed, pixel_jitter=j)
            where = (perm, lighting, variant_name(v), "jitter" if j else "centre")
            if (perm, lighting, j) not in _REFS:
                _REFS[(perm, lighting, j)] = oracle.Oracle(data).render(nthreads=8, **kw)
            ref, ref_cnt = _REFS[(perm, lighting, j)]
            img = sc.render(**kw)
            cnt = sc.counters()
            assert compare_images(img, ref) == 0, where
            assert_ray_counts(cnt, ref_cnt)
            assert cnt["samples"] == data.camera.width * data.camera.height * SPP
            first = _FIRST.setdefault((perm, lighting, j), img)
            assert _close(img, first, 1e-12), where
            cimg, ccnt = _render_counting(sc, **kw)
            assert compare_images(cimg, ref) == 0, where + ("counting",)
            assert _close(cimg, img, 1e-12), where + ("counting",)
            assert (ccnt["rays_closest"], ccnt["rays_shadow"]) == (cnt["rays_closest"], cnt["rays_shadow"]), where
            assert ccnt["node_fetches"] > 0 and 0 < ccnt["tri_full"] <= ccnt["tri_tests"], where
        sc.close()
        _RAN.add(v)
        _RAN_COUNT.add(v & ~EXTRA)  # the counting kernels: the PRT_FEAT_EXTRA compilation, same tables and records
    _CASES_DONE.add((perm, lighting, stride))


def test_fp64_variant_coverage(gpu):
    """Every fp64 production variant except the listed unreachable ones, and every reachable counting variant, ran in the
    matrix cases above (and passed them)."""
    coverage_table("fp64 production K3 variants:", _RAN, UNREACHABLE_F64)
    coverage_table("fp64 counting K3 variants (all PRT_FEAT_EXTRA):", _RAN_COUNT, {}, flags=(LLDS, PAD))
    assert _CASES_DONE == set(MATRIX_CASES), f"matrix cases that did not pass: {sorted(set(MATRIX_CASES) - _CASES_DONE)}"
    want = all_variants() - set(UNREACHABLE_F64)
    assert _RAN == want, sorted(variant_name(v) for v in _RAN ^ want)
    want_count = {v & ~EXTRA for v in want}
    assert _RAN_COUNT == want_count, sorted(variant_name(v) for v in _RAN_COUNT ^ want_count)


def test_every_fp32_variant_within_tier2_of_the_oracle(gpu, dev_lib, monkeypatch):
    """Every scene x LDS tables on / off x packed / padded records in the fp32 fast mode: the reported fp32 variant and the
    second tolerance tier against the oracle's samples (test_gpu_f32.py's image check).  Then: every reachable variant ran."""
    spp = 32
    ran = set()
    for perm, lighting in SCENES:
        data = _data(perm, lighting)
        seed = _seed(perm, lighting)
        ref, sigma = oracle_tier2_reference(data, spp, max_depth=DEPTH, seed=seed)
        for no_lds, stride in itertools.product((0, 1), (96, 128)):
            sc = _upload(monkeypatch, data, no_lds, stride)
            v64 = variant(sc)
            assert variant(sc, F32) == 0
            img = sc.render(spp=spp, max_depth=DEPTH, seed=seed, precision=F32)
            v = variant(sc, F32)
            _check_variant(sc, v, perm, lighting, no_lds, stride, False, F32)
            assert variant(sc) == v64  # the fp64 byte is untouched by the fp32 tables
            ran.add(v)
            try:
                check_image_tier2(img, ref, sigma, spp)
            except AssertionError as e:
                raise AssertionError(f"{perm}/{lighting} {variant_name(v)}: {e}") from None
            assert sc.counters()["samples"] == data.camera.width * data.camera.height * spp
            sc.close()
    coverage_table("fp32 production K3 variants:", ran, UNREACHABLE_F32)
    want = all_variants() - set(UNREACHABLE_F32)
    assert ran == want, sorted(variant_name(v) for v in ran ^ want)


@pytest.mark.parametrize("perm,lighting", [("ct", "quad"), ("all", "sphere"), ("lean", "sphere")])
def test_render_samples_of_more_variants_match_the_oracle_per_sample(gpu, perm, lighting):
    """prt_render_samples (the production and the counting instantiation of K3, one sample per item) on a CookTorrance
    scene and on icosphere-lit scenes (light tables): per sample the oracle's radiance to 1e-9 and its path signature."""
    data = _data(perm, lighting)
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    assert variant(sc) & EXTRA == (EXTRA if lighting == "sphere" else 0)
    rng = np.random.default_rng(5)
    px = np.stack([rng.integers(0, cam.width, 240), rng.integers(0, cam.height, 240)], axis=1)
    kw = dict(spp=12, max_depth=DEPTH, seed=_seed(perm, lighting))
    g, gt = sc.render_samples(px, trace=True, **kw)
    gp = sc.render_samples(px, **kw)
    assert _close(g, gp, 1e-12)
    o, ot = oracle.Oracle(data).render_samples(px, trace=True, **kw)
    same = (gt == ot).all(-1)
    assert same.all(), int((~same).sum())
    assert (np.abs(g - o) / np.maximum(1.0, np.abs(o))).max() <= 1e-9
    assert gt[..., 0].max() > 3


# ------------------------------------------------------------------------------------------ schedule invariance
# The clamped ranges of the hooks (render_impl): nothing outside them may reach a GPU run — an unclamped build would hang.
SCHEDULE_RANGES = {"KEEP": (0, 64), "CACHED_MIN": (1, 65), "LEAF_BATCH": (1, 64), "INNER_MIN": (0, 64), "SCRAMBLE": (0, 1)}
SCHEDULES = ([{"KEEP": v} for v in (0, 1, 24, 63, 64)] + [{"CACHED_MIN": v} for v in (1, 8, 64, 65)]
             + [{"LEAF_BATCH": v} for v in (1, 2, 48, 64)] + [{"INNER_MIN": v} for v in (0, 12, 64)]
             + [{"SCRAMBLE": v} for v in (0, 1)]
             + [dict(KEEP=0, CACHED_MIN=1, LEAF_BATCH=1, INNER_MIN=0),
                dict(KEEP=64, CACHED_MIN=65, LEAF_BATCH=64, INNER_MIN=64, SCRAMBLE=1),
                dict(KEEP=1, CACHED_MIN=65, LEAF_BATCH=64, INNER_MIN=0),
                dict(KEEP=63, CACHED_MIN=8, LEAF_BATCH=2, INNER_MIN=64, SCRAMBLE=1)])


def _set_schedule(monkeypatch, setting):
    for k in SCHEDULE_RANGES:
        monkeypatch.delenv(f"PRT_TUNE_{k}", raising=False)
    for k, v in setting.items():
        lo, hi = SCHEDULE_RANGES[k]
        assert lo <= v <= hi, (k, v)
        monkeypatch.setenv(f"PRT_TUNE_{k}", str(v))


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("perm,lighting", SCENES)
def test_frames_are_schedule_invariant(gpu, dev_lib, monkeypatch, perm, lighting, precision):
    """One variant per permutation and lighting, the scheduling thresholds swept one at a time over their clamped ranges and
    at a few corners: the frame (bit for bit), the samples and ray counts, and in a counting run the node fetches and the
    triangle tests, are those of the default schedule; a progressive pass (the accumulate path) and adaptive rounds (the
    list-item path) likewise.  The counting runs' inner / leaf rounds show that the hooks took effect."""
    data = _data(perm, lighting)
    _set_schedule(monkeypatch, {})
    sc = api.Scene(data).upload(gpu)
    kw = dict(spp=SPP, max_depth=DEPTH, seed=_seed(perm, lighting), precision=precision)
    ray_keys = ("samples", "rays_closest", "rays_shadow")
    work_keys = ray_keys + ("node_fetches", "tri_tests", "tri_full")

    def run():
        img = sc.render(**kw)
        cnt = sc.counters()
        cimg, ccnt = _render_counting(sc, **kw)
        with api.Accumulator(sc, max_depth=DEPTH, seed=kw["seed"], precision=precision) as acc:
            acc.add(3)
            acc.add(5)
            prog = acc.image()
        with api.AdaptiveAccumulator(sc, rel_tol=0.05, abs_tol=1e-3, min_spp=8, max_spp=64, batch=4, max_depth=DEPTH,
                                     seed=kw["seed"], precision=precision) as ad:
            ad.step(8)
            ad.step(8)
            adapt = ad.export()
        return img, cnt, cimg, ccnt, prog, adapt

    base = run()
    img0, cnt0, cimg0, ccnt0, prog0, adapt0 = base
    assert variant(sc, precision) & VALID
    assert cnt0["rays_closest"] > 0 and ccnt0["node_fetches"] > 0
    assert 0 < adapt0["counts"].min() and adapt0["counts"].max() == 16
    rounds = {(ccnt0["inner_rounds"], ccnt0["leaf_rounds"])}
    for setting in SCHEDULES:
        _set_schedule(monkeypatch, setting)
        img, cnt, cimg, ccnt, prog, adapt = run()
        _set_schedule(monkeypatch, {})
        where = (perm, lighting, variant_name(variant(sc, precision)), setting)
        assert np.array_equal(img.view(np.uint64), img0.view(np.uint64)), where
        assert [cnt[k] for k in ray_keys] == [cnt0[k] for k in ray_keys], where
        assert np.array_equal(cimg.view(np.uint64), cimg0.view(np.uint64)), where
        assert [ccnt[k] for k in work_keys] == [ccnt0[k] for k in work_keys], where
        assert np.array_equal(prog.view(np.uint64), prog0.view(np.uint64)), where + ("progressive",)
        for k in ("sums", "moments", "counts"):
            assert np.array_equal(adapt[k], adapt0[k]) and adapt[k].tobytes() == adapt0[k].tobytes(), where + ("adaptive", k)
        rounds.add((ccnt["inner_rounds"], ccnt["leaf_rounds"]))
    assert len(rounds) > 1, rounds
    sc.close()
