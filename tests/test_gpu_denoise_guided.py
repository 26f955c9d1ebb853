"""GPU tests of the variance AOV and the variance-guided a-trous filter (prt_accum_variance, prt_denoise_guided*,
prt_accum_*_denoised_guided, include/prt.h; api.Scene.denoise_guided, api.AdaptiveAccumulator.variance / denoised_guided;
Camera::DenoiseGuided).  The filter is pinned against the numpy float64 model of tests/denoise_guided_model.py, the variance
against tests/adaptive_model.py bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, build, scenes
from tests import denoise_guided_model as G
from tests import denoise_model as M

pytestmark = pytest.mark.gpu

SCENES = {"tiny": scenes.tiny_scene, "mixed": scenes.mixed_materials}

# The bound is the plain filter's (tests/test_gpu_denoise.py): a weight's sensitivity to a rounding error of the luminance
# difference is e exp(-e) <= 0.37 whatever the denominator sigma_color sqrt(g) + 1e-4 is, and the device takes Y of the
# colour difference (close colours subtract exactly).  Measured on an MI355X: colour 7.8e-7 on the random inputs and 1.3e-6
# on the rendered frames; variance 7.3e-7 on the random inputs and 2.4e-6 on the firefly frame.  Only the filtered variance
# of the rendered frames exceeds it: 1.22e-5 on `tiny` (demodulate = 0; 1.01e-5 at the defaults, 1.13e-5 with seven
# levels), so there, and only there, the bound is 4 x the measured gap rounded up to one digit.
BOUND = 1e-5
BOUND_V_RENDERED = 5e-5


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def random_inputs(rng, h, w, miss=0.2, nan=0.0):
    rgb = rng.gamma(1.0, 0.5, (h, w, 3)).astype(np.float32)
    alb = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    z = rng.uniform(1.0, 3.0, (h, w)).astype(np.float32)
    z[rng.random((h, w)) < miss] = np.inf
    if nan:
        rgb[rng.random((h, w)) < nan, 0] = np.nan
    return rgb, {"albedo": alb, "normal": nrm, "depth": z}


def random_variance(rng, h, w):
    """gamma(1, 0.05) with about 5 % of the pixels set to each of 0, a negative number, NaN, +inf and 1e4."""
    v = rng.gamma(1.0, 0.05, (h, w)).astype(np.float32)
    u = rng.random((h, w))
    for k, bad in enumerate((0.0, -0.3, np.nan, np.inf, 1e4)):
        v[(u >= 0.05 * k) & (u < 0.05 * (k + 1))] = bad
    return v


PARAMS = [
    dict(),
    dict(demodulate=0),
    dict(iterations=1),
    dict(iterations=7),
    dict(sigma_color=0.0),
    dict(iterations=10, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
]


def filter_gap(got, ref):
    assert np.isfinite(got).all()
    scale = max(1e-30, float(np.abs(ref).max()))
    gap = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-4 * scale)
    return float(gap.max())


def model_of(rgb, var, feat, params):
    d = api.denoise_guided_defaults()
    d.update(params)
    return G.atrous_guided(rgb, var, feat["albedo"], feat["normal"], feat["depth"], **d)


def test_guided_defaults_differ_from_the_plain_ones_only_where_stated(gpu):
    g, p = api.denoise_guided_defaults(), api.denoise_defaults()
    assert {k for k in g if g[k] != p[k]} <= {"iterations", "sigma_color"}
    assert g["sigma_color"] in (1.0, 2.0, 4.0, 8.0) and g["iterations"] in (4, 5)  # a point of the documented sweep


def test_filter_matches_the_model_on_random_inputs(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rng = np.random.default_rng(11)
    worst_c = worst_v = 0.0
    for (h, w) in [(1, 1), (17, 1), (1, 23), (37, 53), (64, 64), (70, 33)]:
        rgb, feat = random_inputs(rng, h, w, nan=0.02)
        var = random_variance(rng, h, w)
        for params in PARAMS:
            got, gv = sc.denoise_guided(rgb, var, feat, return_variance=True, **params)
            ref, rv = model_of(rgb, var, feat, params)
            gc, gvv = filter_gap(got, ref), filter_gap(gv, rv)
            print(f"  {h}x{w} {params}: colour gap {gc:.2e}, variance gap {gvv:.2e}")
            worst_c, worst_v = max(worst_c, gc), max(worst_v, gvv)
            assert gc <= BOUND and gvv <= BOUND, ((h, w), params, gc, gvv)
            assert got.tobytes() == sc.denoise_guided(rgb, var, feat, **params).tobytes()  # with and without the variance out
    print(f"guided filter vs model, random inputs: largest relative gap colour {worst_c:.2e}, variance {worst_v:.2e}")


def adaptive_run(sc, **kw):
    acc = api.AdaptiveAccumulator(sc, rel_tol=0.1, abs_tol=0.0, min_spp=16, max_spp=64, batch=8, max_depth=8, seed=2, **kw)
    acc.run(16)
    return acc


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_filter_matches_the_model_on_rendered_frames(gpu, name):
    data = SCENES[name]()
    sc = api.Scene(data).upload(gpu)
    with adaptive_run(sc) as acc:
        rgb, var = acc.image(f32=True), acc.variance()
    feat = sc.features(seed=2)
    assert (var > 0).mean() > 0.3
    worst = 0.0
    for params in PARAMS:
        got, gv = sc.denoise_guided(rgb, var, feat, return_variance=True, **params)
        ref, rv = model_of(rgb, var, feat, params)
        gc, gvv = filter_gap(got, ref), filter_gap(gv, rv)
        print(f"  {name} {params}: colour gap {gc:.2e}, variance gap {gvv:.2e}")
        worst = max(worst, gc, gvv)
        assert gc <= BOUND and gvv <= BOUND_V_RENDERED, (params, gc, gvv)
    print(f"{name}: guided filter vs model on a rendered frame, largest relative gap {worst:.2e}")


def test_accumulator_variance_is_the_batch_means_estimate(gpu):
    sc = api.Scene(scenes.mixed_materials()).upload(gpu)
    with adaptive_run(sc) as acc:
        st, var = acc.export(), acc.variance()
        torch, dev = torch_dev()
        d = torch.empty(var.shape, dtype=torch.float32, device=dev)
        acc.variance(d_f32_ptr=d.data_ptr())
        torch.cuda.synchronize(dev)
        assert d.cpu().numpy().tobytes() == var.tobytes()
    cnt = st["counts"]
    assert (cnt == 64).any() and ((cnt >= 16) & (cnt < 64)).any(), np.unique(cnt)  # ran to the end / stopped early
    with np.errstate(all="ignore"):
        from tests import adaptive_model
        ref = np.float32(adaptive_model.estimate(st["sums"], st["moments"], cnt, 8)[1] / cnt)
    assert var.dtype == np.float32 and var.shape == cnt.shape
    assert np.array_equal(var, ref, equal_nan=True)
    assert np.array_equal(var, G.accum_variance(st["sums"], st["moments"], cnt, 8), equal_nan=True)
    assert np.isfinite(var).all() and (var > 0).any()
    # a tile share: pixels of the other rank have no samples and variance 0; the owned ones are the single-rank values
    with adaptive_run(sc, rank=0, nranks=2) as half:
        hv, hc = half.variance(), half.pixel_samples()
    assert (hc == 0).any() and (hc > 0).any()
    assert (hv[hc == 0] == 0).all()
    assert np.array_equal(hv[hc > 0], var[hc > 0])


def _device_pipeline(sc, acc, kw, torch, dev, **params):
    """prt_denoise_guided_device of prt_accum_resolve's fp32 frame, prt_accum_variance and prt_render_features."""
    cam = acc.camera
    H, W = cam.height, cam.width
    f32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    acc.resolve(d_f32_ptr=f32.data_ptr())
    var = torch.empty((H, W), dtype=torch.float32, device=dev)
    acc.variance(d_f32_ptr=var.data_ptr())
    al = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    nr = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    dp = torch.empty((H, W), dtype=torch.float32, device=dev)
    sc.features_device(al.data_ptr(), nr.data_ptr(), dp.data_ptr(), None, camera=cam, feature_spp=params.get("feature_spp", 1), **kw)
    out = torch.empty_like(f32)
    sc.denoise_guided_device(W, H, f32.data_ptr(), var.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), out.data_ptr(), **params)
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    sc.tonemap_srgb8(out.data_ptr(), W, H, u8.data_ptr())
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), u8.cpu().numpy()


@pytest.mark.parametrize("jitter", [False, True])
def test_accumulator_denoised_guided_is_the_device_pipeline(gpu, jitter):
    torch, dev = torch_dev()
    data = scenes.mixed_materials()
    sc = api.Scene(data).upload(gpu)
    kw = dict(max_depth=8, seed=4, pixel_jitter=jitter)
    acc = api.AdaptiveAccumulator(sc, rel_tol=0.1, abs_tol=0.0, min_spp=16, max_spp=64, batch=8, **kw)
    acc.run(16)
    H, W = data.camera.height, data.camera.width
    for params in (dict(), dict(iterations=3, sigma_color=2.0, feature_spp=3)):
        ref, ref8 = _device_pipeline(sc, acc, kw, torch, dev, **params)
        plain = acc.denoised(feature_spp=params.get("feature_spp", 1))
        got = acc.denoised_guided(**params)
        assert got.tobytes() == ref.tobytes(), params
        assert got.tobytes() != plain.tobytes()
        assert acc.denoised(feature_spp=params.get("feature_spp", 1)).tobytes() == plain.tobytes()  # one feature cache, undisturbed
        f32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        acc.resolve_denoised_guided(f32.data_ptr(), u8.data_ptr(), **params)
        torch.cuda.synchronize(dev)
        assert f32.cpu().numpy().tobytes() == ref.tobytes()
        assert np.array_equal(u8.cpu().numpy(), ref8)
        u8b = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        acc.resolve_denoised_guided(None, u8b.data_ptr(), **params)  # bytes only
        torch.cuda.synchronize(dev)
        assert np.array_equal(u8b.cpu().numpy(), ref8)
    acc.close()


def test_determinism_zero_iterations_and_colour_term_off(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rng = np.random.default_rng(5)
    rgb, feat = random_inputs(rng, 129, 67, nan=0.01)
    var = random_variance(rng, 129, 67)
    (a, av), (b, bv) = (sc.denoise_guided(rgb, var, feat, return_variance=True) for _ in range(2))
    assert a.tobytes() == b.tobytes() and av.tobytes() == bv.tobytes()
    z, zv = sc.denoise_guided(rgb, var, feat, return_variance=True, iterations=0, demodulate=1)
    assert z.tobytes() == rgb.tobytes()
    ok = np.isfinite(var) & (var >= 0)
    assert (~ok).any() and zv.tobytes() == np.where(ok, var, np.float32(0)).astype(np.float32).tobytes()
    for params in (dict(), dict(iterations=3, demodulate=0, sigma_normal=0.7)):
        off = sc.denoise_guided(rgb, var, feat, sigma_color=0.0, **params)
        d = api.denoise_guided_defaults()
        d.update(params)
        d.pop("sigma_color")
        plain = sc.denoise(rgb, feat, sigma_color=0.0, **d)
        np.testing.assert_allclose(off, plain, rtol=2e-6, atol=0)


def test_refusals(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)

    def refused(fn):
        with pytest.raises(api.PrtError) as e:
            fn()
        assert e.value.code == _abi.PRT_E_INVALID, e.value
    with api.Accumulator(sc, max_depth=6, seed=2) as plain:
        plain.add(16)
        refused(plain.denoised_guided)
        refused(plain.variance)
    with api.AdaptiveAccumulator(sc, rel_tol=0.1, abs_tol=0.0, min_spp=16, max_spp=32, batch=8, max_depth=6, seed=2) as acc:
        refused(acc.variance)  # nothing rendered
        acc.step(8)  # a single batch
        refused(acc.variance)
        refused(acc.denoised_guided)
        acc.step(8)
        assert acc.denoised_guided().shape == acc._shape
        refused(lambda: acc.denoised_guided(iterations=11))
        refused(lambda: acc.denoised_guided(sigma_normal=float("nan")))
    with api.AdaptiveAccumulator(sc, rel_tol=0.1, abs_tol=0.0, min_spp=16, max_spp=32, batch=8, max_depth=6, seed=2, rank=0,
                                 nranks=2) as two:
        two.run(16)
        refused(two.denoised_guided)
    rgb, feat = random_inputs(np.random.default_rng(1), 8, 8)
    var = np.full((8, 8), 0.01, np.float32)
    for bad in (dict(iterations=11), dict(iterations=-1), dict(demodulate=2), dict(sigma_color=float("nan")), dict(feature_spp=0)):
        refused(lambda: sc.denoise_guided(rgb, var, feat, **bad))
    # the raw call: a null variance, and an output that aliases an input
    L, p = sc._L, api.denoise_params(sc._L, guided=True)
    out = np.empty_like(rgb)
    ptr = lambda a: a.ctypes.data
    a, n, z = feat["albedo"], feat["normal"], feat["depth"]
    assert L.prt_denoise_guided(sc._h, 8, 8, ptr(rgb), None, ptr(a), ptr(n), ptr(z), C.byref(p), ptr(out), None) == _abi.PRT_E_INVALID
    assert L.prt_denoise_guided(sc._h, 8, 8, ptr(rgb), ptr(var), ptr(a), ptr(n), ptr(z), C.byref(p), ptr(rgb), None) == _abi.PRT_E_INVALID
    assert L.prt_denoise_guided(sc._h, 8, 8, ptr(rgb), ptr(var), ptr(a), ptr(n), ptr(z), C.byref(p), ptr(out), ptr(var)) == _abi.PRT_E_INVALID
    assert L.prt_denoise_guided(sc._h, 8, 8, ptr(rgb), ptr(var), ptr(a), ptr(n), ptr(z), C.byref(p), ptr(out), None) == 0


def test_firefly_frame_on_the_device(gpu):
    """The firefly frame of tests/test_denoise_guided_cpu.py: the pixel at 100 with variance 1e4 comes out below half its
    input, and the device agrees with the model."""
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rgb, var, feat = G.firefly_frame()
    at = (13, 19)
    params = dict(api.denoise_guided_defaults(), demodulate=0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    got, gv = sc.denoise_guided(rgb, var, feat, return_variance=True, **params)
    ref, rv = G.atrous_guided(rgb, var, feat["albedo"], feat["normal"], feat["depth"], **params)
    gc, gvv = filter_gap(got, ref), filter_gap(gv, rv)
    print(f"firefly on the device: {got[at][0]:.4f} of 100; gaps to the model colour {gc:.2e}, variance {gvv:.2e}")
    assert gc <= BOUND and gvv <= BOUND
    assert (got[at] < 50.0).all()
    assert (sc.denoise(rgb, feat, **dict(api.denoise_defaults(), demodulate=0, sigma_normal=0.0, sigma_depth=0.0,
                                         sigma_albedo=0.0))[at] > 99.0).all()


def test_guided_quality_on_cornell_box(gpu):
    """cornell-box 256^2, depth 20, 32 spp (min = max = 32, batch 4) seed 1 against a 4096-spp seed-2 reference: the guided
    filter at its defaults lowers the relMSE.  The figures are printed (DESIGN.md §7 has the table)."""
    data = scenes.cornell_box(width=256, height=256)
    sc = api.Scene(data).upload(gpu)
    ref = sc.render(spp=4096, max_depth=20, seed=2)
    with api.AdaptiveAccumulator(sc, rel_tol=0.0, abs_tol=0.0, min_spp=32, max_spp=32, batch=4, max_depth=20, seed=1) as acc:
        acc.run(32)
        assert (acc.pixel_samples() == 32).all()
        raw = acc.image()
        plain = acc.denoised()
        guided = acc.denoised_guided()
    r_raw, r_plain, r_guided = M.rel_mse(raw, ref), M.rel_mse(plain, ref), M.rel_mse(guided, ref)
    print(f"cornell-box 256^2 32 spp: relMSE raw {r_raw:.4g}, plain {r_plain:.4g} (x{r_plain / r_raw:.3f}), "
          f"guided {r_guided:.4g} (x{r_guided / r_raw:.3f})")
    assert r_guided < r_raw, (r_raw, r_guided)


def test_cpp_camera_denoise_guided_and_driver(gpu, tmp_path):
    build.build_host_example()
    lib_dir = os.path.dirname(build.HOST_LIB)
    root = os.path.dirname(lib_dir)
    exe = str(tmp_path / "denoise_guided_camera")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "denoise_guided_camera.cpp"), "-L", lib_dir,
                           "-Wl,-rpath," + lib_dir, "-lpooraytracer_host", "-lprt_hip", "-o", exe])
    data = scenes.tiny_scene()
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    cam_png = str(tmp_path / "camera.png")
    f64 = str(tmp_path / "camera.f64")
    r = subprocess.run([exe, res, data.name, "32", "6", "0.1", "16", f64, cam_png], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = tmp_path / "driver"
    out.mkdir()
    r = subprocess.run([build.MAIN_EXE, res, data.name, "32", "6", str(out), "--adaptive=0.1", "--min-spp=16", "--denoise-guided"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "variance-guided denoise (%d levels)" % api.denoise_guided_defaults()["iterations"] in r.stdout
    files = sorted(os.listdir(out))
    guided = [f for f in files if f.endswith("_guided.png")]
    assert len(guided) == 1 and guided[0][:-4] + ".hdr" in files, files
    for ext in (".png", ".hdr"):  # the driver's files are Camera::DenoiseGuided's attachment
        assert (out / (guided[0][:-4] + ext)).read_bytes() == open(cam_png[:-4] + ext, "rb").read(), ext
    assert (out / guided[0]).read_bytes() != (out / guided[0].replace("_guided.png", ".png")).read_bytes()
    # ... and the attachment is the binding's guided frame of the same adaptive render
    cam = data.camera
    img = np.fromfile(f64, dtype=np.float64).reshape(cam.height, cam.width, 3)
    sc = api.Scene(scenes.apply_loader_uv_fixup(data)).upload(gpu)
    with api.AdaptiveAccumulator(sc, rel_tol=0.1, abs_tol=0.0, min_spp=16, max_spp=32, max_depth=6, seed=1) as acc:
        acc.run(16)
        assert np.array_equal(img, acc.denoised_guided().astype(np.float64))
    # without --adaptive the flag is refused
    r = subprocess.run([build.MAIN_EXE, res, data.name, "32", "6", str(out), "--denoise-guided"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "--denoise-guided needs --adaptive" in r.stderr
    r = subprocess.run([build.MAIN_EXE, res, data.name, "32", "6", str(out), "--adaptive=0.1", "--denoise-guided=11"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "1..10" in r.stderr
