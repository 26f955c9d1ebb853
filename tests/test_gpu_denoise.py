"""GPU tests of the first-hit feature buffers and the a-trous denoiser (prt_render_features / prt_denoise* /
prt_accum_*_denoised, include/prt.h; api.Scene.features / denoise, api.Accumulator.denoised; Camera::Denoise).

Features are pinned against the CPU oracle's camera rays and closest hits; the filter against the numpy float64 model of
tests/denoise_model.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, build, scenes
from tests import denoise_model as M

pytestmark = pytest.mark.gpu

SCENES = {"tiny": scenes.tiny_scene, "mixed": scenes.mixed_materials}


def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def oracle_features(data, orc, dirs):
    """Model features of one sample per pixel: camera rays with directions `dirs` (H, W, 3) traced by the oracle."""
    cam = data.camera
    center, _, _, _ = M.camera_setup(cam)
    rays = np.zeros(cam.width * cam.height, dtype=_abi.RAY_DTYPE)
    rays["o"] = center
    rays["d"] = dirs.reshape(-1, 3)
    rays["tmin"], rays["tmax"] = 1e-4, np.inf
    hits = orc.trace_closest(rays)
    a, n, z = M.hit_features(data, rays["d"], hits, orc.texture_value)
    return a, n, z, hits["prim"]


def assert_features_close(got, a, n, z, mask=None):
    """got (device, fp32) against model float64 features rounded to fp32; returns the pixels that differ."""
    H, W = got["depth"].shape
    bad = np.zeros(H * W, bool)
    ga, gn, gz = got["albedo"].reshape(-1, 3), got["normal"].reshape(-1, 3), got["depth"].reshape(-1)
    bad |= (np.abs(ga - a.astype(np.float32)) > 1e-6 * np.maximum(1.0, np.abs(a))).any(1)
    bad |= (np.abs(gn - n.astype(np.float32)) > 2e-7 + 1e-6 * np.abs(n)).any(1)
    fin = np.isfinite(z)
    bad |= fin != np.isfinite(gz)
    both = fin & np.isfinite(gz)
    bad[both] |= np.abs(gz[both] - z[both].astype(np.float32)) > 1e-6 * z[both]
    return np.flatnonzero(bad)


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_features_match_the_oracle_without_jitter(gpu, name):
    data = SCENES[name]()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    got = sc.features(seed=3)
    rays = oracle.camera_rays(cam)
    a, n, z, prim = oracle_features(data, orc, rays[..., 3:])
    assert np.array_equal(got["prim"].reshape(-1), prim)
    assert (prim >= 0).mean() > 0.5
    bad = assert_features_close(got, a, n, z)
    assert bad.size == 0, (name, bad[:10].tolist())
    # every sample is the same ray: the means over 4 samples are the one sample's features, bit for bit
    got4 = sc.features(seed=3, feature_spp=4)
    for k in got:
        assert np.array_equal(got4[k], got[k]), k
    if name == "mixed":  # every material kind is on screen, the textured ones included
        first = np.asarray(data.mesh_first_tri, np.int64)
        kinds = {data.materials[data.mesh_material[m]].type for m in np.unique(np.searchsorted(first, prim[prim >= 0], side="right") - 1)}
        assert {0, 1, 2, 3, 5} <= kinds, kinds


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_features_match_the_oracle_with_jitter(gpu, name):
    data = SCENES[name]()
    cam = data.camera
    seed, spp = 5, 3
    sc = api.Scene(data).upload(gpu)
    orc = oracle.Oracle(data)
    got = sc.features(seed=seed, feature_spp=spp, pixel_jitter=True)
    per, prim0 = [], None
    for s in range(spp):
        a, n, z, prim = oracle_features(data, orc, M.jittered_rays(cam, seed, s, oracle.rng_stream))
        per.append((a, n, z))
        if s == 0:
            prim0 = prim
    a, n, z = M.mean_features(per)
    # the rays are the library's up to the rounding of pixel00 + fx du + fy dv: a ray within that of a triangle edge may
    # hit the neighbour.  Such knife-edge pixels are counted and bounded, not hidden.
    prim_diff = int((got["prim"].reshape(-1) != prim0).sum())
    bad = assert_features_close(got, a, n, z)
    print(f"{name}: jittered features, {bad.size} of {z.size} pixels off the model, {prim_diff} sample-0 triangles differ")
    assert bad.size <= max(2, z.size // 200), bad[:10].tolist()
    assert prim_diff <= max(2, z.size // 200)
    # jitter changes the rays: the features are not the pixel-centre ones
    assert not np.array_equal(got["depth"], sc.features(seed=seed)["depth"])


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


PARAMS = [
    dict(),
    dict(demodulate=0),
    dict(iterations=1, sigma_color=0.3, sigma_normal=0.2, sigma_depth=0.05, sigma_albedo=0.3),
    dict(iterations=3, sigma_color=4.0, sigma_normal=0.0, sigma_depth=float("inf"), sigma_albedo=-1.0),
    dict(iterations=7, sigma_color=2.0, sigma_normal=1.0, sigma_depth=0.5, sigma_albedo=0.5, demodulate=0),
    dict(iterations=10, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
]


def filter_gap(got, ref):
    assert np.isfinite(got).all()
    scale = max(1e-30, float(np.abs(ref).max()))
    gap = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-4 * scale)
    return float(gap.max())


def test_filter_matches_the_model_on_random_inputs(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rng = np.random.default_rng(11)
    worst = 0.0
    for (h, w) in [(1, 1), (17, 1), (1, 23), (37, 53), (64, 64), (70, 33)]:
        rgb, feat = random_inputs(rng, h, w, nan=0.02)
        for params in PARAMS:
            got = sc.denoise(rgb, feat, **params)
            d = api.denoise_defaults()
            d.update(params)
            ref = M.atrous(rgb, feat["albedo"], feat["normal"], feat["depth"], **d)
            g = filter_gap(got, ref)
            assert g <= 1e-5, ((h, w), params, g)
            worst = max(worst, g)
    print(f"filter vs model, random inputs: largest relative gap {worst:.2e}")


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_filter_matches_the_model_on_real_frames(gpu, name):
    data = SCENES[name]()
    sc = api.Scene(data).upload(gpu)
    rgb = sc.render(spp=8, max_depth=8, seed=2).astype(np.float32)
    feat = sc.features(seed=2)
    worst = 0.0
    for params in PARAMS[:5]:
        got = sc.denoise(rgb, feat, **params)
        d = api.denoise_defaults()
        d.update(params)
        ref = M.atrous(rgb, feat["albedo"], feat["normal"], feat["depth"], **d)
        g = filter_gap(got, ref)
        assert g <= 1e-5, (params, g)
        worst = max(worst, g)
    print(f"{name}: filter vs model on a rendered frame, largest relative gap {worst:.2e}")


def test_filter_is_deterministic_and_zero_iterations_copy(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rgb, feat = random_inputs(np.random.default_rng(5), 129, 67, nan=0.01)
    a, b = sc.denoise(rgb, feat), sc.denoise(rgb, feat)
    assert a.tobytes() == b.tobytes()
    z = sc.denoise(rgb, feat, iterations=0, demodulate=1)
    assert z.tobytes() == rgb.tobytes()


def test_constant_after_demodulation_survives_on_the_device(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rng = np.random.default_rng(6)
    _, feat = random_inputs(rng, 45, 61)
    feat["albedo"][:3] = 0.0
    for k in (0.5, 7.0):
        rgb = (k * np.fmax(feat["albedo"], np.float32(M.EPS))).astype(np.float32)
        for params in (dict(), dict(iterations=6, sigma_color=0.01, sigma_normal=0.05, sigma_depth=0.01, sigma_albedo=0.02)):
            got = sc.denoise(rgb, feat, demodulate=1, **params)
            np.testing.assert_allclose(got, rgb, rtol=2e-6, atol=0)


def _device_pipeline(sc, acc, torch, dev, **params):
    """prt_denoise_device of prt_accum_resolve's fp32 frame and prt_render_features of the accumulator's camera."""
    cam = acc.camera
    H, W = cam.height, cam.width
    f32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    acc.resolve(d_f32_ptr=f32.data_ptr())
    al = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    nr = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    dp = torch.empty((H, W), dtype=torch.float32, device=dev)
    sc.features_device(al.data_ptr(), nr.data_ptr(), dp.data_ptr(), None, camera=cam, feature_spp=params.get("feature_spp", 1),
                       **acc._kw)
    out = torch.empty_like(f32)
    sc.denoise_device(W, H, f32.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), out.data_ptr(), **params)
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    sc.tonemap_srgb8(out.data_ptr(), W, H, u8.data_ptr())
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), u8.cpu().numpy()


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
def test_accumulator_denoised_is_the_device_pipeline(gpu, adaptive, jitter):
    torch, dev = torch_dev()
    data = scenes.mixed_materials()
    sc = api.Scene(data).upload(gpu)
    kw = dict(max_depth=8, seed=4, pixel_jitter=jitter)
    if adaptive:
        acc = api.AdaptiveAccumulator(sc, rel_tol=0.1, abs_tol=0.0, min_spp=16, max_spp=64, batch=8, **kw)
        acc.run(16)
    else:
        acc = api.Accumulator(sc, **kw)
        acc.add(12)
    acc._kw = kw
    H, W = data.camera.height, data.camera.width
    for params in (dict(), dict(iterations=3, sigma_color=2.0, feature_spp=3)):
        ref, ref8 = _device_pipeline(sc, acc, torch, dev, **params)
        got = acc.denoised(**params)
        assert got.tobytes() == ref.tobytes(), params
        f32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        acc.resolve_denoised(f32.data_ptr(), u8.data_ptr(), **params)
        torch.cuda.synchronize(dev)
        assert f32.cpu().numpy().tobytes() == ref.tobytes()
        assert np.array_equal(u8.cpu().numpy(), ref8)
        u8b = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        acc.resolve_denoised(None, u8b.data_ptr(), **params)  # bytes only
        torch.cuda.synchronize(dev)
        assert np.array_equal(u8b.cpu().numpy(), ref8)
    acc.close()


def test_moved_geometry_retraces_the_cached_features(gpu):
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    acc = api.Accumulator(sc, max_depth=6, seed=2)
    acc.add(8)
    before = acc.denoised()
    assert before.tobytes() == acc.denoised().tobytes()  # cached features: same frame
    sc.update_vertices(data.vertices * np.array([1.0, 1.0, 1.0]) + np.array([0.05, 0.0, 0.0]))
    after = acc.denoised()
    expect = sc.denoise(acc.image(f32=True), sc.features(max_depth=6, seed=2))
    assert after.tobytes() == expect.tobytes()
    assert after.tobytes() != before.tobytes()
    acc.reset()
    acc.close()
    two = api.Accumulator(sc, max_depth=6, seed=2, rank=0, nranks=2)
    two.add(2)
    with pytest.raises(api.PrtError) as e:
        two.denoised()
    assert e.value.code == _abi.PRT_E_INVALID
    two.close()


def test_argument_errors(gpu):
    sc = api.Scene(scenes.tiny_scene()).upload(gpu)
    rgb, feat = random_inputs(np.random.default_rng(1), 8, 8)
    for bad in (dict(iterations=11), dict(iterations=-1), dict(demodulate=2), dict(sigma_color=float("nan")), dict(feature_spp=0)):
        with pytest.raises(api.PrtError) as e:
            sc.denoise(rgb, feat, **bad)
        assert e.value.code == _abi.PRT_E_INVALID, bad
    with pytest.raises(api.PrtError) as e:
        sc.features(feature_spp=0)
    assert e.value.code == _abi.PRT_E_INVALID


def test_denoised_quality_on_cornell_box(gpu):
    """cornell-box 256^2, depth 20, 16 spp seed 1 against a 4096-spp seed-2 reference: default parameters at least halve
    the relMSE."""
    data = scenes.cornell_box(width=256, height=256)
    sc = api.Scene(data).upload(gpu)
    ref = sc.render(spp=4096, max_depth=20, seed=2)
    with api.Accumulator(sc, max_depth=20, seed=1) as acc:
        acc.add(16)
        raw = acc.image()
        den = acc.denoised()
    r_raw, r_den = M.rel_mse(raw, ref), M.rel_mse(den, ref)
    print(f"cornell-box 256^2 16 spp: relMSE raw {r_raw:.4g}, denoised {r_den:.4g}, ratio {r_den / r_raw:.3f}")
    assert r_den <= 0.5 * r_raw, (r_raw, r_den)


def test_cpp_camera_denoise_and_driver(gpu, tmp_path):
    build.build_host_example()
    data = scenes.tiny_scene()
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    for extra, tag in (([], "plain"), (["--ladder=4,8"], "ladder"), (["--adaptive=0.1", "--min-spp=16"], "adaptive")):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([build.MAIN_EXE, res, data.name, "32", "6", str(out), "--denoise=3"] + extra, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        files = sorted(os.listdir(out))
        frames = [f for f in files if f.endswith(".png") and not f.endswith("_denoised.png")]
        assert len(frames) == (2 if tag == "ladder" else 1), files
        for f in frames:
            stem = f[:-4]
            assert stem + "_denoised.png" in files and stem + "_denoised.hdr" in files, files
            assert os.path.getsize(out / (stem + "_denoised.png")) > 100
        assert "denoised (3 levels)" in r.stdout
