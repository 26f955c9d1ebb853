"""GPU tests of progressive, resumable rendering (prt_accum_*, include/prt.h; api.Accumulator; Camera::RenderProgressive).

Sample s of pixel (i, j) draws from the stream keyed (seed, j*W+i, s) whatever pass renders it, so after n samples an
accumulator's frame is Scene.render(spp=n)'s: the same samples summed in another order (~1e-13 apart)."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, build, distributed, scenes

pytestmark = pytest.mark.gpu

KW = dict(max_depth=8, seed=3)


def close(a, b, tol):
    """Every pixel and channel within tol * max(1, |b|); returns the largest relative gap."""
    gap = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert np.isfinite(a).all() and gap.max() <= tol, (float(gap.max()), np.argwhere(gap > tol)[:5].tolist())
    return float(gap.max())


SCENES = {"tiny": scenes.tiny_scene, "mixed": lambda: scenes.mixed_materials()}


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_snapshots_equal_the_one_shot_frame(gpu, name, jitter):
    sc = api.Scene(SCENES[name]()).upload(gpu)
    worst = 0.0
    with api.Accumulator(sc, pixel_jitter=jitter, **KW) as acc:
        assert acc.samples == 0 and not acc.image().any()  # 0 samples resolve to zeros, not NaN
        n = 0
        for k in (1, 2, 7, 27):
            acc.add(k)
            n += k
            assert acc.samples == n
            img = acc.image()
            ref = sc.render(spp=n, pixel_jitter=jitter, **KW)
            assert ref.any()
            worst = max(worst, close(img, ref, 1e-11))
    print(f"{name} jitter={jitter}: largest relative gap to render(spp=n) {worst:.2e}")
    # prt_get_counters after a pass reports that pass
    with api.Accumulator(sc, **KW) as acc:
        acc.add(5)
        c = sc.counters()
        cam = sc.data.camera
        assert c["samples"] == cam.width * cam.height * 5 and c["rays_closest"] > 0 and c["kernel_ms"] > 0


def test_snapshot_matches_the_oracle(gpu):
    data = scenes.mixed_materials()
    sc = api.Scene(data).upload(gpu)
    with api.Accumulator(sc, **KW) as acc:
        acc.add(3).add(7)
        img = acc.image()
    ref, _ = oracle.Oracle(data).render(spp=10, **KW)
    bad = (np.abs(img - ref) > 1e-9 * np.maximum(1.0, np.abs(ref))).any(-1)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ from the oracle: {np.argwhere(bad)[:8].tolist()}"
    assert np.allclose(img.mean(axis=(0, 1)), ref.mean(axis=(0, 1)), rtol=1e-9)


def test_snapshot_is_the_mean_of_the_pixels_samples(gpu):
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    rng = np.random.default_rng(7)
    px = np.stack([rng.integers(0, data.camera.width, 16), rng.integers(0, data.camera.height, 16)], axis=1)
    with api.Accumulator(sc, **KW) as acc:
        for k in (4, 9):
            acc.add(k)
            n = acc.samples
            img = acc.image()
            mean = sc.render_samples(px, sample_begin=0, sample_count=n, **KW).mean(axis=1)
            close(img[px[:, 1], px[:, 0]], mean, 1e-12)


def test_determinism_and_pass_split(gpu):
    sc = api.Scene(scenes.mixed_materials()).upload(gpu)
    sums = []
    for _ in range(2):
        with api.Accumulator(sc, **KW) as acc:
            for k in (3, 5, 2):
                acc.add(k)
            sums.append(acc.state()[0])
    assert np.array_equal(sums[0], sums[1])  # same schedule: the same bits
    with api.Accumulator(sc, **KW) as ones, api.Accumulator(sc, **KW) as once:
        for _ in range(12):
            ones.add(1)
        once.add(12)
        close(ones.image(), once.image(), 1e-11)


def test_export_import_resumes_on_a_new_scene(gpu):
    data = scenes.mixed_materials()
    sc = api.Scene(data).upload(gpu)
    acc = api.Accumulator(sc, **KW)
    acc.add(20)
    sums, n, fp = acc.state()
    assert n == 20 and sums.shape == (data.camera.height, data.camera.width, 3)
    acc.close()
    sc.close()
    sc2 = api.Scene(scenes.mixed_materials()).upload(gpu)
    with api.Accumulator(sc2, **KW) as acc2:
        with pytest.raises(api.PrtError) as e:
            acc2.restore(sums, n, fp ^ 1)
        assert e.value.code == _abi.PRT_E_INVALID
        assert acc2.samples == 0
        acc2.restore(sums, n, fp)
        assert acc2.samples == 20
        acc2.add(30)
        close(acc2.image(), sc2.render(spp=50, **KW), 1e-11)
    # another seed is another fingerprint
    with api.Accumulator(sc2, max_depth=8, seed=4) as other:
        with pytest.raises(api.PrtError) as e:
            other.restore(sums, n, fp)
        assert e.value.code == _abi.PRT_E_INVALID


def test_tile_shares_sum_to_the_single_rank_frame(gpu):
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    W, H = data.camera.width, data.camera.height
    with api.Accumulator(sc, tile_size=16, **KW) as whole:
        whole.add(2).add(5)
        full = whole.image()
    total = np.zeros_like(full)
    for r in range(4):
        with api.Accumulator(sc, tile_size=16, rank=r, nranks=4, **KW) as acc:
            acc.add(2).add(5)
            part = acc.image()
            sums = acc.state()[0]
        mine = distributed.owned_mask(W, H, 16, r, 4)
        assert 0 < mine.sum() < W * H
        assert (part[~mine] == 0).all() and (sums[~mine] == 0).all()
        total += part
    close(total, full, 1e-12)


def test_resolve_srgb8_is_tonemap_of_the_fp32_frame(gpu):
    import torch
    data = scenes.mixed_materials()
    sc = api.Scene(data).upload(gpu)
    with api.Accumulator(sc, **KW) as acc:
        acc.add(6)
        u8 = acc.srgb8()
        f32 = acc.image(f32=True)
        f64 = acc.image()
        assert np.array_equal(f32, f64.astype(np.float32))
        H, W = f32.shape[:2]
        t = torch.from_numpy(f32).cuda()
        ref = torch.zeros(t.shape, dtype=torch.uint8, device="cuda")
        sc.tonemap_srgb8(t.data_ptr(), W, H, ref.data_ptr())
        # the device resolve writes all three outputs in one pass, to torch buffers
        d64 = torch.zeros(t.shape, dtype=torch.float64, device="cuda")
        d32 = torch.zeros(t.shape, dtype=torch.float32, device="cuda")
        d8 = torch.zeros(t.shape, dtype=torch.uint8, device="cuda")
        acc.resolve(d64.data_ptr(), d32.data_ptr(), d8.data_ptr())
        torch.cuda.synchronize()
    assert u8.shape == (H, W, 3) and u8.dtype == np.uint8 and u8.any()
    assert np.array_equal(u8, ref.cpu().numpy())
    assert np.array_equal(d8.cpu().numpy(), u8) and np.array_equal(d32.cpu().numpy(), f32)
    assert np.array_equal(d64.cpu().numpy(), f64)


def test_fp32_mode_snapshots(gpu):
    sc = api.Scene(scenes.mixed_materials()).upload(gpu)
    worst = 0.0
    with api.Accumulator(sc, precision=_abi.PRECISION_F32, **KW) as acc:
        n = 0
        for k in (1, 2, 7, 27):
            acc.add(k)
            n += k
            worst = max(worst, close(acc.image(), sc.render(spp=n, precision=_abi.PRECISION_F32, **KW), 1e-4))
    print(f"fp32 mode: largest relative gap to render(spp=n, precision=F32) {worst:.2e}")


def test_moved_geometry_stops_the_accumulator(gpu):
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    with api.Accumulator(sc, **KW) as acc:
        acc.add(3)
        moved = data.vertices * 0.9
        sc.update_vertices(moved)
        with pytest.raises(api.PrtError) as e:
            acc.add(1)
        assert e.value.code == _abi.PRT_E_INVALID
        assert acc.samples == 3
        acc.reset()
        assert acc.samples == 0
        acc.add(5)
        img = acc.image()
    fresh = api.Scene(dataclasses.replace(data, vertices=moved)).upload(gpu)
    close(img, fresh.render(spp=5, **KW), 1e-11)


def test_two_accumulators_on_two_streams(gpu):
    import torch
    sc = api.Scene(scenes.mixed_materials()).upload(gpu)
    seq = []
    for seed in (5, 6):
        with api.Accumulator(sc, max_depth=8, seed=seed) as acc:
            acc.add(3).add(4)
            seq.append(acc.image())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with api.Accumulator(sc, max_depth=8, seed=5) as a, api.Accumulator(sc, max_depth=8, seed=6) as b:
        a.add(3, stream=s1.cuda_stream)
        b.add(3, stream=s2.cuda_stream)
        a.add(4, stream=s1.cuda_stream)
        b.add(4, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(a.image(), seq[0]) and np.array_equal(b.image(), seq[1])


def test_accum_c_errors(gpu):
    import ctypes as C
    data = scenes.tiny_scene()
    sc = api.Scene(data).upload(gpu)
    L = sc._L
    c = _abi.make_camera(data.camera)
    h = C.c_void_p()
    p = _abi.make_params(**KW)
    p.reserved = 1
    assert L.prt_accum_create(sc._h, C.byref(c), C.byref(p), C.byref(h)) == _abi.PRT_E_INVALID
    p = _abi.make_params(**KW)
    assert L.prt_accum_create(sc._h, C.byref(c), C.byref(p), C.byref(h)) == 0
    try:
        assert L.prt_accum_render(h, 0, None) == _abi.PRT_E_INVALID
        assert L.prt_accum_render(h, -2, None) == _abi.PRT_E_INVALID
        assert L.prt_accum_resolve(h, None, None, None, None) == _abi.PRT_E_INVALID
        sums = np.zeros((data.camera.height, data.camera.width, 3))
        n, fp = C.c_uint64(0), C.c_uint64(0)
        assert L.prt_accum_export(h, sums.ctypes.data, C.byref(n), C.byref(fp)) == 0
        # resuming at the last representable sample index: one more sample would pass INT32_MAX
        assert L.prt_accum_import(h, sums.ctypes.data, 2**31 - 1, fp.value) == 0
        assert L.prt_accum_render(h, 1, None) == _abi.PRT_E_LIMIT
        assert L.prt_accum_import(h, sums.ctypes.data, 2**31, fp.value) == _abi.PRT_E_LIMIT
        assert L.prt_accum_import(h, sums.ctypes.data, 2**31 - 10, fp.value) == 0
        assert L.prt_accum_render(h, 11, None) == _abi.PRT_E_LIMIT
    finally:
        L.prt_accum_destroy(h)


def test_cpp_driver_ladder(gpu, tmp_path):
    from tests.golden.make_results_pairs import parse_hdr
    build.build_host_example()
    data = scenes.tiny_scene()
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    out = str(tmp_path / "o.f64")
    r = subprocess.run([build.MAIN_EXE, "--ladder=2,5", res, data.name, "100", "6", str(tmp_path), out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    files = sorted(os.listdir(tmp_path))
    for spp in (2, 5):
        tag = f"{data.name}_spp{spp}-depth6_"
        pngs = [f for f in files if f.startswith(tag) and f.endswith(".png")]
        hdrs = [f for f in files if f.startswith(tag) and f.endswith(".hdr")]
        assert len(pngs) == 1 and len(hdrs) == 1, files
    assert not [f for f in files if "spp100" in f]
    fixed = scenes.apply_loader_uv_fixup(data)
    ref = api.Scene(fixed).upload(gpu).render(spp=5, max_depth=6, seed=1)
    cam = data.camera
    close(np.fromfile(out, dtype=np.float64).reshape(cam.height, cam.width, 3), ref, 1e-11)
    hdr = [f for f in files if f.startswith(f"{data.name}_spp5-") and f.endswith(".hdr")][0]
    _, rgbe, _ = parse_hdr(open(os.path.join(tmp_path, hdr), "rb").read())
    e = rgbe[..., 3].astype(np.int32)
    q = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)[..., None]
    val = rgbe[..., :3].astype(np.float64) * q
    # the writer stores float(x) truncated to [m q, (m+1) q); allow half a quantum of slack on either side of that bracket
    d = ref.astype(np.float32).astype(np.float64) - val
    qe = np.where(q > 0, q, 1e-30)
    assert (d >= -0.5 * qe).all() and (d <= 1.5 * qe).all(), float(np.max(np.abs(d) / qe))
    bad = subprocess.run([build.MAIN_EXE, res, data.name, "--ladder=5,2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "strictly increasing" in bad.stderr
