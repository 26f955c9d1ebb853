"""Radiance queries (-m gpu): prt_ray_color — K3 with a caller-supplied ray source (the PRT_FEAT_RAYS instantiations of k_render)
— on the scene family of tests/test_gpu_kernel_matrix.py (40x32, spp 8, depth 8; every material permutation, quad and
icosphere lights).

  1. a batch of two cameras' rays keyed j*W+i is each camera's frame (1e-9 per channel, every pixel);
  2. rays no camera of the scene produces, per sample against the oracle (a 1x1 camera per ray);
  3. bit-exact invariances: order, splitting, default keys, duplicates, batch lengths around the wave size;
  4. sample ranges add up;  5. misses and counters;  6. the no-LDS and padded-stride variants;  7. fp32 at tier 2;
  8. after a device-side refit;  9. arguments.

Tolerances: 1e-9 per channel is the project's fp64 tier against the oracle (compare_images, no exceptions below 10^5
pixels); 1e-12 between summation orders / kernel variants of the same arithmetic (a sum of at most 8 terms of fp64
rounding 1.1e-16 each); everything else is bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, scenes
from tests.test_gpu_f32 import check_image_tier2, oracle_tier2_reference
from tests.test_gpu_kernel_matrix import DEPTH, SCENES, SPP, _close, _data, _seed, _upload, variant
from tests.test_gpu_parity import compare_images

pytestmark = pytest.mark.gpu
F64, F32 = _abi.PRECISION_F64, _abi.PRECISION_F32
LLDS, PAD = _abi.VARIANT_LLDS, _abi.VARIANT_PAD
W, H = 40, 32


def camera_b(data):
    """A second view of the matrix scene: another eye, another look-at."""
    return scenes.Camera(W, H, 50.0, eye=(0.31, 0.27, 0.78), look_at=(-0.12, -0.31, -0.2))


def camera_batch(cam):
    """The oracle's camera rays of `cam` in pixel order, and their keys j*W+i."""
    r = oracle.camera_rays(cam).reshape(-1, 6)
    rays = np.zeros(r.shape[0], dtype=_abi.RAY_DTYPE)
    rays["o"], rays["d"] = r[:, :3], r[:, 3:]
    rays["tmin"], rays["tmax"] = 123.0, -1.0  # not read by the call: an interval that would hide every hit if it were
    return rays, np.arange(r.shape[0], dtype=np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


_SCENES = {}


def _scene(gpu, perm, lighting):
    """One upload per scene of the family, shared by the tests that do not change it."""
    if (perm, lighting) not in _SCENES:
        _SCENES[(perm, lighting)] = api.Scene(_data(perm, lighting)).upload(gpu)
    return _SCENES[(perm, lighting)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("perm,lighting", SCENES)
def test_two_cameras_in_one_batch_are_their_frames(gpu, perm, lighting):
    data = _data(perm, lighting)
    sc = _scene(gpu, perm, lighting)
    cams = (data.camera, camera_b(data))
    parts = [camera_batch(c) for c in cams]
    rays = np.concatenate([p[0] for p in parts])
    keys = np.concatenate([p[1] for p in parts])
    kw = dict(spp=SPP, max_depth=DEPTH, seed=_seed(perm, lighting), sample_chunks=2)
    out = sc.ray_color(rays, keys, **kw)
    cnt = sc.counters()
    assert cnt["samples"] == rays.shape[0] * SPP
    assert cnt["rays_closest"] >= 2 * rays.shape[0] and cnt["rays_shadow"] > 0 and cnt["kernel_ms"] > 0
    for k, cam in enumerate(cams):
        frame = sc.render(camera=cam, **kw)
        assert frame.max() > 0
        img = out[k * W * H:(k + 1) * W * H].reshape(H, W, 3)
        assert compare_images(img, frame) == 0, (perm, lighting, "camera", "AB"[k])


# ------------------------------------------------------------------------------------------------ 2
def probe_rays(data, n=333, seed=11):
    """Random origins inside the box and surface points pushed 1e-3 along the normal, with random directions."""
    rng = np.random.default_rng(seed)
    n_in = n // 2
    o_in = rng.uniform(-0.9, 0.9, (n_in, 3))
    v = np.asarray(data.vertices, dtype=np.float64)
    cdf = np.cumsum(0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=-1))
    p = scenes.surface_points(data, n - n_in, np.random.default_rng(seed + 1))
    # the triangle each point lies on, as surface_points drew it (same generator state, same first draw)
    tri = np.minimum(np.searchsorted(cdf, np.random.default_rng(seed + 1).random(n - n_in) * cdf[-1]), v.shape[0] - 1)
    nrm = np.cross(v[tri, 1] - v[tri, 0], v[tri, 2] - v[tri, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    o = np.concatenate([o_in, p + 1e-3 * nrm])
    d = rng.normal(size=(n, 3))
    d *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(d, axis=-1, keepdims=True)  # not normalised, like camera directions
    return o, d


def one_ray_camera(o, d):
    up = (0.0, 1.0, 0.0) if abs(d[1]) < 0.9 * np.linalg.norm(d) else (1.0, 0.0, 0.0)
    return scenes.Camera(1, 1, 30.0, eye=tuple(o), look_at=tuple(o + d), up=up)


@pytest.mark.parametrize("perm,lighting", [("lean", "quad"), ("all", "sphere")])
def test_probe_rays_match_the_oracle_per_sample(gpu, perm, lighting):
    data = _data(perm, lighting)
    sc = _scene(gpu, perm, lighting)
    o, d = probe_rays(data)
    n = o.shape[0]
    kw = dict(max_depth=DEPTH, seed=_seed(perm, lighting))
    orc = oracle.Oracle(data)
    rays = np.zeros(n, dtype=_abi.RAY_DTYPE)
    want = np.zeros((n, 4, 3))
    for i in range(n):
        cam = one_ray_camera(o[i], d[i])
        r = oracle.camera_rays(cam).reshape(6)
        # the oracle's one pixel-centre ray IS (o_i, d_i), up to the rounding of Camera::Initialize's arithmetic
        assert np.array_equal(r[:3], o[i])
        assert np.abs(r[3:] - d[i]).max() <= 8 * np.finfo(np.float64).eps * max(1.0, np.abs(o[i]).max(), np.abs(d[i]).max()), i
        rays["o"][i], rays["d"][i] = r[:3], r[3:]
        want[i] = orc.render_samples([(0, 0)], camera=cam, sample_begin=0, sample_count=4, spp=1, **kw)[0]
    assert (want.max(axis=(1, 2)) > 0).mean() > 0.5  # the rays see lit surfaces
    keys = np.zeros(n, dtype=np.uint32)  # the oracle's pixel (0, 0)
    for s in range(4):
        got = sc.ray_color(rays, keys, sample_begin=s, spp=1, **kw)
        err = np.abs(got - want[:, s])
        bad = (err > 1e-9 * np.abs(want[:, s]) + 1e-12).any(-1)
        print(f"{perm}/{lighting} sample {s}: max abs err {err.max():.3e}, rays outside: {int(bad.sum())}")
        assert not bad.any(), (perm, lighting, s, np.argwhere(bad)[:8].ravel().tolist())


# ------------------------------------------------------------------------------------------------ 3
def _mixed_batch(data):
    """1280 + 37 rays: camera A's frame and the first 37 of camera B's, every ray with a key of its own."""
    a, _ = camera_batch(data.camera)
    b, _ = camera_batch(camera_b(data))
    rays = np.concatenate([a, b[:37]])
    return rays, (np.arange(rays.shape[0], dtype=np.uint32) * 7 + 3).astype(np.uint32)


@pytest.mark.parametrize("perm,lighting", [("all", "sphere"), ("tex", "quad")])
def test_bit_exact_invariances(gpu, perm, lighting):
    data = _data(perm, lighting)
    sc = _scene(gpu, perm, lighting)
    rays, keys = _mixed_batch(data)
    n = rays.shape[0]
    assert n == 1280 + 37
    kw = dict(spp=4, max_depth=DEPTH, seed=_seed(perm, lighting), sample_chunks=2)
    base = sc.ray_color(rays, keys, **kw)
    assert base.max() > 0
    # order
    order = np.random.default_rng(3).permutation(n)
    assert np.array_equal(bits(sc.ray_color(rays[order], keys[order], **kw)), bits(base[order]))
    # two calls
    cut = 700
    two = np.concatenate([sc.ray_color(rays[:cut], keys[:cut], **kw), sc.ray_color(rays[cut:], keys[cut:], **kw)])
    assert np.array_equal(bits(two), bits(base))
    # default keys
    own = sc.ray_color(rays, None, **kw)
    assert np.array_equal(bits(own), bits(sc.ray_color(rays, np.arange(n, dtype=np.uint32), **kw)))
    assert not np.array_equal(bits(own), bits(base))
    # a ray listed twice with one key; the same ray under two keys
    o = np.array([0.8, 0.0, 0.8])
    dup = np.zeros(130, dtype=_abi.RAY_DTYPE)
    dup["o"], dup["d"] = o, (0.0, -1.0, 0.0)  # straight down onto the white floor, clear of every ball
    k2 = np.full(130, 5, dtype=np.uint32)
    k2[1::2] = 6
    r = sc.ray_color(dup, k2, **kw)
    assert (bits(r[0::2]) == bits(r[0])).all() and (bits(r[1::2]) == bits(r[1])).all()
    assert r[0].max() > 0 and not np.array_equal(r[0], r[1])
    # lengths around the wave size: a prefix of the batch gives the prefix of the result
    for m in (1, 63, 64, 65):
        assert np.array_equal(bits(sc.ray_color(rays[:m], keys[:m], **kw)), bits(base[:m])), m


# ------------------------------------------------------------------------------------------------ 4
def test_sample_ranges_add_up(gpu):
    perm, lighting = "ct", "quad"
    data = _data(perm, lighting)
    sc = _scene(gpu, perm, lighting)
    rays, keys = _mixed_batch(data)
    kw = dict(max_depth=DEPTH, seed=_seed(perm, lighting))
    singles = [sc.ray_color(rays, keys, sample_begin=s, spp=1, **kw) for s in range(4)]
    assert not np.array_equal(singles[0], singles[1])
    whole = sc.ray_color(rays, keys, spp=4, sample_chunks=4, **kw)
    mean = np.mean(singles, axis=0)
    assert np.allclose(whole, mean, rtol=1e-12, atol=0.0), float(np.abs(whole - mean).max())
    # and a range that does not start at 0
    later = sc.ray_color(rays, keys, sample_begin=2, spp=2, sample_chunks=2, **kw)
    assert np.allclose(later, 0.5 * (singles[2] + singles[3]), rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("perm,lighting", [("lean", "quad"), ("all", "sphere")])  # per-sample flow; the glossy kernels' flat shortcut
@pytest.mark.parametrize("chunks", [1, 3])
def test_misses_and_counters(gpu, perm, lighting, chunks):
    sc = _scene(gpu, perm, lighting)
    n, spp = 333, 4
    rng = np.random.default_rng(2)
    rays = np.zeros(n, dtype=_abi.RAY_DTYPE)
    rays["o"] = rng.uniform(-1, 1, (n, 3)) + (0.0, 0.0, 5.0)  # outside the closed box ...
    rays["d"] = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(0.5, 2.0, n)], -1)  # ... pointing away
    bg = (0.25, 0.5, 0.125)
    out, out32 = sc.ray_color(rays, spp=spp, max_depth=DEPTH, seed=1, sample_chunks=chunks, background=bg, f32=True)
    assert np.array_equal(out, np.tile(bg, (n, 1)))  # (4 terms of bg / 4: exact in binary)
    assert np.array_equal(out32, out.astype(np.float32))
    cnt = sc.counters()
    assert cnt["rays_closest"] == n * chunks  # one primary ray per work item, not per sample
    assert cnt["rays_shadow"] == 0
    assert cnt["samples"] == n * spp


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("perm,lighting,no_lds,stride", [("all", "sphere", 1, 96), ("tex", "quad", 0, 128), ("lean", "quad", 1, 128)])
def test_no_lds_and_padded_variants(gpu, dev_lib, monkeypatch, perm, lighting, no_lds, stride):
    data = _data(perm, lighting)
    rays, _ = _mixed_batch(data)
    keys = np.arange(rays.shape[0], dtype=np.uint32)  # camera A's rays come first: their keys are its pixel indices
    kw = dict(spp=SPP, max_depth=DEPTH, seed=_seed(perm, lighting), sample_chunks=2)
    ref = _upload(monkeypatch, data, 0, 96)
    v0 = variant(ref)
    assert v0 & LLDS and not v0 & PAD
    want = ref.ray_color(rays, keys, **kw)
    frame = ref.render(**kw)
    assert compare_images(want[:W * H].reshape(H, W, 3), frame) == 0
    ref.close()
    sc = _upload(monkeypatch, data, no_lds, stride)
    v = variant(sc)
    assert bool(v & LLDS) == (not no_lds) and bool(v & PAD) == (stride == 128)
    got = sc.ray_color(rays, keys, **kw)
    assert _close(got, want, 1e-12), float(np.abs(got - want).max())
    assert _close(got[:W * H].reshape(H, W, 3), sc.render(**kw), 1e-12)
    sc.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("perm,lighting", [("lean", "quad"), ("all", "sphere")])
def test_fp32_batch_within_tier2_of_the_oracle(gpu, perm, lighting):
    data = _data(perm, lighting)
    spp, seed = 32, _seed(perm, lighting)
    ref, sigma = oracle_tier2_reference(data, spp, max_depth=DEPTH, seed=seed)  # what the fp32 frame tests compare with
    sc = api.Scene(data).upload(gpu)
    rays, keys = camera_batch(data.camera)
    img = sc.ray_color(rays, keys, spp=spp, max_depth=DEPTH, seed=seed, precision=F32).reshape(H, W, 3)
    check_image_tier2(img, ref, sigma, spp)
    assert sc.counters()["samples"] == W * H * spp
    # the fp32 frame kernels took the same paths from the same rays rounded to float
    frame = sc.render(spp=spp, max_depth=DEPTH, seed=seed, precision=F32)
    check_image_tier2(frame, ref, sigma, spp)
    sc.close()


# ------------------------------------------------------------------------------------------------ 8
def test_after_refit_device(gpu):
    import torch
    perm, lighting = "lean", "quad"
    data = _data(perm, lighting)
    sc = api.Scene(data).upload(gpu)
    rays, keys = camera_batch(data.camera)
    kw = dict(spp=SPP, max_depth=DEPTH, seed=_seed(perm, lighting), sample_chunks=2)
    before = sc.ray_color(rays, keys, **kw)
    m = data.mesh_names.index("ball1")
    a, b = int(data.mesh_first_tri[m]), int(data.mesh_first_tri[m + 1])
    v = np.array(data.vertices, dtype=np.float64, copy=True)
    v[a:b] += (0.04, 0.03, -0.05)  # one ball, a small displacement; no emitter moves
    d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    torch.cuda.synchronize()
    sc.refit_device(d_v.data_ptr())
    after = sc.ray_color(rays, keys, **kw)  # orders itself after the refit
    frame = sc.render(**kw)
    assert compare_images(after.reshape(H, W, 3), frame) == 0
    assert not np.array_equal(before, after)
    sc.close()


# ------------------------------------------------------------------------------------------------ 9
def test_arguments(gpu):
    import torch
    perm, lighting = "lean", "quad"
    data = _data(perm, lighting)
    sc = _scene(gpu, perm, lighting)
    L = sc._L
    rays, keys = camera_batch(data.camera)
    rays, keys = rays[:100].copy(), keys[:100].copy()
    n = 100
    kw = dict(spp=2, max_depth=DEPTH, seed=4)

    def refused(code, **over):
        with pytest.raises(api.PrtError) as e:
            sc.ray_color(rays, keys, **{**kw, **over})
        assert e.value.code == code, (over, str(e.value))
        assert "prt_ray_color" in str(e.value)

    refused(_abi.PRT_E_INVALID, spp=0)
    refused(_abi.PRT_E_INVALID, sample_begin=-1)
    refused(_abi.PRT_E_INVALID, sample_begin=2**31 - 2)  # + spp 2 = 2^31 > INT32_MAX
    refused(_abi.PRT_E_INVALID, precision=2)
    refused(_abi.PRT_E_INVALID, pixel_jitter=True)
    refused(_abi.PRT_E_INVALID, reserved=1)
    p = _abi.make_params(**kw)
    out = np.zeros((n, 3))
    # a null ray buffer with n > 0; both outputs null
    assert L.prt_ray_color(sc._h, None, None, n, C.byref(p), 0, out.ctypes.data, None) == _abi.PRT_E_INVALID
    assert L.prt_ray_color(sc._h, rays.ctypes.data, None, n, C.byref(p), 0, None, None) == _abi.PRT_E_INVALID
    assert L.prt_ray_color_device(sc._h, None, None, n, C.byref(p), 0, 1 << 21, None, None) == _abi.PRT_E_INVALID
    assert L.prt_ray_color_device(sc._h, 1 << 20, None, n, C.byref(p), 0, None, None, None) == _abi.PRT_E_INVALID
    # rays the host call checks
    for field, value in (("o", np.nan), ("o", np.inf), ("d", np.nan), ("d", -np.inf)):
        bad = rays.copy()
        bad[field][57, 1] = value
        with pytest.raises(api.PrtError) as e:
            sc.ray_color(bad, keys, **kw)
        assert e.value.code == _abi.PRT_E_INVALID and "ray 57" in str(e.value)
    bad = rays.copy()
    bad["d"][99] = 0.0
    with pytest.raises(api.PrtError) as e:
        sc.ray_color(bad, keys, **kw)
    assert e.value.code == _abi.PRT_E_INVALID and "ray 99" in str(e.value)
    # n x chunks >= 2^32 (refused before any buffer is touched: the pointers are never dereferenced)
    with pytest.raises(api.PrtError) as e:
        sc.ray_color_device(1 << 20, 2**26, 1 << 21, None, spp=64, sample_chunks=64, max_depth=DEPTH)
    assert e.value.code == _abi.PRT_E_LIMIT
    with pytest.raises(api.PrtError) as e:
        sc.ray_color_device(1 << 20, 2**32, 1 << 21, None, spp=1, max_depth=DEPTH)
    assert e.value.code == _abi.PRT_E_LIMIT
    # n == 0
    assert L.prt_ray_color(sc._h, None, None, 0, C.byref(p), 0, out.ctypes.data, None) == _abi.PRT_OK
    assert L.prt_ray_color_device(sc._h, None, None, 0, C.byref(p), 0, 1 << 21, None, None) == _abi.PRT_OK
    assert sc.ray_color(rays[:0], **kw).shape == (0, 3)
    # sentinels behind the n-th triple; f64-only, f32-only and both
    want = sc.ray_color(rays, keys, **kw)
    assert want.max() > 0
    b64 = np.full(n * 3 + 16, -7.0)
    b32 = np.full(n * 3 + 16, -7.0, dtype=np.float32)
    assert L.prt_ray_color(sc._h, rays.ctypes.data, keys.ctypes.data, n, C.byref(p), 0, b64.ctypes.data, b32.ctypes.data) == 0
    assert np.array_equal(b64[:n * 3].reshape(n, 3), want) and (b64[n * 3:] == -7.0).all()
    assert np.array_equal(b32[:n * 3].reshape(n, 3), want.astype(np.float32)) and (b32[n * 3:] == -7.0).all()
    only32 = np.full(n * 3 + 16, -7.0, dtype=np.float32)
    assert L.prt_ray_color(sc._h, rays.ctypes.data, keys.ctypes.data, n, C.byref(p), 0, None, only32.ctypes.data) == 0
    assert np.array_equal(only32, b32)
    # the device call: buffers with a margin, on a stream of its own
    d_rays = torch.from_numpy(rays.view(np.float64).reshape(n, 8)).cuda()
    d_keys = torch.from_numpy(keys.view(np.int32)).cuda()
    d64 = torch.full((n * 3 + 16,), -7.0, dtype=torch.float64, device="cuda")
    d32 = torch.full((n * 3 + 16,), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sc.ray_color_device(d_rays.data_ptr(), n, d64.data_ptr(), d32.data_ptr(), d_keys_ptr=d_keys.data_ptr(), stream=st.cuda_stream, **kw)
    st.synchronize()
    assert np.array_equal(d64.cpu().numpy(), b64) and np.array_equal(d32.cpu().numpy(), b32)
    # max_depth < 0: zeros (and nothing behind them)
    z = np.full(n * 3 + 16, -7.0)
    pz = _abi.make_params(**{**kw, "max_depth": -1})
    assert L.prt_ray_color(sc._h, rays.ctypes.data, keys.ctypes.data, n, C.byref(pz), 0, z.ctypes.data, None) == 0
    assert (z[:n * 3] == 0.0).all() and (z[n * 3:] == -7.0).all()


def test_close_shared_scenes(gpu):
    """(housekeeping: the uploads the tests above shared)"""
    for sc in _SCENES.values():
        sc.close()
    _SCENES.clear()
