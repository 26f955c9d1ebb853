"""GPU tests of adaptive sampling (prt_accum_*_adaptive, include/prt.h; api.AdaptiveAccumulator; Camera::RenderAdaptive).

Every running pixel shares the global count n, so a pixel that stopped after n_p samples holds Scene.render(spp=n_p)'s
value there; tests/adaptive_model.py restates a whole run in numpy from per-sample radiance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from pooraytracer_amd import _abi, api, build, scenes
from tests import adaptive_model as M

pytestmark = pytest.mark.gpu

KW = dict(max_depth=8, seed=3)
AD = dict(batch=8, min_spp=32, max_spp=256, abs_tol=0.0)
REL = {"tiny": 0.05, "mixed": 0.1}  # stop a good share of the pixels before max_spp (oracle: ~70 % and ~47 %)
SCENES = {"tiny": lambda: scenes.cornell_box(ball_subdiv=1, width=48, height=48), "mixed": lambda: scenes.mixed_materials()}


def close(a, b, tol):
    gap = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert np.isfinite(a).all() and gap.max() <= tol, (float(gap.max()), np.argwhere(gap > tol)[:5].tolist())
    return float(gap.max())


def adaptive_run(sc, rel_tol, rounds=32, **kw):
    ad = dict(AD, **{k: kw.pop(k) for k in list(kw) if k in AD})
    kw = dict(KW, **kw)
    acc = api.AdaptiveAccumulator(sc, rel_tol=rel_tol, **ad, **kw)
    history = []
    while True:
        k = acc.step(rounds)
        if k == 0:
            break
        history.append(k)
    return acc, history


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_adaptive_matches_the_model_on_oracle_radiance(gpu, name):
    model_parity(gpu, name, batch=AD["batch"], rounds=32)


def model_parity(gpu, name, batch, rounds):
    """An adaptive run with rounds of `rounds` samples in batches of `batch` against adaptive_model.run on the oracle's
    per-sample radiance: the same counts (a decision within 1e-9 of the threshold excepted), sums and moments."""
    ad = dict(AD, batch=batch)
    data = SCENES[name]()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    with adaptive_run(sc, REL[name], rounds=rounds, batch=batch)[0] as acc:
        got = acc.export()
        assert np.array_equal(got["counts"], acc.pixel_samples())
    px = np.stack(np.meshgrid(np.arange(cam.width), np.arange(cam.height)), -1).reshape(-1, 2)
    rad = oracle.Oracle(data).render_samples(px, sample_begin=0, sample_count=AD["max_spp"], **KW)
    ref = M.run(rad, rel_tol=REL[name], rounds=rounds, **ad)
    cnt = got["counts"].reshape(-1)
    stopped = (cnt < AD["max_spp"]).mean()
    assert 0.1 <= stopped <= 0.9, stopped
    diff = np.flatnonzero(cnt != ref["counts"])
    if diff.size:
        # only a decision within 1e-9 of the threshold may go the other way: at the smaller count, the model's se / threshold
        for i in diff:
            m = min(int(cnt[i]), int(ref["counts"][i]))
            sub = M.run(rad[i:i + 1, :m], rel_tol=REL[name], rounds=rounds, **dict(ad, max_spp=m))
            r = M.ratio(sub, REL[name], 0.0, batch)[0]
            print(f"{name}: pixel {i} count {cnt[i]} vs model {ref['counts'][i]}, model se/threshold at {m} = {r!r}")
            assert abs(r - 1.0) <= 1e-9, (i, r)
    same = np.setdiff1d(np.arange(cnt.size), diff)
    close(got["sums"].reshape(-1, 3)[same], ref["sums"][same], 1e-9)
    gap = np.abs(got["moments"].reshape(-1)[same] - ref["moments"][same]) / np.maximum(1e-300, np.abs(ref["moments"][same]))
    assert gap.max() <= 1e-9, float(gap.max())
    assert got["samples"] == ref["samples"]
    print(f"{name} batch {batch} rounds {rounds}: {stopped:.0%} stopped before max_spp, {diff.size} decisions at the threshold, "
          f"n_active {ref['n_active']}")
    return ref


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_each_count_is_the_fixed_spp_frame(gpu, name, jitter):
    sc = api.Scene(SCENES[name]()).upload(gpu)
    acc, hist = adaptive_run(sc, REL[name], pixel_jitter=jitter)
    with acc:
        img, cnt = acc.image(), acc.pixel_samples()
        assert acc.samples == cnt.max()
    worst = 0.0
    ms = np.unique(cnt)
    assert ms.size >= 3, ms
    for m in ms:
        ref = sc.render(spp=int(m), pixel_jitter=jitter, **KW)
        worst = max(worst, close(img[cnt == m], ref[cnt == m], 1e-11))
    print(f"{name} jitter={jitter}: counts {ms.tolist()}, n_active {hist}, largest gap {worst:.2e}")


def test_fp32_mode_each_count_is_the_fixed_spp_frame(gpu):
    sc = api.Scene(SCENES["mixed"]()).upload(gpu)
    acc, _ = adaptive_run(sc, REL["mixed"], precision=1)
    with acc:
        img, cnt = acc.image(), acc.pixel_samples()
    for m in np.unique(cnt):
        ref = sc.render(spp=int(m), precision=1, **KW)
        close(img[cnt == m], ref[cnt == m], 1e-4)


@pytest.mark.parametrize("k", [32, 64])
def test_no_stopping_is_the_plain_accumulator(gpu, k):
    import torch
    sc = api.Scene(SCENES["mixed"]()).upload(gpu)
    n = 128
    acc = api.AdaptiveAccumulator(sc, rel_tol=1e9, abs_tol=1e9, min_spp=n, max_spp=n, batch=8, **KW)
    plain = api.Accumulator(sc, sample_chunks=k // 8, **KW)
    with acc, plain:
        rounds = 0
        while acc.step(k):
            plain.add(k)
            rounds += 1
        assert rounds == n // k and acc.samples == plain.samples == n
        st, (sums, _, _) = acc.export(), plain.state()
        assert (st["counts"] == n).all()
        assert np.array_equal(st["sums"], sums)
        assert np.array_equal(acc.image(), plain.image())
        assert np.array_equal(acc.image(f32=True), plain.image(f32=True))
        assert np.array_equal(acc.srgb8(), plain.srgb8())
        torch.cuda.synchronize()


def test_zero_variance_pixels_stop_at_min_spp(gpu):
    data = SCENES["tiny"]()
    cam = data.camera
    sc = api.Scene(data).upload(gpu)
    acc, _ = adaptive_run(sc, 0.01)
    with acc:
        cnt = acc.pixel_samples().reshape(-1)
    assert ((cnt % AD["batch"]) == 0).all() and (cnt >= AD["min_spp"]).all() and (cnt <= AD["max_spp"]).all()
    px = np.stack(np.meshgrid(np.arange(cam.width), np.arange(cam.height)), -1).reshape(-1, 2)
    s = sc.render_samples(px, sample_begin=0, sample_count=AD["min_spp"], **KW)
    flat = (s == s[:, :1]).all(axis=(1, 2))  # camera ray missed or met an emitter: every sample the same radiance
    assert flat.sum() >= 4, flat.sum()
    assert (cnt[flat] == AD["min_spp"]).all(), np.unique(cnt[flat])
    assert (cnt[~flat] > AD["min_spp"]).mean() > 0.5  # rel_tol 0.01 keeps the noisy ones going


def test_determinism_and_tile_shares(gpu):
    sc = api.Scene(SCENES["mixed"]()).upload(gpu)
    runs = []
    for _ in range(2):
        acc, hist = adaptive_run(sc, REL["mixed"], tile_size=16)
        with acc:
            runs.append((acc.export(), hist))
    a, b = runs[0][0], runs[1][0]
    assert runs[0][1] == runs[1][1]
    for key in ("sums", "moments", "counts"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert (a["samples"], a["fingerprint"]) == (b["samples"], b["fingerprint"])
    parts = []
    for rank in (0, 1):
        acc, _ = adaptive_run(sc, REL["mixed"], tile_size=16, rank=rank, nranks=2)
        with acc:
            parts.append(acc.export())
    assert (parts[0]["counts"] > 0).any() and (parts[1]["counts"] > 0).any()
    assert not ((parts[0]["counts"] > 0) & (parts[1]["counts"] > 0)).any()
    assert np.array_equal(parts[0]["counts"] + parts[1]["counts"], a["counts"])
    assert np.array_equal(parts[0]["sums"] + parts[1]["sums"], a["sums"])
    assert np.array_equal(parts[0]["moments"] + parts[1]["moments"], a["moments"])


def test_checkpoint_resumes_on_a_new_scene_and_bad_input_is_refused(gpu):
    data = SCENES["mixed"]()
    sc = api.Scene(data).upload(gpu)
    full, _ = adaptive_run(sc, REL["mixed"])
    with full:
        want = full.export()
    with api.AdaptiveAccumulator(sc, rel_tol=REL["mixed"], **AD, **KW) as acc:
        assert acc.step(32) and acc.step(32)
        ck = acc.export()
        # a plain checkpoint and a plain pass cannot represent per-pixel counts
        sums = np.zeros((data.camera.height, data.camera.width, 3))
        n, fp = C.c_uint64(0), C.c_uint64(0)
        assert sc._L.prt_accum_export(acc._h, sums.ctypes.data, C.byref(n), C.byref(fp)) == _abi.PRT_E_INVALID
        assert sc._L.prt_accum_render(acc._h, 8, None) == _abi.PRT_E_INVALID
        assert sc._L.prt_accum_import(acc._h, sums.ctypes.data, 0, ck["fingerprint"]) == _abi.PRT_E_INVALID
        for bad_n in (12, 0, -8):  # not a multiple of batch / not positive
            with pytest.raises((api.PrtError, ValueError)):
                acc.step(bad_n)
    sc2 = api.Scene(data).upload(gpu)
    with api.AdaptiveAccumulator(sc2, rel_tol=REL["mixed"], **AD, **KW) as acc:
        acc.load(ck)
        assert acc.samples == 64
        while acc.step(32):
            pass
        got = acc.export()
        for key in ("sums", "moments", "counts"):
            assert got[key].tobytes() == want[key].tobytes(), key
        refused = [
            dict(ck, counts=ck["counts"] + np.uint32(8) * (ck["counts"] == 64)),  # a count above samples
            dict(ck, counts=ck["counts"] - np.uint32(4) * (ck["counts"] > 0)),  # not a multiple of batch
            dict(ck, moments=np.where(np.arange(ck["moments"].size).reshape(ck["moments"].shape) == 7, -1.0, ck["moments"])),
            dict(ck, moments=np.where(np.arange(ck["moments"].size).reshape(ck["moments"].shape) == 7, np.nan, ck["moments"])),
            dict(ck, fingerprint=ck["fingerprint"] ^ 1),
        ]
        for st in refused:
            with pytest.raises(api.PrtError) as e:
                acc.load(st)
            assert e.value.code == _abi.PRT_E_INVALID
    with api.AdaptiveAccumulator(sc2, rel_tol=REL["mixed"] * 2, **AD, **KW) as other:  # a different rel_tol
        with pytest.raises(api.PrtError) as e:
            other.load(ck)
        assert e.value.code == _abi.PRT_E_INVALID
    with api.AdaptiveAccumulator(sc2, rel_tol=REL["mixed"], **AD, **KW, tile_size=16, rank=1, nranks=2) as r1:
        one = dict(ck, fingerprint=r1.export()["fingerprint"])
        with pytest.raises(api.PrtError):  # rank 1 does not own every pixel that has samples
            r1.load(one)
    # every invalid PrtAdaptiveParams field
    c, p = _abi.make_camera(data.camera), _abi.make_params(**KW)
    h = C.c_void_p()
    good = dict(min_spp=32, max_spp=256, batch=8, reserved=0, rel_tol=0.1, abs_tol=0.0)
    for field, val in (("min_spp", 8), ("min_spp", 36), ("max_spp", 24), ("max_spp", 260), ("batch", -1), ("reserved", 1),
                       ("rel_tol", -0.1), ("rel_tol", float("nan")), ("abs_tol", float("inf")), ("abs_tol", -1.0)):
        a = _abi.PrtAdaptiveParams(**dict(good, **{field: val}))
        assert sc2._L.prt_accum_create_adaptive(sc2._h, C.byref(c), C.byref(p), C.byref(a), C.byref(h)) == _abi.PRT_E_INVALID, field
        assert not h.value
    a = _abi.PrtAdaptiveParams(**good)
    assert sc2._L.prt_accum_create_adaptive(sc2._h, C.byref(c), C.byref(p), C.byref(a), C.byref(h)) == 0
    sc2._L.prt_accum_destroy(h)


def test_counters_report_the_rounds_last_launch(gpu):
    sc = api.Scene(SCENES["tiny"]()).upload(gpu)
    with api.AdaptiveAccumulator(sc, rel_tol=REL["tiny"], **AD, **KW) as acc:
        acc.step(32)
        k = acc.step(32)
        c = sc.counters()
        assert 0 < k < 48 * 48 and c["samples"] == k * 32 and c["rays_closest"] > 0
    # a round longer than 64 batches is issued as several launches (512 + 16 samples here); the counters report the last
    n = 8 * 64 + 16
    with api.AdaptiveAccumulator(sc, rel_tol=0.0, abs_tol=0.0, min_spp=n, max_spp=n, batch=8, **KW) as acc:
        assert acc.step(n) == 48 * 48 and sc.counters()["samples"] == 48 * 48 * 16
        assert (acc.pixel_samples() == n).all() and acc.step(8) == 0


def test_cpp_driver_adaptive(gpu, tmp_path):
    build.build_host_example()
    data = scenes.tiny_scene()
    res = str(tmp_path / "res")
    scenes.export_obj(data, res)
    out, counts = str(tmp_path / "o.f64"), str(tmp_path / "c.u32")
    r = subprocess.run([build.MAIN_EXE, "--adaptive=0.05", res, data.name, "200", "6", str(tmp_path), out, "--min-spp=32",
                        f"--counts={counts}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    cam = data.camera
    cnt = np.fromfile(counts, dtype=np.uint32).reshape(cam.height, cam.width)
    files = sorted(os.listdir(tmp_path))
    tag = f"{data.name}_adaptive0.05_spp{cnt.max()}-depth6_"
    assert len([f for f in files if f.startswith(tag) and f.endswith(".png")]) == 1, files
    assert len([f for f in files if f.startswith(tag) and f.endswith(".hdr")]) == 1, files
    fixed = scenes.apply_loader_uv_fixup(data)
    sc = api.Scene(fixed).upload(gpu)
    b = _abi.ADAPTIVE_DEFAULT_BATCH
    with api.AdaptiveAccumulator(sc, rel_tol=0.05, abs_tol=0.0, min_spp=32, max_spp=200 // b * b, max_depth=6, seed=1) as acc:
        acc.run(32)
        img, want = acc.image(), acc.pixel_samples()
    assert np.array_equal(cnt, want)
    assert np.unique(cnt).size >= 2
    assert np.array_equal(np.fromfile(out, dtype=np.float64).reshape(cam.height, cam.width, 3), img)
    bad = subprocess.run([build.MAIN_EXE, res, data.name, "--adaptive=x"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--adaptive" in bad.stderr
