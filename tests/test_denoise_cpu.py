"""Feature buffers and the a-trous denoiser (prt_render_features / prt_denoise*, include/prt.h) without a GPU: the ABI
surface, the argument checks that come before any device work, the driver's option parsing, and the numpy model of
tests/denoise_model.py against its own invariants."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, build, scenes
from tests import denoise_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENOISE = ["prt_denoise_defaults", "prt_render_features", "prt_render_features_device", "prt_denoise", "prt_denoise_device",
           "prt_accum_resolve_denoised", "prt_accum_read_denoised"]


def test_denoise_symbols_declared_and_exported(prt_lib):
    hdr = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z0-9_]+)\s*\(", hdr))
    for name in DENOISE:
        assert name in declared and name in _abi.EXPORTS, name
        assert hasattr(prt_lib, name), f"{name} not exported by libprt_hip.so"
    assert prt_lib.prt_abi_version() == 6


def test_denoise_params_layout(tmp_path):
    src = tmp_path / "dn.c"
    T = _abi.PrtDenoiseParams
    offs = ",".join(f"offsetof(PrtDenoiseParams,{f})" for f, _ in T._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "prt.h"\nint main(){printf("' + "%zu " * (len(T._fields_) + 1)
                   + '\\n",sizeof(PrtDenoiseParams),' + offs + ");return 0;}\n")
    exe = tmp_path / "dn"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    assert C.sizeof(T) == 32


def test_defaults_are_valid(prt_lib):
    d = api.denoise_defaults()
    assert 1 <= d["iterations"] <= 10 and d["demodulate"] in (0, 1) and d["feature_spp"] >= 1
    assert all(np.isfinite(d[k]) and d[k] > 0 for k in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"))


def test_entry_points_without_a_device(prt_lib):
    sc = api.Scene(scenes.tiny_scene())  # never uploaded
    c, p = _abi.make_camera(sc.data.camera), _abi.make_params()
    dp = api.denoise_params()
    buf = np.zeros(64 * 64 * 3, np.float32)
    b = buf.ctypes.data
    assert prt_lib.prt_render_features(sc._h, C.byref(c), C.byref(p), 1, b, b, b, b) == _abi.PRT_E_NO_DEVICE
    assert prt_lib.prt_render_features_device(sc._h, C.byref(c), C.byref(p), 1, b, b, b, b, None) == _abi.PRT_E_NO_DEVICE
    assert prt_lib.prt_denoise(sc._h, 8, 8, b, b, b, b, C.byref(dp), b) == _abi.PRT_E_NO_DEVICE
    assert prt_lib.prt_denoise_device(sc._h, 8, 8, b, b, b, b, C.byref(dp), b, None) == _abi.PRT_E_NO_DEVICE
    assert prt_lib.prt_render_features(None, C.byref(c), C.byref(p), 1, b, b, b, b) == _abi.PRT_E_INVALID
    assert prt_lib.prt_denoise(None, 8, 8, b, b, b, b, C.byref(dp), b) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_resolve_denoised(None, C.byref(dp), b, None, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_read_denoised(None, C.byref(dp), b) == _abi.PRT_E_INVALID
    with pytest.raises(api.PrtError) as e:
        sc.features()
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    with pytest.raises(api.PrtError) as e:
        sc.denoise(np.zeros((4, 4, 3)), {"albedo": np.ones((4, 4, 3)), "normal": np.zeros((4, 4, 3)), "depth": np.ones((4, 4))})
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    sc.close()


def test_python_side_checks(prt_lib):
    with pytest.raises(TypeError):
        api.denoise_params(sigma=1.0)
    sc = api.Scene(scenes.tiny_scene())
    with pytest.raises(ValueError):
        sc.denoise(np.zeros((4, 4)), {"albedo": np.ones((4, 4, 3)), "normal": np.zeros((4, 4, 3)), "depth": np.ones((4, 4))})
    with pytest.raises(ValueError):
        sc.denoise(np.zeros((4, 4, 3)), {"albedo": np.ones((4, 5, 3)), "normal": np.zeros((4, 4, 3)), "depth": np.ones((4, 4))})
    sc.close()


def _random_inputs(rng, h, w, miss=0.2):
    rgb = rng.gamma(1.0, 0.5, (h, w, 3))
    alb = rng.uniform(0.0, 1.0, (h, w, 3))
    nrm = rng.normal(size=(h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    z = rng.uniform(1.0, 3.0, (h, w))
    z[rng.random((h, w)) < miss] = np.inf
    return rgb, alb, nrm, z


def test_model_iterations_zero_is_identity():
    rng = np.random.default_rng(1)
    rgb, alb, nrm, z = _random_inputs(rng, 9, 7)
    rgb[2, 3] = np.nan
    out = M.atrous(rgb, alb, nrm, z, iterations=0)
    assert np.array_equal(out, rgb, equal_nan=True)


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_model_with_every_sigma_off_is_a_dilated_b3_convolution(iterations):
    rng = np.random.default_rng(2)
    rgb, alb, nrm, z = _random_inputs(rng, 11, 13)
    for off in (0.0, -1.0, np.inf):
        out = M.atrous(rgb, alb, nrm, z, iterations=iterations, demodulate=0, sigma_color=off, sigma_normal=off, sigma_depth=off,
                       sigma_albedo=off)
        np.testing.assert_allclose(out, M.b3_convolution(rgb, iterations), rtol=1e-12, atol=0)


def test_model_keeps_a_signal_that_is_constant_after_demodulation():
    rng = np.random.default_rng(3)
    _, alb, nrm, z = _random_inputs(rng, 16, 12)
    alb[0, :] = 0.0  # below the floor: max(a, eps) applies
    for k in (0.25, 3.0):
        rgb = k * np.fmax(alb, M.EPS)
        for params in (dict(), dict(iterations=4, sigma_color=0.01, sigma_normal=0.05, sigma_depth=0.01, sigma_albedo=0.02),
                       dict(iterations=1, sigma_color=0.0)):
            out = M.atrous(rgb, alb, nrm, z, demodulate=1, **params)
            np.testing.assert_allclose(out, rgb, rtol=1e-12, atol=0)


def test_model_edges_and_non_finite_pixels():
    rng = np.random.default_rng(4)
    rgb, alb, nrm, z = _random_inputs(rng, 6, 6, miss=0.0)
    rgb[1, 1] = [np.nan, 0, 0]
    rgb[4, 4] = [np.inf, 1, 1]
    out = M.atrous(rgb, alb, nrm, z, iterations=1, demodulate=0)
    assert np.isfinite(out).all()
    assert (out[1, 1] == 0).all() and (out[4, 4] == 0).all()  # non-finite centre -> 0
    # a hit next to misses only: with the depth term on it keeps its own colour; with it off it is blended
    z2 = np.full((5, 5), np.inf)
    z2[2, 2] = 1.0
    c = rng.uniform(0.1, 1.0, (5, 5, 3))
    a, n = np.ones((5, 5, 3)), np.zeros((5, 5, 3))
    out = M.atrous(c, a, n, z2, iterations=1, demodulate=0, sigma_color=0, sigma_normal=0, sigma_albedo=0, sigma_depth=1.0)
    assert np.array_equal(out[2, 2], c[2, 2])
    out = M.atrous(c, a, n, z2, iterations=1, demodulate=0, sigma_color=0, sigma_normal=0, sigma_albedo=0, sigma_depth=0)
    assert not np.allclose(out[2, 2], c[2, 2])


def test_driver_rejects_a_bad_denoise_option():
    exe = build.build_host_example()
    main = os.path.join(os.path.dirname(exe), "pooraytracer_main")
    for bad in ("--denoise=0", "--denoise=11", "--denoise=x", "--denoise=3x", "--denoise="):
        r = subprocess.run([main, "nonexistent-scene-dir", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert "--denoise" in r.stderr, (bad, r.stderr)
