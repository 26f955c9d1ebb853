"""Progressive rendering (prt_accum_*, include/prt.h) without a GPU: the ABI surface, the error a scene that is not uploaded
gives, and the argument checks of api.Accumulator that run before the library is called."""
import ctypes as C
import os
import re

import pytest

from pooraytracer_amd import _abi, api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCUM = ["prt_accum_create", "prt_accum_destroy", "prt_accum_render", "prt_accum_samples", "prt_accum_reset",
         "prt_accum_resolve", "prt_accum_read", "prt_accum_export", "prt_accum_import"]


def test_accum_symbols_declared_and_exported(prt_lib):
    hdr = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z0-9_]+)\s*\(", hdr))
    for name in ACCUM:
        assert name in declared, name
        assert name in _abi.EXPORTS, name
        assert hasattr(prt_lib, name), f"{name} not exported by libprt_hip.so"
    assert "typedef struct PrtAccum PrtAccum;" in hdr


def test_abi_version_is_6(prt_lib):
    assert _abi.PRT_ABI_VERSION == 6
    assert prt_lib.prt_abi_version() == 6
    assert re.search(r"#define PRT_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "prt.h")).read())


def test_accum_create_needs_an_uploaded_scene(prt_lib):
    sc = api.Scene(scenes.tiny_scene())  # host-side preparation only: never uploaded
    with pytest.raises(api.PrtError) as e:
        api.Accumulator(sc)
    assert e.value.code == _abi.PRT_E_NO_DEVICE
    # the C entry point leaves *out NULL on failure
    c, p = _abi.make_camera(sc.data.camera), _abi.make_params()
    h = C.c_void_p(12345)
    assert prt_lib.prt_accum_create(sc._h, C.byref(c), C.byref(p), C.byref(h)) == _abi.PRT_E_NO_DEVICE
    assert not h.value
    sc.close()


def test_accum_null_handles(prt_lib):
    n = C.c_uint64(0)
    assert prt_lib.prt_accum_render(None, 1, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_samples(None, C.byref(n)) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_reset(None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_resolve(None, None, None, None, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_read(None, None, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_export(None, None, C.byref(n), C.byref(n)) == _abi.PRT_E_INVALID
    assert prt_lib.prt_accum_import(None, None, 0, 0) == _abi.PRT_E_INVALID
    prt_lib.prt_accum_destroy(None)  # no-op


def test_accumulator_rejects_spp(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    with pytest.raises(TypeError):
        api.Accumulator(sc, spp=4)
    sc.close()


def _unopened(shape):
    """An Accumulator object without a library handle: the Python-side checks run before any call into the library."""
    acc = api.Accumulator.__new__(api.Accumulator)
    acc._L, acc._h, acc._shape = api.load(), None, shape
    return acc


@pytest.mark.parametrize("n", [0, -3, 1.5])
def test_accumulator_add_checks_n(prt_lib, n):
    with pytest.raises(ValueError):
        _unopened((4, 5, 3)).add(n)


def test_accumulator_restore_checks_shape_and_samples(prt_lib):
    import numpy as np
    acc = _unopened((4, 5, 3))
    with pytest.raises(ValueError):
        acc.restore(np.zeros((5, 4, 3)), 1, 0)
    with pytest.raises(ValueError):
        acc.restore(np.zeros(60), 1, 0)
    with pytest.raises(ValueError):
        acc.restore(np.zeros((4, 5, 3)), -1, 0)
