"""CPU-only checks of the device-rebuild interface (prt_scene_rebuild*, include/prt.h): the two symbols are declared,
listed and exported, the ABI version and PrtRefitInfo are untouched, the refusals that need no device, and the binding's
argument validation, which raises before any call into the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prt_scene_rebuild", "prt_scene_rebuild_device")


def test_rebuild_symbols_declared_listed_and_exported(prt_lib):
    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(PrtScene\* scene, " % name, header, re.M), f"{name} is not declared in prt.h"
        assert name in _abi.EXPORTS and hasattr(prt_lib, name)
        assert getattr(prt_lib, name).argtypes is not None
    assert prt_lib.prt_scene_rebuild.argtypes == [C.c_void_p] * 3
    assert prt_lib.prt_scene_rebuild_device.argtypes == [C.c_void_p] * 4


def test_abi_version_is_still_6(prt_lib):
    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    assert re.search(r"#define\s+PRT_ABI_VERSION\s+6\b", header)
    assert prt_lib.prt_abi_version() == 6
    assert C.sizeof(_abi.PrtRefitInfo) == 64  # no existing struct changed


def test_null_scene_is_invalid(prt_lib):
    v = np.zeros((1, 3, 3))
    assert prt_lib.prt_scene_rebuild(None, v.ctypes.data, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_rebuild_device(None, 4096, None, None) == _abi.PRT_E_INVALID


def test_a_scene_that_is_not_uploaded_is_no_device(prt_lib):
    data = scenes.tiny_scene()
    sc = api.Scene(data)
    v = data.vertices.copy()
    for call, name in ((lambda: sc.rebuild(v), "prt_scene_rebuild"), (lambda: sc.rebuild(v, normals=np.zeros_like(v)), "prt_scene_rebuild"),
                       (lambda: sc.rebuild_device(4096), "prt_scene_rebuild_device")):
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_NO_DEVICE
        assert re.search(r"\b%s\b:" % name, str(e.value)), str(e.value)
    info = sc.refit_info()
    assert info["refits"] == 0 and info["host_stale"] == 0
    sc.close()


def test_rebuild_validates_arguments_before_any_call(prt_lib):
    """Shape and dtype errors are Python exceptions of the binding, as for refit / refit_device."""
    data = scenes.tiny_scene()
    sc = api.Scene(data)
    v = data.vertices.copy()
    for bad in (v[:-1], v.reshape(-1, 9), v[:, :, :2]):
        with pytest.raises(ValueError):
            sc.rebuild(bad)
        with pytest.raises(ValueError):
            sc.rebuild(v, normals=bad)
    for bad in (v.astype(np.float32), v.astype(np.int64)):
        with pytest.raises(TypeError):
            sc.rebuild(bad)
        with pytest.raises(TypeError):
            sc.rebuild(v, normals=bad)
    with pytest.raises(TypeError):
        sc.rebuild(v.tolist())
    for bad in (v, "0x1000", 1.5, True):
        with pytest.raises(TypeError):
            sc.rebuild_device(bad)
    with pytest.raises(TypeError):
        sc.rebuild_device(4096, d_normals_ptr=v)
    with pytest.raises(TypeError):
        sc.rebuild_device(4096, stream="s")
    for null in (None, 0):
        with pytest.raises(ValueError):
            sc.rebuild_device(null)
    sc.close()
