"""CPU-only checks of the refit interface (prt_scene_refit*, include/prt.h): PrtRefitInfo's size and layout against the
header, the new symbols, and the binding's argument validation, which raises before any call into the library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["refits", "records_ms", "boxes_ms", "sah_ratio", "grid_origin", "grid_step", "slab_scale", "host_stale"]


def test_refit_info_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    offs = ",".join(f"offsetof(PrtRefitInfo,{f})" for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "prt.h"\nint main(){printf("%zu' + " %zu" * len(FIELDS) +
                   '\\n",sizeof(PrtRefitInfo),' + offs + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert [f for f, _ in _abi.PrtRefitInfo._fields_] == FIELDS
    assert got == [C.sizeof(_abi.PrtRefitInfo)] + [getattr(_abi.PrtRefitInfo, f).offset for f in FIELDS]
    assert got[0] == 64


def test_refit_symbols_exported_and_declared(prt_lib):
    for name in ("prt_scene_refit", "prt_scene_refit_device", "prt_scene_refit_info"):
        assert name in _abi.EXPORTS and hasattr(prt_lib, name)
        assert getattr(prt_lib, name).argtypes is not None
    assert prt_lib.prt_scene_refit_device.argtypes == [C.c_void_p] * 4


def test_refit_info_before_any_refit(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    info = sc.refit_info()
    assert info["refits"] == 0 and info["sah_ratio"] == 1.0 and info["host_stale"] == 0
    assert info["records_ms"] == 0.0 and info["boxes_ms"] == 0.0
    assert len(info["grid_origin"]) == 3 and all(s > 0 for s in info["grid_step"])
    sc.close()


def test_refit_validates_arguments_before_any_call(prt_lib):
    """Shape and dtype errors are Python exceptions of the binding; only well-formed arguments reach the library, where a
    scene that is not uploaded answers PRT_E_NO_DEVICE."""
    data = scenes.tiny_scene()
    sc = api.Scene(data)
    v = data.vertices.copy()
    for bad in (v[:-1], v.reshape(-1, 9), v[:, :, :2]):
        with pytest.raises(ValueError):
            sc.refit(bad)
        with pytest.raises(ValueError):
            sc.refit(v, normals=bad)
    for bad in (v.astype(np.float32), v.astype(np.int64)):
        with pytest.raises(TypeError):
            sc.refit(bad)
        with pytest.raises(TypeError):
            sc.refit(v, normals=bad)
    with pytest.raises(TypeError):
        sc.refit(v.tolist())
    for bad in (v, "0x1000", 1.5, True):
        with pytest.raises(TypeError):
            sc.refit_device(bad)
    with pytest.raises(TypeError):
        sc.refit_device(4096, d_normals_ptr=v)
    with pytest.raises(TypeError):
        sc.refit_device(4096, stream="s")
    for null in (None, 0):
        with pytest.raises(ValueError):
            sc.refit_device(null)
    # well-formed arguments reach the library
    for call in (lambda: sc.refit(v), lambda: sc.refit(v[::1], normals=np.zeros_like(v)), lambda: sc.refit_device(4096)):
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_NO_DEVICE
    assert sc.refit_info()["refits"] == 0
    sc.close()
