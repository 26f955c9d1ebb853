"""CPU-only checks of the moving-emitter interface (prt_scene_set_dynamic_lights and its companions, include/prt.h): the
symbols are declared, listed and exported, PrtLightUpdateInfo's size and offsets are the header's, the switch round-trips on
a scene that is not uploaded, null arguments are refused, and the calls that need a device say so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from pooraytracer_amd import _abi, api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("prt_scene_set_dynamic_lights", "prt_scene_get_dynamic_lights", "prt_scene_light_update_info", "prt_scene_light_table_words")
FIELDS = ["updates", "gather_ms", "host_tree_ms", "tables_ms", "n_tables", "table_words", "tables_dropped", "relaid"]


def test_symbols_declared_listed_and_exported(prt_lib):
    header = open(os.path.join(ROOT, "include", "prt.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\((const )?PrtScene\* scene, " % name, header, re.M), f"{name} is not declared in prt.h"
        assert name in _abi.EXPORTS and hasattr(prt_lib, name)
        assert getattr(prt_lib, name).argtypes is not None
    assert re.search(r"#define\s+PRT_ABI_VERSION\s+6\b", header) and prt_lib.prt_abi_version() == 6


def test_light_update_info_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    offs = ",".join(f"offsetof(PrtLightUpdateInfo,{f})" for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "prt.h"\nint main(){printf("%zu' + " %zu" * len(FIELDS) +
                   '\\n",sizeof(PrtLightUpdateInfo),' + offs + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert [f for f, _ in _abi.PrtLightUpdateInfo._fields_] == FIELDS
    assert got == [C.sizeof(_abi.PrtLightUpdateInfo)] + [getattr(_abi.PrtLightUpdateInfo, f).offset for f in FIELDS]
    assert got[0] == 48
    assert C.sizeof(_abi.PrtRefitInfo) == 64  # no existing struct changed


def test_switch_round_trips_without_an_upload(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    assert sc.dynamic_lights is False
    sc.dynamic_lights = True
    assert sc.dynamic_lights is True
    sc.update_vertices(sc.data.vertices.copy())  # the switch survives new host positions
    assert sc.dynamic_lights is True
    sc.dynamic_lights = False
    assert sc.dynamic_lights is False
    info = sc.light_update_info()
    assert info["updates"] == 0 and info["tables_dropped"] == 0 and info["relaid"] == 0
    assert info["gather_ms"] == 0.0 and info["host_tree_ms"] == 0.0 and info["tables_ms"] == 0.0
    sc.close()


def test_null_arguments_are_invalid(prt_lib):
    sc = api.Scene(scenes.tiny_scene())
    on, n = C.c_int(0), C.c_uint64(0)
    info = _abi.PrtLightUpdateInfo()
    assert prt_lib.prt_scene_set_dynamic_lights(None, 1) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_get_dynamic_lights(None, C.byref(on)) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_get_dynamic_lights(sc._h, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_light_update_info(None, C.byref(info)) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_light_update_info(sc._h, None) == _abi.PRT_E_INVALID
    assert prt_lib.prt_scene_light_table_words(None, None, 0, C.byref(n)) == _abi.PRT_E_INVALID
    sc.close()


def test_table_plan_is_the_host_builders_layout_under_sanitizers(tmp_path):
    """The host half of a light update, as a stand-alone program under ASan + UBSan (CPU only): the plan of a tree built
    without tables is the layout the full host build gives the same geometry (top nodes, root, headers, word count), the
    planned top part with the host's words picks what the full tree picks, and the listed Triangle precompute equals the
    full one — over lights lists with odd counts, a collapsed mesh and all-degenerate lists."""
    exe = str(tmp_path / "light_plan_san")
    csrc = os.path.join(ROOT, "pooraytracer_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g", "-std=c++17", "-ffp-contract=off"]
    subprocess.check_call(["g++"] + san + ["-I", csrc, os.path.join(ROOT, "tests", "cpp", "light_plan_sanitize.cpp"),
                                         os.path.join(csrc, "scene_setup.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:] + r.stdout.decode()
    assert r.stdout.decode().count(" ok") == 12


def test_calls_that_need_a_device_say_so(prt_lib):
    """With the switch on, a refit or a rebuild of a scene that is not uploaded is still PRT_E_NO_DEVICE, and so is the
    read-back of the table words."""
    data = scenes.tiny_scene()
    sc = api.Scene(data)
    sc.dynamic_lights = True
    v = data.vertices + 0.25
    for call in (lambda: sc.refit(v), lambda: sc.refit_device(4096), lambda: sc.rebuild(v), lambda: sc.rebuild_device(4096),
                 lambda: sc.light_table_words()):
        with pytest.raises(api.PrtError) as e:
            call()
        assert e.value.code == _abi.PRT_E_NO_DEVICE
    assert sc.light_update_info()["updates"] == 0 and sc.refit_info()["refits"] == 0
    sc.close()
