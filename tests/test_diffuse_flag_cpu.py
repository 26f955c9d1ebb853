"""The DIFFUSE form of the render kernel, as far as it can be said without a GPU (the frames are
tests/test_gpu_diffuse_kernel.py's): the flag of a material table that render_diffuse() decides with, on hand-built tables, and
the shipped library's answer to the sub-form query."""
import os
import subprocess

from pooraytracer_amd import _abi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every material an untextured Lambertian or an untextured emitter, none skipping light sampling; nothing scatters in an empty
# table or in a table of emitters only, so they qualify as well (such scenes never launch a PLAIN kernel to begin with, or end
# every path at its first hit)
EXPECTED = {
    "empty": 1, "emitters_only": 1, "lambertians_only": 1, "cornell": 1,
    "textured_lambertian": 0, "textured_emitter": 0, "mirror": 0, "phong_ns0": 0, "phong_ns20": 0, "cooktorrance": 0,
    "debug": 0, "empty_material": 0, "mirror_first": 0, "marked_skip": 0,
}


def test_scene_flag_on_hand_built_material_tables(tmp_path):
    """materials_all_diffuse (scene_setup.cpp) as a stand-alone program under ASan + UBSan (CPU only)."""
    exe = str(tmp_path / "diffuse_flag_check")
    csrc = os.path.join(ROOT, "pooraytracer_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g", "-std=c++17", "-ffp-contract=off"]
    subprocess.check_call(["g++"] + san + ["-I", csrc, os.path.join(ROOT, "tests", "cpp", "diffuse_flag_check.cpp"),
                                         os.path.join(csrc, "scene_setup.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:] + r.stdout.decode()
    got = {k: int(v) for k, v in (line.split() for line in r.stdout.decode().splitlines())}
    assert got == EXPECTED


def test_product_library_answers_unknown_to_the_sub_form_query(prt_lib):
    assert prt_lib.prt_dev_hooks() == 0
    assert api.last_render_subform(prt_lib) == _abi.RENDER_SUBFORM_UNKNOWN == 0
    assert api.last_render_form(prt_lib) == _abi.RENDER_FORM_UNKNOWN
    assert (_abi.RENDER_SUBFORM_NONE, _abi.RENDER_SUBFORM_DIFFUSE) == (1, 2)
    assert prt_lib.prt_abi_version() == _abi.PRT_ABI_VERSION == 6
