"""In-tree build of libprt_hip.so (hipcc, gfx950 only).  hipcc cross-compiles without a GPU.

Every source is compiled to its own object (in parallel, only when it or a header changed) and the objects are linked into
  libprt_hip.so      the product: reads NO developer environment variable (PRT_DEV_HOOKS 0);
  libprt_hip_dev.so  the same objects except prt_api.o, which is compiled with -DPRT_DEV_HOOKS=1: the PRT_TUNE_* / PRT_TEST_*
                     / PRT_VALIDATE_BVH hooks exist only there (failure-injection tests, sweep tools: api.dev_hooks()).
                     PRT_TEST_DUMP_BVH=<file> writes each scene's traversal tree (header, nodes, leaf order) when it is
                     built: host trees at create and on a host rebuild, device trees at upload, either after a refit
                     or a device rebuild of the resident scene (tests/bvh_model.py reads it).
build_probe() builds tests/probe/libprt_probe.so, the test-only wrappers of prt_device.h's primitives — a library of its
own, linked into neither of the two above.
"""
import concurrent.futures
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libprt_hip.so")
DEV_LIB = os.path.join(HERE, "libprt_hip_dev.so")
OBJ = os.path.join(HERE, "_obj")
SOURCES = ["prt_api.cpp", "prt_kernels.hip", "prt_kernels_f32.hip", "bvh_build.cpp", "bvh_build_gpu.hip", "bvh_refit.hip", "light_tables.hip", "ray_sort.hip", "scene_setup.cpp", "prt_denoise.hip", "closest_point.hip", "pseudonormals.hip", "winding_number.hip", "mesh_topology.cpp", "multi_hit.hip", "multi_hit_f32.hip"]
HEADERS = ["prt_types.h", "prt_device.h", "prt_light_pick.h", "prt_wave.h", "prt_vec64.h", "prt_host.h", "prt_launch.h", "mesh_topology.h", os.path.join("..", "..", "include", "prt.h")]
PROBE_HEADERS = ["prt_types.h", "prt_device.h", "prt_light_pick.h", "prt_wave.h", "prt_host.h"]  # what tests/probe/*.hip can reach
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CFLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function", "-fno-gpu-rdc"]
DEV_FLAGS = ["-DPRT_DEV_HOOKS=1"]
JOBS = max(1, min(6, (os.cpu_count() or 2)))


INCLUDES = {"prt_kernels_f32.hip": ["prt_kernels.hip"], "multi_hit_f32.hip": ["multi_hit.hip"]}  # sources that #include another source


def _deps(src):
    return [os.path.join(CSRC, f) for f in [src] + INCLUDES.get(src, []) + HEADERS] + [os.path.abspath(__file__)]


def _obj_path(src, flags):
    tag = hashlib.sha1(" ".join(flags).encode()).hexdigest()[:10] if flags else "std"
    return os.path.join(OBJ, tag, src + ".o")


def _compile(src, flags, force, verbose):
    out = _obj_path(src, flags)
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in _deps(src)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [HIPCC, "-c"] + CFLAGS + list(flags) + ["-o", out, os.path.join(CSRC, src)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def _link(objs, out, verbose):
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(o) for o in objs):
        return out
    cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-o", out] + objs + ["-lrccl"]  # RCCL: prt_render_multi's reduce
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def stale():
    return not os.path.exists(LIB) or not os.path.exists(DEV_LIB) or any(
        os.path.getmtime(d) > min(os.path.getmtime(LIB), os.path.getmtime(DEV_LIB)) for src in SOURCES for d in _deps(src))


def build(force=False, verbose=False, extra_flags=(), out=None):
    """Compile every HIP/C++ source of the hot path into pooraytracer_amd/libprt_hip.so (+ libprt_hip_dev.so).
    With `extra_flags` / `out`: ONE library of that configuration at `out` (A/B builds of the tools)."""
    extra = list(extra_flags)
    jobs = [(src, extra) for src in SOURCES]
    if not extra and out is None:
        if not force and not stale():
            return LIB
        jobs.append(("prt_api.cpp", DEV_FLAGS))
    with concurrent.futures.ThreadPoolExecutor(JOBS) as ex:
        objs = list(ex.map(lambda j: _compile(j[0], j[1], force, verbose), jobs))
    if extra or out is not None:
        return _link(objs[:len(SOURCES)], out or LIB, verbose)
    _link(objs[:len(SOURCES)], LIB, verbose)
    _link([objs[-1]] + objs[1:len(SOURCES)], DEV_LIB, verbose)
    return LIB


PROBE_DIR = os.path.join(os.path.dirname(HERE), "tests", "probe")
PROBE_LIB = os.path.join(PROBE_DIR, "libprt_probe.so")
PROBE_SOURCES = ["prt_probe.hip", "prt_probe_f32.hip"]


def build_probe(force=False, verbose=False):
    """tests/probe/libprt_probe.so: the TEST-ONLY element-wise wrappers of prt_device.h's primitives (fp64 + fp32 twin).
    Same flags as the product, same freshness rule on the headers; linked on its own, never into the product libraries."""
    lib = PROBE_LIB
    deps = [os.path.join(PROBE_DIR, s) for s in PROBE_SOURCES] + [os.path.join(CSRC, h) for h in PROBE_HEADERS] + [os.path.abspath(__file__)]
    if not force and os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in deps):
        return lib
    cmd = [HIPCC, "-shared"] + CFLAGS + ["-o", lib] + [os.path.join(PROBE_DIR, s) for s in PROBE_SOURCES]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return lib


HOST_LIB = os.path.join(HERE, "libpooraytracer_host.so")
HOST_EXE = os.path.join(HERE, "render_scene")
MAIN_EXE = os.path.join(HERE, "pooraytracer_main")
ROOT = os.path.dirname(HERE)


def build_host_example(force=False):
    """g++ build of the C++ host API (include/pooraytracer/*.h over the C ABI) and the main.cpp-style driver."""
    srcs = [os.path.join(HERE, "host", f) for f in ("host_api.cpp", "model.cpp", "png_decode.cpp", "jpeg_decode.cpp")]
    exe_src = os.path.join(ROOT, "examples", "render_scene.cpp")
    main_src = os.path.join(ROOT, "examples", "pooraytracer_main.cpp")
    inc = os.path.join(ROOT, "include")
    deps = srcs + [exe_src, main_src, os.path.join(inc, "prt.h")] + [os.path.join(inc, "pooraytracer", f) for f in os.listdir(os.path.join(inc, "pooraytracer"))]
    fresh = all(os.path.exists(x) and os.path.getmtime(x) >= max(os.path.getmtime(d) for d in deps) for x in (HOST_LIB, HOST_EXE, MAIN_EXE))
    if fresh and not force:
        return HOST_EXE
    build()
    common = ["-O2", "-std=c++17", "-Wall", "-pthread", "-I", inc, "-L", HERE, "-Wl,-rpath,$ORIGIN"]
    subprocess.check_call(["g++", "-shared", "-fPIC"] + common + ["-o", HOST_LIB] + srcs + ["-lprt_hip"])
    subprocess.check_call(["g++"] + common + ["-o", HOST_EXE, exe_src, "-lpooraytracer_host", "-lprt_hip"])
    subprocess.check_call(["g++"] + common + ["-o", MAIN_EXE, main_src, "-lpooraytracer_host", "-lprt_hip"])
    return HOST_EXE


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True,
          extra_flags=["-Rpass-analysis=kernel-resource-usage"] if "--resources" in sys.argv else [])
    print(LIB)
