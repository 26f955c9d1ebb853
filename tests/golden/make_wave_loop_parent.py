"""Writes tests/golden/wave_loop_parent.npz (+ .txt): what tests/test_gpu_wave_loop.py compares against.  Run it on a GPU with
the libraries of the commit BEFORE the wave-loop change, from the repository root:

    python tests/golden/make_wave_loop_parent.py <libprt_hip.so of the parent> <libprt_hip_dev.so of the parent> <its hash>

Every frame is rendered by the shipped library and by the dev-hooks library at each threshold set of the test; the script
refuses to write a fixture if any two of them differ (the thresholds are schedule only), so one frame per case is stored;
the other instantiations (padded records, tables in global memory) and the ray batch get entries of their own.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from pooraytracer_amd import api  # noqa: E402
from tests import test_gpu_wave_loop as T  # noqa: E402


def main():
    lib, dev_lib, commit = sys.argv[1:4]
    api._LIB_PATH, api._DEV_LIB_PATH = os.path.abspath(lib), os.path.abspath(dev_lib)
    out = {}
    for perm in ("lean", "ct"):
        data = T.wave_loop_scene(perm)
        sc = api.Scene(data).upload(0)
        for key, kw in T.cases():
            out[f"{perm}_{key}_bits"], out[f"{perm}_{key}_counters"] = T.render_case(sc, kw)
        out[f"{perm}_counting_bits"], out[f"{perm}_counting_work"] = T.counting_case(sc)
        out[f"{perm}_rays_bits"], out[f"{perm}_rays_counters"] = T.ray_case(sc)
        sc.close()
        with api.dev_hooks():
            for name, setting in T.THRESHOLDS.items():
                for k in T.HOOKS:
                    os.environ.pop(f"PRT_TUNE_{k}", None)
                for k, v in setting.items():
                    os.environ[f"PRT_TUNE_{k}"] = str(v)
                sc = api.Scene(data).upload(0)
                for key, kw in T.cases():
                    bits, counters = T.render_case(sc, kw)
                    assert np.array_equal(bits, out[f"{perm}_{key}_bits"]), (perm, name, key)
                    assert np.array_equal(counters, out[f"{perm}_{key}_counters"]), (perm, name, key)
                sc.close()
            for name, setting in T.VARIANTS.items():  # the other instantiations: their own frames
                for k in T.HOOKS:
                    os.environ.pop(f"PRT_TUNE_{k}", None)
                for k, v in setting.items():
                    os.environ[f"PRT_TUNE_{k}"] = str(v)
                sc = api.Scene(data).upload(0)
                for key, kw in T.cases():
                    if key in T.VARIANT_CASES:
                        out[f"{perm}_{name}_{key}_bits"], out[f"{perm}_{name}_{key}_counters"] = T.render_case(sc, kw)
                print(perm, name, "variant", hex(T.variant(sc)))
                sc.close()
            for k in T.HOOKS:
                os.environ.pop(f"PRT_TUNE_{k}", None)
        print(perm, {k: out[f"{perm}_{k}_counters"].tolist() for k, _ in T.cases()}, out[f"{perm}_counting_work"].tolist())
    np.savez_compressed(T.GOLDEN, **out)
    with open(T.GOLDEN[:-4] + ".txt", "w") as f:
        f.write(f"wave_loop_parent.npz: rendered on an MI355X by commit {commit} (tests/golden/make_wave_loop_parent.py)\n")
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
