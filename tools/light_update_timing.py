"""Cost of moving an emitter: prt_scene_refit_device with prt_scene_set_dynamic_lights on (the light tree, its records and
its O(1) tables follow on the device) against prt_scene_update_vertices (the only way to move a light without the switch:
host positions, every table re-sent, the light tables built on the host), on the same motion.  One GPU.

  python tools/light_update_timing.py [--scenes veach-mis,cornell,sphere100k] [--runs 20] [--out profiles/light_update_timing.json]

The driver starts one worker process per scene under its own `timeout` and stops at the first one that fails; what the
workers finished so far is still written.  Per scene the worker alternates between two vertex sets (the start, and every
emitter vertex displaced sinusoidally by 1 % of the emitters' extent) and records medians over --runs calls after a warm-up,
wall and hipEvent milliseconds, of
  refit_device_lights   refit_device with the switch on and the emitters moving, with the medians of its
                        gather_ms / host_tree_ms / tables_ms split (PrtLightUpdateInfo)
  refit_device_still    refit_device with the switch on and the same positions as resident (emitters still; the read-back
                        carries the emitters' vertices) and with the switch off (the call as it was before the switch existed)
  update_vertices       the yardstick, on the same motion
There is no pass threshold: the numbers are quoted in DESIGN.md §7 and the README.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sphere_in_a_box(s):
    """A synthetic emissive icosphere of 81,920 triangles (subdivision 6: the nearest icosphere to 100k) in a closed box."""
    from pooraytracer_amd import _abi
    b = s._Builder("sphere100k")
    white = b.material(s.Material("white", _abi.MAT_LAMBERTIAN, kd=(0.7, 0.7, 0.7)))
    light = b.material(s.Material("Light", _abi.MAT_DIFFUSE_LIGHT, emission=(8.0, 8.0, 8.0)))
    b.mesh("box", white, *s.box((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)))
    v, uv, n = s.icosphere(6, radius=0.6, center=(0.0, 0.3, 0.0))
    b.mesh("lamp", light, v, uv, n)
    return b.build(s.Camera(256, 256, 60.0, eye=(0.0, 0.0, 1.9), look_at=(0.0, 0.0, 0.0)))


SCENES = {  # name -> (factory, seconds the worker may take)
    "veach-mis": (lambda s: s.veach_mis(256, 144), 240),
    "cornell": (lambda s: s.cornell_box(ball_subdiv=5, width=256, height=256), 180),
    "sphere100k": (sphere_in_a_box, 420),
}


def worker(name, runs):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, build, scenes
    build.build()
    data = SCENES[name][0](scenes)
    mask = np.zeros(data.n_tris, dtype=bool)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = True
    p = data.vertices[mask].reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    moved = data.vertices.copy()
    w = data.vertices[mask]
    moved[mask] = w + 0.01 * ext * np.sin(7.0 / ext * w[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3]))
    sets = [moved, data.vertices.copy()]
    d_sets = [torch.from_numpy(v).cuda() for v in sets]
    d_n = torch.from_numpy(np.ascontiguousarray(data.normals)).cuda()
    sc = api.Scene(data).upload(0)
    sc.dynamic_lights = True
    out = {"n_tris": data.n_tris, "emitter_tris": int(mask.sum()), "runs": runs}

    def timed(fn, n, warm=2, after=None):
        wall, evt, extra = [], [], []
        for i in range(warm + n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn(i)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warm:
                wall.append(1e3 * (t1 - t0))
                evt.append(e0.elapsed_time(e1))
                if after:
                    extra.append(after())
        row = {"calls": n, "wall_ms": statistics.median(wall), "event_ms": statistics.median(evt), "wall_min_ms": min(wall), "wall_max_ms": max(wall)}
        if extra:
            for k in extra[0]:
                row[k] = statistics.median(e[k] for e in extra)
        return row

    def split():
        lu = sc.light_update_info()
        return {k: lu[k] for k in ("gather_ms", "host_tree_ms", "tables_ms")}

    up = {}
    up["refit_device_lights"] = timed(lambda i: sc.refit_device(d_sets[i % 2].data_ptr(), d_n.data_ptr()), runs, after=split)
    lu = sc.light_update_info()
    assert lu["updates"] == runs + 2 and lu["tables_dropped"] == 0, lu
    out["tables"] = {k: lu[k] for k in ("n_tables", "table_words", "relaid")}
    resident = d_sets[(runs + 1) % 2]
    up["refit_device_still"] = timed(lambda i: sc.refit_device(resident.data_ptr(), d_n.data_ptr()), runs)
    assert sc.light_update_info()["updates"] == runs + 2
    sc.dynamic_lights = False
    up["refit_device_still_switch_off"] = timed(lambda i: sc.refit_device(resident.data_ptr(), d_n.data_ptr()), runs)
    up["update_vertices"] = timed(lambda i: sc.update_vertices(sets[i % 2], normals=data.normals), runs, warm=1)
    up["speedup_over_update_vertices_wall"] = up["update_vertices"]["wall_ms"] / up["refit_device_lights"]["wall_ms"]
    out["update"] = up
    sc.close()
    print("LIGHT_UPDATE_TIMING " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="veach-mis,cornell,sphere100k")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_update_timing.json"))
    ap.add_argument("--worker", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.runs)
    result = {"scenes": {}}
    rc = 0
    for name in args.scenes.split(","):
        limit = SCENES[name][1]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--runs", str(args.runs)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LIGHT_UPDATE_TIMING ")]
        if r.returncode != 0 or not line:  # a failed GPU step ends the tool: nothing more is started on the device
            sys.stderr.write(f"[light_update_timing] {name}: exit {r.returncode}\n{r.stderr[-2000:]}\n")
            rc = r.returncode or 1
            break
        result["scenes"][name] = json.loads(line[-1][len("LIGHT_UPDATE_TIMING "):])
        print(f"[light_update_timing] {name}: {json.dumps(result['scenes'][name]['update'])}", file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
