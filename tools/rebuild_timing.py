"""Cost of a new tree for moving geometry: prt_scene_rebuild_device / prt_scene_rebuild (the device-side rebuild of a
resident scene) against prt_scene_update_vertices (host positions, rebuild + re-upload of every table) and against
prt_scene_refit_device (no new tree), on the same motion; and what each tree is worth afterwards.  One GPU.

  python tools/rebuild_timing.py [--scenes cornell,bathroom2,soup1m] [--runs 10] [--out profiles/rebuild_timing.json]

The driver starts one worker process per scene under its own `timeout` and stops at the first one that fails; what the
workers finished so far is still written.  Per scene the worker records
  update     medians over --runs calls after a warm-up (alternating between two vertex sets, the sinusoidal displacement
             at 1 % of the extent; emitters stay put), wall and hipEvent milliseconds, of rebuild_device (positions
             already on the device), rebuild (host positions), update_vertices (the yardstick) and refit_device; the
             builder's own time (PrtBvhInfo.build_ms) of the last rebuild_device
  trees      (the soup) K1 Mrays/s on 2M random rays after a 50 % sinusoidal displacement on three trees of the same
             positions: the refitted one (with its sah_ratio), the rebuilt one and update_vertices' one
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

SCENES = {  # name -> (factory, seconds the worker may take)
    "cornell": (lambda s: s.cornell_box(ball_subdiv=5, width=512, height=512), 180),
    "bathroom2": (lambda s: s.bathroom(512, 512), 300),
    "soup1m": (lambda s: s.triangle_soup(1_000_000), 420),
}


def worker(name, runs):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, build, scenes
    build.build()
    data = SCENES[name][0](scenes)
    soup = name.startswith("soup")
    mask = np.ones(data.n_tris, dtype=bool)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = False
    p = data.vertices[mask].reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())

    def displaced(amount):
        v = data.vertices.copy()
        w = data.vertices[mask]
        v[mask] = w + amount * ext * np.sin(7.0 / ext * w[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3]))
        return v

    sets = [displaced(0.01), data.vertices.copy()]
    d_sets = [torch.from_numpy(v).cuda() for v in sets]
    sc = api.Scene(data).upload(0)
    info = sc.bvh_info()
    out = {"n_tris": data.n_tris, "runs": runs, "bvh": {k: info[k] for k in ("n_nodes", "depth", "tri_stride", "texture_bytes")}}

    def timed(fn, n, warm=2):
        wall, evt = [], []
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
        return {"wall_ms": statistics.median(wall), "event_ms": statistics.median(evt), "wall_min_ms": min(wall), "wall_max_ms": max(wall)}

    up = {}
    up["refit_device"] = timed(lambda i: sc.refit_device(d_sets[i % 2].data_ptr()), runs)
    up["rebuild_device"] = timed(lambda i: sc.rebuild_device(d_sets[i % 2].data_ptr()), runs)
    after = sc.bvh_info()
    up["rebuild_device"].update(build_ms=after["build_ms"], sort_ms=after["sort_ms"], tree_ms=after["tree_ms"], split_ms=after["split_ms"],
                                n_nodes=after["n_nodes"])
    up["rebuild"] = timed(lambda i: sc.rebuild(sets[i % 2]), runs)
    up["update_vertices"] = timed(lambda i: sc.update_vertices(sets[i % 2]), max(3, runs // 2), warm=1)
    up["speedup_rebuild_device_over_update_wall"] = up["update_vertices"]["wall_ms"] / up["rebuild_device"]["wall_ms"]
    up["speedup_rebuild_over_update_wall"] = up["update_vertices"]["wall_ms"] / up["rebuild"]["wall_ms"]
    out["update"] = up
    sc.close()

    if soup:
        lo, hi = data.bounds()
        rays = scenes.random_rays(2_000_000, lo, hi, seed=9)
        d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
        d_h = torch.zeros((rays.shape[0], 4), dtype=torch.float64, device="cuda")

        def speed(s):
            vals = []
            for _ in range(3):
                s.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr())
                torch.cuda.synchronize()
                vals.append(rays.shape[0] / (s.counters()["kernel_ms"] * 1e3))  # Mrays/s
            return statistics.median(vals)

        v = displaced(0.5)
        d_v = torch.from_numpy(v).cuda()
        s = api.Scene(data).upload(0)
        row = {"amount": 0.5, "unit": "Mrays/s", "start": speed(s)}
        s.refit_device(d_v.data_ptr())
        row["sah_ratio_refitted"] = s.refit_info()["sah_ratio"]
        row["refitted"] = speed(s)
        s.rebuild_device(d_v.data_ptr())
        row["rebuilt"] = speed(s)
        s.update_vertices(v)
        row["update_vertices"] = speed(s)
        s.close()
        out["trees"] = row
    print("REBUILD_TIMING " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,bathroom2,soup1m")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_timing.json"))
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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("REBUILD_TIMING ")]
        if r.returncode != 0 or not line:  # a failed GPU step ends the tool: nothing more is started on the device
            sys.stderr.write(f"[rebuild_timing] {name}: exit {r.returncode}\n{r.stderr[-2000:]}\n")
            rc = r.returncode or 1
            break
        result["scenes"][name] = json.loads(line[-1][len("REBUILD_TIMING "):])
        print(f"[rebuild_timing] {name}: {json.dumps(result['scenes'][name]['update'])}", file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
