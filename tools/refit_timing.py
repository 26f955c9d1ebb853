"""Cost of moving geometry: prt_scene_refit / prt_scene_refit_device against prt_scene_update_vertices (the rebuild), the
tree's decay under deformation, and whether the refitted records are the host's bit for bit.  One GPU.

  python tools/refit_timing.py [--scenes cornell,bathroom2,soup1m,soup8m] [--runs 20] [--out profiles/refit_timing.json]

The driver starts one worker process per scene under its own `timeout` and stops at the first one that fails; what the
workers finished so far is still written.  Per scene the worker records
  update     medians over --runs calls after a warm-up (alternating between two vertex sets, the sinusoidal displacement
             at 1 % of the extent; emitters stay put), wall and hipEvent milliseconds, of refit_device (positions already
             on the device), refit (host positions) and update_vertices (the existing rebuild + reload: the yardstick);
             the refit's own split (records / boxes) from PrtRefitInfo
  decay      the same displacement at 1 %, 10 % and 50 %: sah_ratio after the refit, and the K3 frame time (512 x 512, spp 16,
             depth 10; soups: K1 Mrays/s on 2M random rays) on the refitted tree and on the tree update_vertices rebuilds
             from the same positions
  bit_equal  share of the centroid rays (tests/test_gpu_device_bvh.aimed_rays) whose t is bit-identical on the refitted
             scene and on a fresh scene, among rays that hit the same primitive
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
    "cornell": (lambda s: s.cornell_box(ball_subdiv=5, width=512, height=512), 240),
    "bathroom2": (lambda s: s.bathroom(512, 512), 420),
    "soup1m": (lambda s: s.triangle_soup(1_000_000), 420),
    "soup8m": (lambda s: s.triangle_soup(8_000_000), 1100),
}
FRAME = dict(spp=16, max_depth=10, seed=1)


def worker(name, runs):
    import copy

    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, build, scenes
    from tests.test_gpu_device_bvh import aimed_rays
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
    out = {"n_tris": data.n_tris, "runs": runs, "bvh": {k: sc.bvh_info()[k] for k in ("n_nodes", "depth", "tri_stride", "texture_bytes")}}

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
    ri = sc.refit_info()
    up["refit_device"].update(records_ms=ri["records_ms"], boxes_ms=ri["boxes_ms"])
    up["refit"] = timed(lambda i: sc.refit(sets[i % 2]), runs)
    up["update_vertices"] = timed(lambda i: sc.update_vertices(sets[i % 2]), max(3, runs if data.n_tris < 2_000_000 else runs // 4), warm=1)
    up["speedup_device_over_update_wall"] = up["update_vertices"]["wall_ms"] / up["refit_device"]["wall_ms"]
    out["update"] = up
    sc.close()

    lo, hi = data.bounds()
    rays = scenes.random_rays(2_000_000, lo, hi, seed=9) if soup else None
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda() if soup else None
    d_h = torch.zeros((rays.shape[0], 4), dtype=torch.float64, device="cuda") if soup else None

    def speed(s):
        vals = []
        for _ in range(3):
            if soup:
                s.trace_closest_device(d_r.data_ptr(), rays.shape[0], d_h.data_ptr())
                torch.cuda.synchronize()
                vals.append(rays.shape[0] / (s.counters()["kernel_ms"] * 1e3))  # Mrays/s
            else:
                s.render(**FRAME)
                vals.append(s.counters()["kernel_ms"])  # ms per frame
        return statistics.median(vals)

    decay = []
    for amount in (0.01, 0.1, 0.5):
        v = displaced(amount)
        s = api.Scene(data).upload(0)
        base = speed(s)
        s.refit(v)
        row = {"amount": amount, "sah_ratio": s.refit_info()["sah_ratio"], "start": base, "refit": speed(s)}
        s.update_vertices(v)
        row["rebuild"] = speed(s)
        row["unit"] = "Mrays/s" if soup else "ms/frame"
        decay.append(row)
        if amount == 0.1:  # bit-equality of the records, on the centroid rays
            s.close()
            s = api.Scene(data).upload(0)
            s.refit(v)
            new = copy.copy(data)
            new.vertices = v
            fresh = api.Scene(new).upload(0)
            ar, nc = aimed_rays(v, seed=2, max_tris=1)
            ar = ar[:min(nc, 1_000_000)]
            a, b = s.trace_closest(ar), fresh.trace_closest(ar)
            same = (a["prim"] == b["prim"]) & (a["prim"] >= 0)
            out["bit_equal"] = {"rays": int(ar.shape[0]), "same_prim": int(same.sum()),
                                "t_bit_identical_share": float((a["t"][same] == b["t"][same]).mean()),
                                "alpha_beta_bit_identical_share": float(((a["alpha"][same] == b["alpha"][same]) & (a["beta"][same] == b["beta"][same])).mean())}
            fresh.close()
        s.close()
    out["decay"] = decay
    print("REFIT_TIMING " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,bathroom2,soup1m,soup8m")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_timing.json"))
    ap.add_argument("--worker", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.runs)
    result = {"frame": FRAME, "scenes": {}}
    rc = 0
    for name in args.scenes.split(","):
        limit = SCENES[name][1]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", name, "--runs", str(args.runs)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("REFIT_TIMING ")]
        if r.returncode != 0 or not line:  # a failed GPU step ends the tool: nothing more is started on the device
            sys.stderr.write(f"[refit_timing] {name}: exit {r.returncode}\n{r.stderr[-2000:]}\n")
            rc = r.returncode or 1
            break
        result["scenes"][name] = json.loads(line[-1][len("REFIT_TIMING "):])
        print(f"[refit_timing] {name}: {json.dumps(result['scenes'][name]['update'])}", file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
