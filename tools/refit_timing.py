"""Cost of moving geometry: prt_scene_refit / prt_scene_refit_device against prt_scene_update_vertices (the rebuild), the
tree's decay under deformation, and whether the refitted records are the host's bit for bit.  One GPU.

  python tools/refit_timing.py [--scenes cornell,bathroom2,soup1m,soup8m] [--runs 20] [--out profiles/refit_timing.json]

Every scene is one child process under its own `timeout`; the first child that fails ends the run, and what it had printed
(one JSON line per figure, tools/timing_common.py) is still written.  Per scene the child records
  update     medians over --runs calls after a warm-up (alternating between two vertex sets, the sinusoidal displacement
             of timing_common.wobble at 1 % of the extent; emitters stay put), wall and hipEvent milliseconds, of
             refit_device (positions already on the device), refit (host positions) and update_vertices (the existing
             rebuild + reload: the yardstick); the refit's own split (records / boxes) from PrtRefitInfo
  decay      the same displacement at 1 %, 10 % and 50 %: sah_ratio after the refit, and the K3 frame time (512 x 512, spp 16,
             depth 10; soups: K1 Mrays/s on 2M random rays) on the refitted tree and on the tree update_vertices rebuilds
             from the same positions
  bit_equal  share of the centroid rays (tests/test_gpu_device_bvh.aimed_rays) whose t is bit-identical on the refitted
             scene and on a fresh scene, among rays that hit the same primitive
"""
import argparse
import functools
import os
import statistics
import sys

import timing_common as tc

SCENES = ("cornell", "bathroom2", "soup1m", "soup8m")
GROUPS = {"update": "update"}
FRAME = dict(spp=16, max_depth=10, seed=1)


def child(name, runs):
    import copy

    import numpy as np
    import torch
    from pooraytracer_amd import api, build, scenes
    from tests.test_gpu_device_bvh import aimed_rays
    build.build()
    soup = name.startswith("soup")
    data, _ = tc.load(name, **({} if soup else {"width": 512, "height": 512}))
    mask = ~tc.emitter_mask(data)
    sets = [tc.wobble(data.vertices, mask), data.vertices.copy()]
    d_sets = [torch.from_numpy(v).cuda() for v in sets]
    sc = api.Scene(data).upload(0)
    tc.emit(n_tris=data.n_tris, runs=runs, bvh={k: sc.bvh_info()[k] for k in ("n_nodes", "depth", "tri_stride", "texture_bytes")})

    update = functools.partial(tc.emit_timed, "refit_timing " + name, "update", calls=False)
    fast = update("refit_device", lambda i: sc.refit_device(d_sets[i % 2].data_ptr()), runs,
                  more=lambda: {k: sc.refit_info()[k] for k in ("records_ms", "boxes_ms")})
    update("refit", lambda i: sc.refit(sets[i % 2]), runs)
    slow = update("update_vertices", lambda i: sc.update_vertices(sets[i % 2]), max(3, runs if data.n_tris < 2_000_000 else runs // 4), warm=1)
    tc.emit(update="speedup_device_over_update_wall", result=slow["wall_ms"] / fast["wall_ms"])
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
        v = tc.wobble(data.vertices, mask, amount)
        s = api.Scene(data).upload(0)
        base = speed(s)
        s.refit(v)
        row = {"amount": amount, "sah_ratio": s.refit_info()["sah_ratio"], "start": base, "refit": speed(s)}
        s.update_vertices(v)
        row["rebuild"] = speed(s)
        row["unit"] = "Mrays/s" if soup else "ms/frame"
        decay.append(row)
        tc.emit(decay=decay)  # the list so far: the last line holds all of it
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
            tc.emit(bit_equal={"rays": int(ar.shape[0]), "same_prim": int(same.sum()),
                               "t_bit_identical_share": float((a["t"][same] == b["t"][same]).mean()),
                               "alpha_beta_bit_identical_share": float(((a["alpha"][same] == b["alpha"][same]) & (a["beta"][same] == b["beta"][same])).mean())})
            fresh.close()
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    tc.common_args(ap, launches=False, runs=20, out=os.path.join(tc.ROOT, "profiles", "refit_timing.json"), worker=True)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs)
    names = tc.scene_names(ap, args.scenes, SCENES)
    out = {"frame": FRAME, **tc.run_children(__file__, names, tc.flags(args, "runs"), None, GROUPS)}
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
