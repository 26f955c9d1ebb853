"""Cost of a new tree for moving geometry: prt_scene_rebuild_device / prt_scene_rebuild (the device-side rebuild of a
resident scene) against prt_scene_update_vertices (host positions, rebuild + re-upload of every table) and against
prt_scene_refit_device (no new tree), on the same motion; and what each tree is worth afterwards.  One GPU.

  python tools/rebuild_timing.py [--scenes cornell,bathroom2,soup1m] [--runs 10] [--out profiles/rebuild_timing.json]

Every scene is one child process under its own `timeout`; the first child that fails ends the run, and what it had printed
(one JSON line per figure, tools/timing_common.py) is still written.  Per scene the child records
  update     medians over --runs calls after a warm-up (alternating between two vertex sets, the sinusoidal displacement
             of timing_common.wobble at 1 % of the extent; emitters stay put), wall and hipEvent milliseconds, of
             rebuild_device (positions already on the device), rebuild (host positions), update_vertices (the yardstick)
             and refit_device; the builder's own time (PrtBvhInfo.build_ms) of the last rebuild_device
  trees      (the soup) K1 Mrays/s on 2M random rays after a 50 % sinusoidal displacement on three trees of the same
             positions: the refitted one (with its sah_ratio), the rebuilt one and update_vertices' one
There is no pass threshold: the numbers are quoted in DESIGN.md §7 and the README.
"""
import argparse
import functools
import os
import statistics
import sys

import timing_common as tc

SCENES = ("cornell", "bathroom2", "soup1m")
GROUPS = {"update": "update"}


def child(name, runs):
    import numpy as np
    import torch
    from pooraytracer_amd import api, build, scenes
    build.build()
    soup = name.startswith("soup")
    data, _ = tc.load(name, **({} if soup else {"width": 512, "height": 512}))
    mask = ~tc.emitter_mask(data)
    sets = [tc.wobble(data.vertices, mask), data.vertices.copy()]
    d_sets = [torch.from_numpy(v).cuda() for v in sets]
    sc = api.Scene(data).upload(0)
    tc.emit(n_tris=data.n_tris, runs=runs, bvh={k: sc.bvh_info()[k] for k in ("n_nodes", "depth", "tri_stride", "texture_bytes")})

    update = functools.partial(tc.emit_timed, "rebuild_timing " + name, "update", calls=False)
    update("refit_device", lambda i: sc.refit_device(d_sets[i % 2].data_ptr()), runs)
    device = update("rebuild_device", lambda i: sc.rebuild_device(d_sets[i % 2].data_ptr()), runs,
                    more=lambda: {k: sc.bvh_info()[k] for k in ("build_ms", "sort_ms", "tree_ms", "split_ms", "n_nodes")})
    host = update("rebuild", lambda i: sc.rebuild(sets[i % 2]), runs)
    slow = update("update_vertices", lambda i: sc.update_vertices(sets[i % 2]), max(3, runs // 2), warm=1)
    tc.emit(update="speedup_rebuild_device_over_update_wall", result=slow["wall_ms"] / device["wall_ms"])
    tc.emit(update="speedup_rebuild_over_update_wall", result=slow["wall_ms"] / host["wall_ms"])
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

        v = tc.wobble(data.vertices, mask, 0.5)
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
        tc.emit(trees=row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    tc.common_args(ap, launches=False, runs=10, out=os.path.join(tc.ROOT, "profiles", "rebuild_timing.json"), worker=True)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs)
    names = tc.scene_names(ap, args.scenes, SCENES)
    return tc.write_result(tc.run_children(__file__, names, tc.flags(args, "runs"), None, GROUPS), args.out)


if __name__ == "__main__":
    sys.exit(main())
