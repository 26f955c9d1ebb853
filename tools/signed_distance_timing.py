"""Cost of the signed distance query beside the closest-point query, of keeping its tables in step with moving geometry, and
of the host pass behind its switch; prints one JSON object.

  python tools/signed_distance_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-queries 20] [--launches 11]
                                         [--runs 20] [--parent-tree DIR] [--out profiles/signed_distance_timing.json]

The query classes are those of tests/closest_point_model.queries.  Every scene is one child process under its own
`timeout`; the first child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints
each figure as one JSON line as soon as it has it (tools/timing_common.py).  Per scene, on device-resident batches of
2^log2-queries queries:
  `classes`   per class the median (min, max) kernel_ms of --launches launches of closest_point_device and of
              signed_distance_device on the SAME query and output buffers, launched alternately after a warm-up, their ratio,
              and `record_mismatches`: records whose bytes other than sdist's sign bit and the sign word differ (must be 0)
  `switch_on` the wall time of switching signed queries on for the uploaded scene (distance queries already on): the host
              weld and adjacency pass plus the upload of the tables, median of 3; and `topology` with `table_bytes`
  `motion`    (soup1m only) medians over --runs calls of refit_device and rebuild_device with both switches off, with
              distance queries only, and with signed queries, the three states alternating block by block, in wall and
              hipEvent milliseconds, on the motion of timing_common.wobble
--parent-tree DIR: a built checkout of the parent commit.  Its closest_point_device is timed by the same code in the same
session (`parent_closest_point` per class), for the condition that this branch's closest_point_device stays within the
README's 2 % run-to-run spread of the parent's.
"""
import argparse
import os
import statistics
import sys
import time

import timing_common as tc

SCENES = ("cornell-box", "bathroom2", "soup1m")
GROUPS = {"class": "classes", "motion": "motion"}
CLASSES = ("surface", "near", "box")


def child(name, args):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api
    from tests import closest_point_model as CM
    data, device_bvh = tc.load(name)
    sc = api.Scene(data, device_bvh=device_bvh)
    sc.distance_queries = True
    sc.upload(0)
    n = 1 << args.log2_queries
    tc.emit(n_tris=int(data.n_tris), queries=n, launches=args.launches)
    if not args.closest_only:
        walls = []
        for _ in range(3):
            sc.signed_queries = False
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.signed_queries = True
            walls.append(1e3 * (time.perf_counter() - t0))
        tc.emit(switch_on={"wall_ms": round(statistics.median(walls), 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3)},
                topology=sc.topology_info())
    d_a = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    d_b = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    pts = CM.queries(data.vertices, n, 4242)
    for cls in CLASSES:
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"], q["max_dist"] = pts[cls][0], np.inf
        d_q = torch.from_numpy(q.view(np.float64).reshape(-1, 4)).cuda()
        calls = [("closest_point", tc.launcher(sc, sc.closest_point_device, d_q.data_ptr(), n, d_a.data_ptr()))]
        if not args.closest_only:
            calls.append(("signed_distance", tc.launcher(sc, sc.signed_distance_device, d_q.data_ptr(), n, d_b.data_ptr())))
        t, _ = tc.interleaved(calls, args.launches, args.warmup)
        r = {k: tc.stats(v) for k, v in t.items()}
        if not args.closest_only:
            r["signed_over_closest"] = round(r["signed_distance"]["median_ms"] / r["closest_point"]["median_ms"], 4)
            a, b = d_a.view(torch.int64).clone(), d_b.view(torch.int64).clone()
            b[:, 0] &= 0x7FFFFFFFFFFFFFFF  # |sdist|
            b[:, 7] &= 0xFFFFFFFF          # side; the sign word is closest_point's reserved = 0
            r["record_mismatches"] = int((a != b).any(1).sum().item())
            r["negative"] = int((d_b[:, 0] < 0).sum().item())
        tc.emit(f"{name} {cls}: {r}", **{"class": cls}, result=r)
        del d_q
    if args.closest_only or name != "soup1m":
        sc.close()
        return

    # ---- what the switches add to refit_device / rebuild_device (positions already on the device)
    start = np.ascontiguousarray(data.vertices)
    d_sets = [torch.from_numpy(tc.wobble(start, ~tc.emitter_mask(data))).cuda(), torch.from_numpy(start).cuda()]

    def set_state(state):
        sc.signed_queries = state == "signed"
        sc.distance_queries = state != "off"

    for call, res in tc.switch_blocks(sc, start, d_sets, args.runs, ("off", "distance", "signed"), set_state):
        res["signed_added_to_distance_wall_ms"] = round(res["signed"]["wall_ms"] - res["distance"]["wall_ms"], 4)
        res["signed_added_to_distance_event_ms"] = round(res["signed"]["event_ms"] - res["distance"]["event_ms"], 4)
        tc.emit(f"{name} {call}: {res}", motion=call, result=res)
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--closest-only", action="store_true")
    ap.add_argument("--parent-tree", default="")
    tc.common_args(ap, runs=20, out=os.path.join(tc.ROOT, "profiles", "signed_distance_timing.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    names = tc.scene_names(ap, args.scenes, SCENES)
    argv = tc.flags(args, "log2_queries", "launches", "warmup", "runs")

    def parent(name, entry):
        """The parent commit's closest_point_device on the same scene, filed beside this tree's."""
        res = tc.run_children(__file__, [name], argv + ["--closest-only"], None, GROUPS, tree=args.parent_tree)
        for cls, theirs in res["scenes"][name]["classes"].items():
            mine = entry["classes"].get(cls)
            if mine:
                mine["parent_closest_point"] = theirs["closest_point"]
                mine["closest_over_parent"] = round(mine["closest_point"]["median_ms"] / theirs["closest_point"]["median_ms"], 4)
        return res.get("failed")

    out = {"log2_queries": args.log2_queries,
           "method": "median kernel_ms of closest_point_device and signed_distance_device launched alternately on the same buffers "
                     "after warm-up; motion: medians of refit_device / rebuild_device calls, the three switch states alternating "
                     "in blocks; parent_closest_point: the parent commit's library, same code, same session"}
    out.update(tc.run_children(__file__, names, argv, None, GROUPS, then=parent if args.parent_tree else None))
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
