"""Cost of the winding-number query (prt_winding_number_device) at two values of beta, beside its exact form and beside the
signed distance query, of its switch and table, and of keeping the table in step with moving geometry; prints one JSON
object.

  python tools/winding_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-queries 20] [--log2-exact 10]
                                 [--launches 11] [--runs 20] [--parent-tree DIR] [--out profiles/winding_timing.json]

The query classes are those of tests/closest_point_model.queries.  Every scene is one child process under its own
`timeout`; the first child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints
each figure as one JSON line as soon as it has it (tools/timing_common.py).  Per scene, on device-resident batches of
2^log2-queries queries:
  `classes`   per class the median (min, max) kernel_ms of --launches launches of winding_number_device at beta = 2 and
              beta = 3 and of signed_distance_device on the SAME query buffer, launched alternately after a warm-up; the
              exact form (beta = inf: every triangle for every query, the only way to the value without the table) on the
              first 2^log2-exact queries of the class, as `exact_us_per_query` beside `beta2_us_per_query`; the largest
              |w(beta) - w(inf)| on those queries; the work counters per query at beta = 2
  `switch_on` the wall time of switching winding queries on for the uploaded scene (distance queries already on), median
              of 3, and `table_bytes` = 256 bytes per node
  `motion`    (soup1m only) medians over --runs calls of refit_device and rebuild_device with the switch off and on, the
              two states alternating block by block, in wall and hipEvent milliseconds, on the motion of
              timing_common.wobble
--parent-tree DIR: a built checkout of the parent commit.  Its refit_device and rebuild_device are timed by the same code
in the same session (`motion_parent`).
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


def motion(sc, data, name, runs, states, set_state):
    import numpy as np
    import torch
    start = np.ascontiguousarray(data.vertices)
    d_sets = [torch.from_numpy(tc.wobble(start, ~tc.emitter_mask(data))).cuda(), torch.from_numpy(start).cuda()]
    for call, res in tc.switch_blocks(sc, start, d_sets, runs, states, set_state):
        tc.emit(f"{name} {call}: {res}", motion=call, result=res)


def child(name, args):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api
    from tests import closest_point_model as CM
    data, device_bvh = tc.load(name)
    sc = api.Scene(data, device_bvh=device_bvh)
    if args.motion_only:  # the parent commit's library: it has no winding switch
        sc.upload(0)
        motion(sc, data, name, args.runs, ("off",), lambda state: None)
        sc.close()
        return
    sc.signed_queries = True
    sc.upload(0)
    n, m = 1 << args.log2_queries, 1 << args.log2_exact
    tc.emit(n_tris=int(data.n_tris), n_nodes=int(sc.bvh_info()["n_nodes"]), queries=n, exact_queries=m, launches=args.launches)
    walls = []
    for _ in range(3):
        sc.winding_queries = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.winding_queries = True
        walls.append(1e3 * (time.perf_counter() - t0))
    tc.emit(switch_on={"wall_ms": round(statistics.median(walls), 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3)},
            table_bytes=256 * int(sc.bvh_info()["n_nodes"]))
    d_w = {b: torch.zeros(n, dtype=torch.float64, device="cuda") for b in (2.0, 3.0)}
    d_exact = torch.zeros(m, dtype=torch.float64, device="cuda")
    d_sd = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    pts = CM.queries(data.vertices, n, 4242)
    for cls in CLASSES:
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"], q["max_dist"] = pts[cls][0], np.inf
        d_q = torch.from_numpy(q.view(np.float64).reshape(-1, 4)).cuda()
        beta2 = tc.launcher(sc, sc.winding_number_device, d_q.data_ptr(), n, d_w[2.0].data_ptr(), beta=2.0)
        beta3 = tc.launcher(sc, sc.winding_number_device, d_q.data_ptr(), n, d_w[3.0].data_ptr(), beta=3.0)
        signed = tc.launcher(sc, sc.signed_distance_device, d_q.data_ptr(), n, d_sd.data_ptr())
        exact = tc.launcher(sc, sc.winding_number_device, d_q.data_ptr(), m, d_exact.data_ptr(), beta=float("inf"))
        t, _ = tc.interleaved([("beta2", beta2), ("beta3", beta3), ("signed_distance", signed)], args.launches, args.warmup)
        r = {k: tc.stats(v) for k, v in t.items()}
        r["exact"] = tc.stats([exact()["kernel_ms"] for _ in range(3)])
        r["exact_us_per_query"] = round(1e3 * r["exact"]["median_ms"] / m, 4)
        for b in ("beta2", "beta3"):
            r[b + "_us_per_query"] = round(1e3 * r[b]["median_ms"] / n, 6)
            r["exact_over_" + b + "_per_query"] = round(r["exact_us_per_query"] / r[b + "_us_per_query"], 1)
            r[b + "_over_signed_distance"] = round(r[b]["median_ms"] / r["signed_distance"]["median_ms"], 4)
        for b in (2.0, 3.0):
            r[f"max_error_beta{int(b)}"] = float((d_w[b][:m] - d_exact).abs().max().item())
        c = beta2(count_work=True)
        r["beta2_work_per_query"] = {k: round(c[f] / n, 3) for k, f in (("nodes", "node_fetches"), ("solid_angles", "tri_tests"),
                                                                        ("far_inner", "inner_rounds"), ("far_leaf", "leaf_rounds"))}
        tc.emit(f"{name} {cls}: {r}", **{"class": cls}, result=r)
        del d_q
    if name == "soup1m":
        def set_state(state):
            sc.winding_queries = state == "winding"
            sc.signed_queries = False
            sc.distance_queries = state == "winding"
        motion(sc, data, name, args.runs, ("off", "winding"), set_state)
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--log2-exact", type=int, default=10)
    ap.add_argument("--motion-only", action="store_true")
    ap.add_argument("--parent-tree", default="")
    tc.common_args(ap, runs=20, out=os.path.join(tc.ROOT, "profiles", "winding_timing.json"))
    args = ap.parse_args()
    if args.log2_exact > args.log2_queries:
        ap.error("--log2-exact: at most --log2-queries")
    if args.child:
        return child(args.child, args)
    names = tc.scene_names(ap, args.scenes, SCENES)
    argv = tc.flags(args, "log2_queries", "log2_exact", "launches", "warmup", "runs")

    def parent(name, entry):
        """The parent commit's refit_device and rebuild_device on the soup, filed beside this tree's."""
        if name != "soup1m":
            return None
        res = tc.run_children(__file__, [name], argv + ["--motion-only"], None, GROUPS, tree=args.parent_tree)
        entry["motion_parent"] = res["scenes"][name]["motion"]
        return res.get("failed")

    out = {"log2_queries": args.log2_queries, "log2_exact": args.log2_exact,
           "method": "median kernel_ms of winding_number_device (beta 2, 3) and signed_distance_device launched alternately on the "
                     "same query buffer after warm-up; exact: beta = inf on the first 2^log2_exact queries, median of 3; motion: "
                     "medians of refit_device / rebuild_device calls, switch off and on alternating in blocks; motion_parent: "
                     "the parent commit's library, same code, same session"}
    out.update(tc.run_children(__file__, names, argv, None, GROUPS, then=parent if args.parent_tree else None))
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
