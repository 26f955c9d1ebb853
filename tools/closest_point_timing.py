"""Cost of the closest-point query, and of keeping its corner table in step with moving geometry; prints one JSON object.

  python tools/closest_point_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-queries 20] [--launches 11]
                                       [--runs 20] [--out profiles/closest_point_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept (tools/timing_common.py).  Per scene, on
device-resident batches of 2^log2-queries queries (tests/closest_point_model.queries), max_dist = inf:
  surface   points on random triangles
  near      those displaced by up to 1 % of the extent in a random direction
  box       uniform in the bounds padded by 10 % of the extent
`kernel_ms` is the median of --launches launches of closest_point_device after a warm-up (hipEvents around the launch),
with min and max beside it, and Mqueries/s from the median.  `plain_schedule` is the same kernel without the refill of
finished lanes (one lane per query; dev-hooks build), launched alternately; `record_mismatches` must be 0.  `k1` is, from the same run, K1's time for as many incoherent
rays (origin uniform in the scene's box, direction uniform on the sphere, tmax = inf) on that scene: context, launched
alternately with the queries.  One counting launch per class gives per query `node_fetches` and `tri_tests`, and the stack
entries the bound they carry dropped at the pop without a fetch (`dropped_inner`, `dropped_leaf`): what a 4-byte stack
entry would have fetched (a node) or tested (a leaf's triangles) on top.
`switch` is what prt_scene_set_distance_queries adds to moving geometry, on the motion of timing_common.wobble (the
sinusoidal displacement at 1 % of the extent, alternating with the start positions, emitters in place, positions already on
the device): medians over --runs calls of refit_device and of rebuild_device with the switch off and with it on - the same
scene object, the two states alternating block by block (timing_common.switch_blocks) - in wall and hipEvent
milliseconds, and `table_bytes`.
"""
import argparse
import os
import sys

import timing_common as tc

SCENES = ("cornell-box", "bathroom2", "soup1m")
GROUPS = {"class": "classes", "switch": "switch"}
CLASSES = ("surface", "near", "box")


def child(name, args):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, scenes
    from tests import closest_point_model as CM
    data, device_bvh = tc.load(name)
    sc = api.Scene(data, device_bvh=device_bvh)
    sc.distance_queries = True
    sc.upload(0)
    # the plain schedule (one lane per query, no refill) for comparison: the same kernel's other instantiation, which only
    # the dev-hooks build of the library launches (PRT_TUNE_CLOSEST_PLAIN; the shipped library reads no environment variable)
    os.environ["PRT_TUNE_CLOSEST_PLAIN"] = "1"
    with api.dev_hooks():
        sc_plain = api.Scene(data, device_bvh=device_bvh)
    sc_plain.distance_queries = True
    sc_plain.upload(0)
    n = 1 << args.log2_queries
    info = sc.bvh_info()
    tc.emit(n_tris=int(data.n_tris), n_nodes=int(info["n_nodes"]), stack_need=int(info["stack_need"]), launches=args.launches, queries=n,
            table_bytes=int(data.n_tris) * 96)
    lo, hi = data.bounds()
    rays = scenes.random_rays(n, lo, hi, seed=12345)
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
    d_h = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_o = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    d_p = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    del rays
    k1 = tc.launcher(sc, sc.trace_closest_device, d_r.data_ptr(), n, d_h.data_ptr())
    pts = CM.queries(data.vertices, n, 4242)
    for cls in CLASSES:
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"], q["max_dist"] = pts[cls][0], np.inf
        d_q = torch.from_numpy(q.view(np.float64).reshape(-1, 4)).cuda()
        query = tc.launcher(sc, sc.closest_point_device, d_q.data_ptr(), n, d_o.data_ptr())
        plain = tc.launcher(sc_plain, sc_plain.closest_point_device, d_q.data_ptr(), n, d_p.data_ptr())
        t, _ = tc.interleaved([("closest_point", query), ("plain_schedule", plain), ("k1", k1)], args.launches, args.warmup)
        c = query(count_work=True)
        r = {k: tc.stats(v) for k, v in t.items()}
        r["plain_over_refill"] = round(r["plain_schedule"]["median_ms"] / r["closest_point"]["median_ms"], 4)
        r["record_mismatches"] = int((d_o.view(torch.int64) != d_p.view(torch.int64)).any(1).sum().item())
        r["closest_point"]["mqueries_s"] = round(n / r["closest_point"]["median_ms"] / 1e3, 1)
        r["k1"]["mrays_s"] = round(n / r["k1"]["median_ms"] / 1e3, 1)
        r["ratio_to_k1"] = round(r["closest_point"]["median_ms"] / r["k1"]["median_ms"], 4)
        r["per_query"] = {"node_fetches": round(c["node_fetches"] / n, 3), "tri_tests": round(c["tri_tests"] / n, 3),
                          "dropped_inner": round(c["inner_rounds"] / n, 3), "dropped_leaf": round(c["leaf_rounds"] / n, 3)}
        d = d_o[:, 0]
        r["mean_dist"] = float(d.mean().item())
        r["misses"] = int(torch.isinf(d).sum().item())
        tc.emit(f"{name} {cls}: {r['closest_point']['median_ms']} ms, x{r['ratio_to_k1']} of K1", **{"class": cls}, result=r)
        del d_q
    sc_plain.close()

    # ---- what the switch adds to refit_device / rebuild_device
    start = np.ascontiguousarray(data.vertices)
    d_sets = [torch.from_numpy(tc.wobble(start, ~tc.emitter_mask(data))).cuda(), torch.from_numpy(start).cuda()]

    def set_state(state):
        sc.distance_queries = state == "on"

    for call, res in tc.switch_blocks(sc, start, d_sets, args.runs, ("off", "on"), set_state):
        res["added_wall_ms"] = round(res["on"]["wall_ms"] - res["off"]["wall_ms"], 4)
        res["added_event_ms"] = round(res["on"]["event_ms"] - res["off"]["event_ms"], 4)
        tc.emit(f"{name} {call}: +{res['added_wall_ms']} ms wall with the switch on", switch=call, result=res)
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--log2-queries", type=int, default=20)
    tc.common_args(ap, runs=20, out=os.path.join(tc.ROOT, "profiles", "closest_point_timing.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    names = tc.scene_names(ap, args.scenes, SCENES)
    from pooraytracer_amd import build
    build.build()
    out = {"log2_queries": args.log2_queries,
           "method": "median kernel_ms of launches alternating with K1 after warm-up; counters from one counting launch; "
                     "switch: medians of refit_device / rebuild_device calls, switch off and on alternating in blocks"}
    out.update(tc.run_children(__file__, names, tc.flags(args, "log2_queries", "launches", "warmup", "runs"), None, GROUPS))
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
