"""Cost of the winding-number query (prt_winding_number_device) at two values of beta, beside its exact form and beside the
signed distance query, of its switch and table, and of keeping the table in step with moving geometry; prints one JSON
object.

  python tools/winding_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-queries 20] [--log2-exact 10]
                                 [--launches 11] [--runs 20] [--parent-tree DIR] [--out profiles/winding_timing.json]

The scenes and query classes are those of tools/closest_point_timing.py.  Every scene is one child process under its own
`timeout`; the first child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints
each figure as one JSON line as soon as it has it.  Per scene, on device-resident batches of 2^log2-queries queries:
  `classes`   per class the median (min, max) kernel_ms of --launches launches of winding_number_device at beta = 2 and
              beta = 3 and of signed_distance_device on the SAME query buffer, launched alternately after a warm-up; the
              exact form (beta = inf: every triangle for every query, the only way to the value without the table) on the
              first 2^log2-exact queries of the class, as `exact_us_per_query` beside `beta2_us_per_query`; the largest
              |w(beta) - w(inf)| on those queries; the work counters per query at beta = 2
  `switch_on` the wall time of switching winding queries on for the uploaded scene (distance queries already on), median
              of 3, and `table_bytes` = 256 bytes per node
  `motion`    (soup1m only) medians over --runs calls of refit_device and rebuild_device with the switch off and on, the
              two states alternating block by block, in wall and hipEvent milliseconds, on the motion of
              tools/refit_timing.py
--parent-tree DIR: a built checkout of the parent commit.  Its refit_device and rebuild_device are timed by the same code
in the same session (`motion_parent`).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PRT_TIMING_TREE") or ROOT  # the checkout whose package and library a child times
if TREE not in sys.path:
    sys.path.insert(0, TREE)

WORKLOADS = {
    "cornell-box": ("cornell_box", {}, False),
    "bathroom2": ("bathroom", {}, False),
    "soup1m": ("triangle_soup", {"n_tris": 1_000_000}, True),
}
CHILD_TIMEOUT_S = 600
CLASSES = ("surface", "near", "box")


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def motion(sc, data, runs, states, set_state):
    """Medians of refit_device / rebuild_device (positions already on the device) in each of `states`, alternating in blocks."""
    import numpy as np
    import torch
    from pooraytracer_amd import _abi
    mask = np.ones(data.n_tris, dtype=bool)  # emitters stay in place under a refit
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = False
    w = data.vertices[mask]
    ext = float((w.reshape(-1, 3).max(0) - w.reshape(-1, 3).min(0)).max())
    start = np.ascontiguousarray(data.vertices)
    v = start.copy()
    v[mask] = w + 0.01 * ext * np.sin(7.0 / ext * w[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3]))
    d_sets = [torch.from_numpy(v).cuda(), torch.from_numpy(start).cuda()]

    def timed(fn, k, warm=2):
        wall, evt = [], []
        for i in range(warm + k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn(d_sets[i % 2].data_ptr())
            e1.record()
            torch.cuda.synchronize()
            if i >= warm:
                wall.append(1e3 * (time.perf_counter() - t0))
                evt.append(e0.elapsed_time(e1))
        return wall, evt

    block = max(2, runs // 4) * 2
    out = {}
    for call, fn in (("refit_device", sc.refit_device), ("rebuild_device", sc.rebuild_device)):
        acc = {s: ([], []) for s in states}
        done = 0
        while done < runs:
            for state in acc:
                sc.refit(start)  # the host copy is made current first: the switch refuses to turn on while it is stale
                set_state(state)
                wall, evt = timed(fn, block)
                acc[state][0].extend(wall)
                acc[state][1].extend(evt)
            done += block
        out[call] = {s: {"wall_ms": round(statistics.median(a[0]), 4), "event_ms": round(statistics.median(a[1]), 4),
                         "wall_min_ms": round(min(a[0]), 4), "wall_max_ms": round(max(a[0]), 4), "calls": len(a[0])} for s, a in acc.items()}
        print(json.dumps({"motion": call, "result": out[call]}), flush=True)
        print(f"{call}: {out[call]}", file=sys.stderr, flush=True)
    return out


def child(name, log2_queries, log2_exact, launches, warmup, runs, motion_only):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, scenes
    from tests import closest_point_model as CM
    factory, kw, device_bvh = WORKLOADS[name]
    data = getattr(scenes, factory)(**kw)
    sc = api.Scene(data, device_bvh=device_bvh)
    if motion_only:  # the parent commit's library: it has no winding switch
        sc.upload(0)
        motion(sc, data, runs, ("off",), lambda state: None)
        sc.close()
        return
    sc.signed_queries = True
    sc.upload(0)
    n, m = 1 << log2_queries, 1 << log2_exact
    print(json.dumps({"n_tris": int(data.n_tris), "n_nodes": int(sc.bvh_info()["n_nodes"]), "queries": n, "exact_queries": m,
                      "launches": launches}), flush=True)
    walls = []
    for _ in range(3):
        sc.winding_queries = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.winding_queries = True
        walls.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"switch_on": {"wall_ms": round(statistics.median(walls), 3), "min_ms": round(min(walls), 3),
                                    "max_ms": round(max(walls), 3)}, "table_bytes": 256 * int(sc.bvh_info()["n_nodes"])}), flush=True)
    d_w = {b: torch.zeros(n, dtype=torch.float64, device="cuda") for b in (2.0, 3.0)}
    d_exact = torch.zeros(m, dtype=torch.float64, device="cuda")
    d_sd = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    pts = CM.queries(data.vertices, n, 4242)
    for cls in CLASSES:
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"], q["max_dist"] = pts[cls][0], np.inf
        d_q = torch.from_numpy(q.view(np.float64).reshape(-1, 4)).cuda()

        def run(fn):
            fn()
            torch.cuda.synchronize()
            return sc.counters()

        calls = [("beta2", lambda: sc.winding_number_device(d_q.data_ptr(), n, d_w[2.0].data_ptr(), beta=2.0)),
                 ("beta3", lambda: sc.winding_number_device(d_q.data_ptr(), n, d_w[3.0].data_ptr(), beta=3.0)),
                 ("signed_distance", lambda: sc.signed_distance_device(d_q.data_ptr(), n, d_sd.data_ptr()))]
        for _ in range(warmup):
            for _, fn in calls:
                run(fn)
        t = {k: [] for k, _ in calls}
        for _ in range(launches):  # alternating, so that a drift of the box hits all alike
            for k, fn in calls:
                t[k].append(run(fn)["kernel_ms"])
        r = {k: stats(v) for k, v in t.items()}
        exact_ms = [run(lambda: sc.winding_number_device(d_q.data_ptr(), m, d_exact.data_ptr(), beta=float("inf")))["kernel_ms"]
                    for _ in range(3)]
        r["exact"] = stats(exact_ms)
        r["exact_us_per_query"] = round(1e3 * r["exact"]["median_ms"] / m, 4)
        for b in ("beta2", "beta3"):
            r[b + "_us_per_query"] = round(1e3 * r[b]["median_ms"] / n, 6)
            r["exact_over_" + b + "_per_query"] = round(r["exact_us_per_query"] / r[b + "_us_per_query"], 1)
            r[b + "_over_signed_distance"] = round(r[b]["median_ms"] / r["signed_distance"]["median_ms"], 4)
        for b in (2.0, 3.0):
            r[f"max_error_beta{int(b)}"] = float((d_w[b][:m] - d_exact).abs().max().item())
        c = run(lambda: sc.winding_number_device(d_q.data_ptr(), n, d_w[2.0].data_ptr(), beta=2.0, count_work=True))
        r["beta2_work_per_query"] = {k: round(c[f] / n, 3) for k, f in (("nodes", "node_fetches"), ("solid_angles", "tri_tests"),
                                                                        ("far_inner", "inner_rounds"), ("far_leaf", "leaf_rounds"))}
        print(json.dumps({"class": cls, "result": r}), flush=True)
        print(f"{name} {cls}: {r}", file=sys.stderr, flush=True)
        del d_q
    if name == "soup1m":
        def set_state(state):
            sc.winding_queries = state == "winding"
            sc.signed_queries = False
            sc.distance_queries = state == "winding"
        motion(sc, data, runs, ("off", "winding"), set_state)
    sc.close()


def collect(stdout):
    res = {"classes": {}, "motion": {}}
    for line in stdout.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if "class" in rec:
            res["classes"][rec["class"]] = rec["result"]
        elif "motion" in rec:
            res["motion"][rec["motion"]] = rec["result"]
        else:
            res.update(rec)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,bathroom2,soup1m")
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--log2-exact", type=int, default=10)
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--child", default="")
    ap.add_argument("--motion-only", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_timing.json"))
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches: the median of at least 10 launches")
    if args.log2_exact > args.log2_queries:
        ap.error("--log2-exact: at most --log2-queries")
    if args.child:
        return child(args.child, args.log2_queries, args.log2_exact, args.launches, args.warmup, args.runs, args.motion_only)
    out = {"log2_queries": args.log2_queries, "log2_exact": args.log2_exact,
           "method": "median kernel_ms of winding_number_device (beta 2, 3) and signed_distance_device launched alternately on the "
                     "same query buffer after warm-up; exact: beta = inf on the first 2^log2_exact queries, median of 3; motion: "
                     "medians of refit_device / rebuild_device calls, switch off and on alternating in blocks; motion_parent: "
                     "the parent commit's library, same code, same session",
           "scenes": {}}
    for name in args.scenes.split(","):
        if name not in WORKLOADS:
            ap.error(f"unknown scene {name}")
        base = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", name,
                "--log2-queries", str(args.log2_queries), "--log2-exact", str(args.log2_exact), "--launches", str(args.launches),
                "--warmup", str(args.warmup), "--runs", str(args.runs)]
        r = subprocess.run(base, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        out["scenes"][name] = collect(r.stdout)
        if r.returncode == 0 and args.parent_tree and name == "soup1m":
            env = dict(os.environ, PRT_TIMING_TREE=os.path.abspath(args.parent_tree))
            r = subprocess.run(base + ["--motion-only"], stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(args.parent_tree), env=env)
            out["scenes"][name]["motion_parent"] = collect(r.stdout)["motion"]
        if r.returncode != 0:
            out["failed"] = {"scene": name, "returncode": r.returncode}
            break  # nothing more is started after a failure
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
