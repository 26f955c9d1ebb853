"""Cost of the signed distance query beside the closest-point query, of keeping its tables in step with moving geometry, and
of the host pass behind its switch; prints one JSON object.

  python tools/signed_distance_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-queries 20] [--launches 11]
                                         [--runs 20] [--parent-tree DIR] [--out profiles/signed_distance_timing.json]

The scenes and query classes are those of tools/closest_point_timing.py.  Every scene is one child process under its own
`timeout`; the first child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints
each figure as one JSON line as soon as it has it.  Per scene, on device-resident batches of 2^log2-queries queries:
  `classes`   per class the median (min, max) kernel_ms of --launches launches of closest_point_device and of
              signed_distance_device on the SAME query and output buffers, launched alternately after a warm-up, their ratio,
              and `record_mismatches`: records whose bytes other than sdist's sign bit and the sign word differ (must be 0)
  `switch_on` the wall time of switching signed queries on for the uploaded scene (distance queries already on): the host
              weld and adjacency pass plus the upload of the tables, median of 3; and `topology` with `table_bytes`
  `motion`    (soup1m only) medians over --runs calls of refit_device and rebuild_device with both switches off, with
              distance queries only, and with signed queries, the three states alternating block by block, in wall and
              hipEvent milliseconds, on the motion of tools/refit_timing.py
--parent-tree DIR: a built checkout of the parent commit.  Its closest_point_device is timed by the same code in the same
session (`parent_closest_point` per class), for the condition that this branch's closest_point_device stays within the
README's 2 % run-to-run spread of the parent's.
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


def child(name, log2_queries, launches, warmup, runs, closest_only):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, scenes
    from tests import closest_point_model as CM
    factory, kw, device_bvh = WORKLOADS[name]
    data = getattr(scenes, factory)(**kw)
    sc = api.Scene(data, device_bvh=device_bvh)
    sc.distance_queries = True
    sc.upload(0)
    n = 1 << log2_queries
    print(json.dumps({"n_tris": int(data.n_tris), "queries": n, "launches": launches}), flush=True)
    if not closest_only:
        walls = []
        for _ in range(3):
            sc.signed_queries = False
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.signed_queries = True
            walls.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"switch_on": {"wall_ms": round(statistics.median(walls), 3), "min_ms": round(min(walls), 3),
                                        "max_ms": round(max(walls), 3)}, "topology": sc.topology_info()}), flush=True)
    d_a = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    d_b = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    pts = CM.queries(data.vertices, n, 4242)
    for cls in CLASSES:
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"], q["max_dist"] = pts[cls][0], np.inf
        d_q = torch.from_numpy(q.view(np.float64).reshape(-1, 4)).cuda()

        def run(fn, out):
            fn(d_q.data_ptr(), n, out.data_ptr())
            torch.cuda.synchronize()
            return sc.counters()["kernel_ms"]

        calls = [("closest_point", sc.closest_point_device, d_a)]
        if not closest_only:
            calls.append(("signed_distance", sc.signed_distance_device, d_b))
        for _ in range(warmup):
            for _, fn, out in calls:
                run(fn, out)
        t = {k: [] for k, _, _ in calls}
        for _ in range(launches):  # alternating, so that a drift of the box hits both alike
            for k, fn, out in calls:
                t[k].append(run(fn, out))
        r = {k: stats(v) for k, v in t.items()}
        if not closest_only:
            r["signed_over_closest"] = round(r["signed_distance"]["median_ms"] / r["closest_point"]["median_ms"], 4)
            a, b = d_a.view(torch.int64).clone(), d_b.view(torch.int64).clone()
            b[:, 0] &= 0x7FFFFFFFFFFFFFFF  # |sdist|
            b[:, 7] &= 0xFFFFFFFF          # side; the sign word is closest_point's reserved = 0
            r["record_mismatches"] = int((a != b).any(1).sum().item())
            r["negative"] = int((d_b[:, 0] < 0).sum().item())
        print(json.dumps({"class": cls, "result": r}), flush=True)
        print(f"{name} {cls}: {r}", file=sys.stderr, flush=True)
        del d_q
    if closest_only or name != "soup1m":
        sc.close()
        return

    # ---- what the switches add to refit_device / rebuild_device (positions already on the device)
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

    def set_state(state):  # the host copy is made current first: the switches refuse to turn on while it is stale
        sc.refit(start)
        sc.signed_queries = state == "signed"
        sc.distance_queries = state != "off"

    block = max(2, runs // 4) * 2
    for call, fn in (("refit_device", sc.refit_device), ("rebuild_device", sc.rebuild_device)):
        acc = {s: ([], []) for s in ("off", "distance", "signed")}
        done = 0
        while done < runs:
            for state in acc:
                set_state(state)
                wall, evt = timed(fn, block)
                acc[state][0].extend(wall)
                acc[state][1].extend(evt)
            done += block
        res = {s: {"wall_ms": round(statistics.median(a[0]), 4), "event_ms": round(statistics.median(a[1]), 4),
                   "wall_min_ms": round(min(a[0]), 4), "wall_max_ms": round(max(a[0]), 4), "calls": len(a[0])} for s, a in acc.items()}
        res["signed_added_to_distance_wall_ms"] = round(res["signed"]["wall_ms"] - res["distance"]["wall_ms"], 4)
        res["signed_added_to_distance_event_ms"] = round(res["signed"]["event_ms"] - res["distance"]["event_ms"], 4)
        print(json.dumps({"motion": call, "result": res}), flush=True)
        print(f"{name} {call}: {res}", file=sys.stderr, flush=True)
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
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--child", default="")
    ap.add_argument("--closest-only", action="store_true")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_distance_timing.json"))
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches: the median of at least 10 launches")
    if args.child:
        return child(args.child, args.log2_queries, args.launches, args.warmup, args.runs, args.closest_only)
    out = {"log2_queries": args.log2_queries,
           "method": "median kernel_ms of closest_point_device and signed_distance_device launched alternately on the same buffers "
                     "after warm-up; motion: medians of refit_device / rebuild_device calls, the three switch states alternating "
                     "in blocks; parent_closest_point: the parent commit's library, same code, same session",
           "scenes": {}}
    for name in args.scenes.split(","):
        if name not in WORKLOADS:
            ap.error(f"unknown scene {name}")
        base = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", name,
                "--log2-queries", str(args.log2_queries), "--launches", str(args.launches), "--warmup", str(args.warmup),
                "--runs", str(args.runs)]
        r = subprocess.run(base, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        out["scenes"][name] = collect(r.stdout)
        if r.returncode == 0 and args.parent_tree:
            env = dict(os.environ, PRT_TIMING_TREE=os.path.abspath(args.parent_tree))
            r = subprocess.run(base + ["--closest-only"], stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(args.parent_tree), env=env)
            for cls, res in collect(r.stdout)["classes"].items():
                mine = out["scenes"][name]["classes"].get(cls)
                if mine:
                    mine["parent_closest_point"] = res["closest_point"]
                    mine["closest_over_parent"] = round(mine["closest_point"]["median_ms"] / res["closest_point"]["median_ms"], 4)
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
