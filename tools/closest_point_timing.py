"""Cost of the closest-point query, and of keeping its corner table in step with moving geometry; prints one JSON object.

  python tools/closest_point_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-queries 20] [--launches 11]
                                       [--runs 20] [--out profiles/closest_point_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept.  Per scene, on device-resident batches of
2^log2-queries queries (tests/closest_point_model.queries), max_dist = inf:
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
`switch` is what prt_scene_set_distance_queries adds to moving geometry, on the motion of tools/refit_timing.py (the
sinusoidal displacement at 1 % of the extent, alternating with the start positions, emitters in place, positions already on
the device): medians over --runs calls of refit_device and of rebuild_device with the switch off and with it on - the same
scene object, the two states alternating block by block - in wall and hipEvent milliseconds, and `table_bytes`.
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

# name -> (scenes factory, keywords, tree built on the GPU)
WORKLOADS = {
    "cornell-box": ("cornell_box", {}, False),
    "bathroom2": ("bathroom", {}, False),
    "soup1m": ("triangle_soup", {"n_tris": 1_000_000}, True),
}
CHILD_TIMEOUT_S = 900
CLASSES = ("surface", "near", "box")


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def child(name, log2_queries, launches, warmup, runs):
    import numpy as np
    import torch
    from pooraytracer_amd import _abi, api, scenes
    from tests import closest_point_model as CM
    factory, kw, device_bvh = WORKLOADS[name]
    data = getattr(scenes, factory)(**kw)
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
    n = 1 << log2_queries
    info = sc.bvh_info()
    print(json.dumps({"n_tris": int(data.n_tris), "n_nodes": int(info["n_nodes"]), "stack_need": int(info["stack_need"]),
                      "launches": launches, "queries": n, "table_bytes": int(data.n_tris) * 96}), flush=True)
    lo, hi = data.bounds()
    rays = scenes.random_rays(n, lo, hi, seed=12345)
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
    d_h = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_o = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    d_p = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    del rays

    def k1():
        sc.trace_closest_device(d_r.data_ptr(), n, d_h.data_ptr())
        torch.cuda.synchronize()
        return sc.counters()

    pts = CM.queries(data.vertices, n, 4242)
    for cls in CLASSES:
        q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
        q["p"], q["max_dist"] = pts[cls][0], np.inf
        d_q = torch.from_numpy(q.view(np.float64).reshape(-1, 4)).cuda()

        def query(count=False, s=sc, out=d_o):
            s.closest_point_device(d_q.data_ptr(), n, out.data_ptr(), count_work=count)
            torch.cuda.synchronize()
            return s.counters()

        for _ in range(warmup):
            query()
            query(s=sc_plain, out=d_p)
            k1()
        t_q, t_p, t_k = [], [], []
        for _ in range(launches):  # alternating, so that a drift of the box hits all alike
            t_q.append(query()["kernel_ms"])
            t_p.append(query(s=sc_plain, out=d_p)["kernel_ms"])
            t_k.append(k1()["kernel_ms"])
        c = query(count=True)
        r = {"closest_point": stats(t_q), "plain_schedule": stats(t_p), "k1": stats(t_k)}
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
        print(json.dumps({"class": cls, "result": r}), flush=True)
        print(f"{name} {cls}: {r['closest_point']['median_ms']} ms, x{r['ratio_to_k1']} of K1", file=sys.stderr, flush=True)
        del d_q
    sc_plain.close()

    # ---- what the switch adds to refit_device / rebuild_device
    mask = np.ones(data.n_tris, dtype=bool)
    first = np.asarray(data.mesh_first_tri, dtype=np.int64)
    for m, mat in enumerate(data.mesh_material):
        if data.materials[int(mat)].type == _abi.MAT_DIFFUSE_LIGHT:
            mask[first[m]:first[m + 1]] = False
    p = data.vertices[mask].reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    v = data.vertices.copy()
    w = data.vertices[mask]
    v[mask] = w + 0.01 * ext * np.sin(7.0 / ext * w[..., [1, 2, 0]] + np.array([0.3, 1.1, 2.3]))
    d_sets = [torch.from_numpy(v).cuda(), torch.from_numpy(np.ascontiguousarray(data.vertices)).cuda()]

    def timed(fn, k, warm=2):
        wall, evt = [], []
        for i in range(warm + k):
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
        return wall, evt

    # the switch can only be turned on while the host copy of the geometry is current: each block ends on the start
    # positions, and a host refit to them makes the copy current again before the switch changes
    block = max(2, runs // 4) * 2
    start = np.ascontiguousarray(data.vertices)
    out = {}
    for call, fn in (("refit_device", sc.refit_device), ("rebuild_device", sc.rebuild_device)):
        acc = {False: ([], []), True: ([], [])}
        done = 0
        while done < runs:
            for on in (False, True):
                sc.refit(start)
                sc.distance_queries = on
                wall, evt = timed(lambda i: fn(d_sets[i % 2].data_ptr()), block)
                acc[on][0].extend(wall)
                acc[on][1].extend(evt)
            done += block
        res = {("on" if on else "off"): {"wall_ms": round(statistics.median(a[0]), 4), "event_ms": round(statistics.median(a[1]), 4),
                                        "wall_min_ms": round(min(a[0]), 4), "wall_max_ms": round(max(a[0]), 4), "calls": len(a[0])}
               for on, a in acc.items()}
        res["added_wall_ms"] = round(res["on"]["wall_ms"] - res["off"]["wall_ms"], 4)
        res["added_event_ms"] = round(res["on"]["event_ms"] - res["off"]["event_ms"], 4)
        out[call] = res
        print(json.dumps({"switch": call, "result": res}), flush=True)
        print(f"{name} {call}: +{res['added_wall_ms']} ms wall with the switch on", file=sys.stderr, flush=True)
    sc.close()


def collect(stdout):
    """A child's JSON lines as one scene entry: the header, then classes[cls] and switch[call]."""
    res = {"classes": {}, "switch": {}}
    for line in stdout.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if "class" in rec:
            res["classes"][rec["class"]] = rec["result"]
        elif "switch" in rec:
            res["switch"][rec["switch"]] = rec["result"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_point_timing.json"))
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches: the median of at least 10 launches")
    if args.child:
        return child(args.child, args.log2_queries, args.launches, args.warmup, args.runs)
    from pooraytracer_amd import build
    build.build()
    out = {"log2_queries": args.log2_queries,
           "method": "median kernel_ms of launches alternating with K1 after warm-up; counters from one counting launch; "
                     "switch: medians of refit_device / rebuild_device calls, switch off and on alternating in blocks",
           "scenes": {}}
    for name in args.scenes.split(","):
        if name not in WORKLOADS:
            ap.error(f"unknown scene {name}")
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", name,
               "--log2-queries", str(args.log2_queries), "--launches", str(args.launches), "--warmup", str(args.warmup),
               "--runs", str(args.runs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        out["scenes"][name] = collect(r.stdout)
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
