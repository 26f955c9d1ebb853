"""Cost of the any-hit occlusion query against the closest-hit query on identical ray batches; prints one JSON object.

  python tools/occlusion_timing.py [--scenes cornell-box,bathroom2,soup8m] [--log2-rays 24] [--launches 11]
                                   [--out profiles/occlusion_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept.  Per scene, on device-resident batches of
2^log2-rays rays:
  s0       the S0 incoherent rays (origin uniform in the scene's box, direction uniform on the sphere), tmax = inf
  shadow   scenes.shadow_segments: segments between pairs of random surface points, unit direction, over
           [1e-3, dist - 1e-3] (K3's NEE interval); pairs closer than 1e-2 are dropped, `rays` is what is left
  miss     the S0 rays cut off at tmax = 1e-4 of the box diagonal, which no triangle of these scenes lies within (the
           occluded fraction is reported: 0 or next to it): both kernels walk the same nodes and any-hit has no early-out
each traced by trace_closest_device and by trace_occluded_device, in fp64 and fp32, and on the soup also through the sorted
calls.  The two kernels alternate launch by launch after a warm-up of both; a figure is the median kernel_ms (hipEvents
around the launch, keys + sort included for the sorted calls) of --launches launches, with min and max beside it.
`ratio` = closest / occluded (above 1: any-hit is faster).  `mismatches` counts rays whose byte differs from
(closest prim >= 0): it must be 0.  One counting launch of each kernel gives the node fetches and triangle tests per ray.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> (scenes factory, keywords, tree built on the GPU, also time the sorted calls)
WORKLOADS = {
    "cornell-box": ("cornell_box", {}, False, False),
    "bathroom2": ("bathroom", {}, False, False),
    "soup8m": ("triangle_soup", {"n_tris": 8_000_000}, True, True),
}
CHILD_TIMEOUT_S = 900


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def child(name, log2_rays, launches, warmup):
    import numpy as np
    import torch
    from pooraytracer_amd import api, scenes
    factory, kw, device_bvh, with_sort = WORKLOADS[name]
    data = getattr(scenes, factory)(**kw)
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    n_max = 1 << log2_rays
    lo, hi = data.bounds()
    print(json.dumps({"n_tris": int(data.n_tris), "launches": launches}), flush=True)
    d_h = torch.zeros((n_max, 4), dtype=torch.float64, device="cuda")
    d_o = torch.zeros(n_max, dtype=torch.uint8, device="cuda")
    for kind in ("s0", "shadow", "miss"):
        rays = scenes.shadow_segments(data, n_max, seed=777) if kind == "shadow" else scenes.random_rays(n_max, lo, hi, seed=12345)
        if kind == "miss":
            rays["tmax"] = 1e-4 * float(np.linalg.norm(np.asarray(hi) - np.asarray(lo)))
        n = int(rays.shape[0])
        d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
        del rays
        for prec, pname in ((0, "f64"), (1, "f32")):
            for sort in ((False, True) if with_sort else (False,)):
                def closest(count=False):
                    sc.trace_closest_device(d_r.data_ptr(), n, d_h.data_ptr(), count_work=count, precision=prec, sort=sort)
                    torch.cuda.synchronize()
                    return sc.counters()

                def occluded(count=False):
                    sc.trace_occluded_device(d_r.data_ptr(), n, d_o.data_ptr(), count_work=count, precision=prec, sort=sort)
                    torch.cuda.synchronize()
                    return sc.counters()

                for _ in range(warmup):
                    closest()
                    occluded()
                t_c, t_o = [], []
                for _ in range(launches):  # alternating, so that a drift of the box hits both alike
                    t_c.append(closest()["kernel_ms"])
                    t_o.append(occluded()["kernel_ms"])
                prim = d_h.view(torch.int32).reshape(n_max, 8)[:n, 6]
                r = {"rays": n, "closest": stats(t_c), "occluded": stats(t_o),
                     "occluded_fraction": round(float((d_o[:n] != 0).float().mean().item()), 4),
                     "mismatches": int(((prim >= 0) != (d_o[:n] != 0)).sum().item())}
                r["ratio"] = round(r["closest"]["median_ms"] / r["occluded"]["median_ms"], 4)
                r["closest"]["mrays_s"] = round(n / r["closest"]["median_ms"] / 1e3, 1)
                r["occluded"]["mrays_s"] = round(n / r["occluded"]["median_ms"] / 1e3, 1)
                if not sort:
                    cc, co = closest(count=True), occluded(count=True)
                    r["per_ray"] = {"closest": {"node_fetches": round(cc["node_fetches"] / n, 3), "tri_tests": round(cc["tri_tests"] / n, 3)},
                                    "occluded": {"node_fetches": round(co["node_fetches"] / n, 3), "tri_tests": round(co["tri_tests"] / n, 3)}}
                print(json.dumps({"batch": kind, "variant": pname + ("-sorted" if sort else ""), "result": r}), flush=True)
                print(f"{name} {kind} {pname}{'-sorted' if sort else ''}: x{r['ratio']}", file=sys.stderr, flush=True)
        del d_r
    sc.close()


def collect(stdout):
    """A child's JSON lines as one scene entry: the header, then batches[kind][variant]."""
    res = {"batches": {}}
    for line in stdout.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if "batch" in rec:
            res["batches"].setdefault(rec["batch"], {})[rec["variant"]] = rec["result"]
        else:
            res.update(rec)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,bathroom2,soup8m")
    ap.add_argument("--log2-rays", type=int, default=24)
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches: the median of at least 10 launches")
    if args.child:
        return child(args.child, args.log2_rays, args.launches, args.warmup)
    from pooraytracer_amd import build
    build.build()
    out = {"log2_rays": args.log2_rays, "method": "median kernel_ms of alternating launches after warm-up; ratio = closest / occluded",
           "scenes": {}}
    for name in args.scenes.split(","):
        if name not in WORKLOADS:
            ap.error(f"unknown scene {name}")
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", name,
               "--log2-rays", str(args.log2_rays), "--launches", str(args.launches), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
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
