"""Cost of the surface query against the closest-hit query on identical ray batches; prints one JSON object.

  python tools/surface_timing.py [--scenes cornell-box,bathroom2,soup8m] [--batches s0,shadow] [--log2-rays 24]
                                 [--launches 11] [--out profiles/surface_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept.  Per scene, on the device-resident batches of
2^log2-rays rays that tools/occlusion_timing.py uses:
  s0       the S0 incoherent rays (origin uniform in the scene's box, direction uniform on the sphere), tmax = inf
  shadow   scenes.shadow_segments: segments between pairs of random surface points, unit direction, over
           [1e-3, dist - 1e-3]; pairs closer than 1e-2 are dropped, `rays` is what is left
each traced by trace_closest_device (32 bytes out per ray) and by trace_surface_device (192 bytes out per ray), unsorted and
through the sorted calls, in fp64 and fp32.  The two kernels alternate launch by launch after a warm-up of both; a figure is
the median kernel_ms (hipEvents around the launch, keys + sort included for the sorted calls) of --launches launches, with
min and max beside it.  `ratio` = surface / closest (above 1: what the record costs over the hit).  `write_gb_s` = the
192 bytes per ray the surface call must write over its median time; `extra_write_gb_s` = the 160 bytes it writes beyond
the hit over the time it takes beyond the closest-hit call.  `head_mismatches` counts records whose first 32 bytes differ
from the closest-hit call's PrtHit: it must be 0.  `hit_fraction` and `textured_fraction` (hits whose albedo came from a
texture fetch) say what the write-out had to do.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> (scenes factory, keywords, tree built on the GPU)
WORKLOADS = {
    "cornell-box": ("cornell_box", {}, False),
    "bathroom2": ("bathroom", {}, False),
    "soup8m": ("triangle_soup", {"n_tris": 8_000_000}, True),
}
CHILD_TIMEOUT_S = 900
RECORD_BYTES, HIT_BYTES = 192, 32


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def child(name, log2_rays, launches, warmup, batches):
    import numpy as np
    import torch
    from pooraytracer_amd import api, scenes
    factory, kw, device_bvh = WORKLOADS[name]
    data = getattr(scenes, factory)(**kw)
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    n_max = 1 << log2_rays
    lo, hi = data.bounds()
    textured = torch.tensor([m.texture >= 0 and m.type in (0, 1, 5) for m in data.materials] + [False], device="cuda")  # [-1]: a miss
    print(json.dumps({"n_tris": int(data.n_tris), "launches": launches}), flush=True)
    d_h = torch.zeros((n_max, HIT_BYTES // 8), dtype=torch.float64, device="cuda")
    d_s = torch.zeros((n_max, RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
    for kind in batches:
        rays = scenes.shadow_segments(data, n_max, seed=777) if kind == "shadow" else scenes.random_rays(n_max, lo, hi, seed=12345)
        n = int(rays.shape[0])
        d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
        del rays
        for prec, pname in ((0, "f64"), (1, "f32")):
            for sort in (False, True):
                def closest():
                    sc.trace_closest_device(d_r.data_ptr(), n, d_h.data_ptr(), precision=prec, sort=sort)
                    torch.cuda.synchronize()
                    return sc.counters()

                def surface():
                    sc.trace_surface_device(d_r.data_ptr(), n, d_s.data_ptr(), precision=prec, sort=sort)
                    torch.cuda.synchronize()
                    return sc.counters()

                for _ in range(warmup):
                    closest()
                    surface()
                t_c, t_s = [], []
                for _ in range(launches):  # alternating, so that a drift of the box hits both alike
                    t_c.append(closest()["kernel_ms"])
                    t_s.append(surface()["kernel_ms"])
                words = d_s.view(torch.int64)[:n]
                mat = d_s.view(torch.int32).reshape(n_max, RECORD_BYTES // 4)[:n, 42].long()
                r = {"rays": n, "closest": stats(t_c), "surface": stats(t_s),
                     "hit_fraction": round(float((mat >= 0).float().mean().item()), 4),
                     "textured_fraction": round(float(textured[mat].float().mean().item()), 4),
                     "head_mismatches": int((words[:, :4] != d_h.view(torch.int64)[:n]).any(1).sum().item())}
                ms_c, ms_s = r["closest"]["median_ms"], r["surface"]["median_ms"]
                r["ratio"] = round(ms_s / ms_c, 4)
                r["closest"]["mrays_s"] = round(n / ms_c / 1e3, 1)
                r["surface"]["mrays_s"] = round(n / ms_s / 1e3, 1)
                r["surface"]["write_gb_s"] = round(n * RECORD_BYTES / ms_s / 1e6, 1)
                if ms_s > ms_c:
                    r["surface"]["extra_write_gb_s"] = round(n * (RECORD_BYTES - HIT_BYTES) / (ms_s - ms_c) / 1e6, 1)
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
    ap.add_argument("--batches", default="s0,shadow")
    ap.add_argument("--log2-rays", type=int, default=24)
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches: the median of at least 10 launches")
    batches = args.batches.split(",")
    if any(b not in ("s0", "shadow") for b in batches):
        ap.error("--batches: s0, shadow")
    if args.child:
        return child(args.child, args.log2_rays, args.launches, args.warmup, batches)
    from pooraytracer_amd import build
    build.build()
    out = {"log2_rays": args.log2_rays, "method": "median kernel_ms of alternating launches after warm-up; ratio = surface / closest",
           "scenes": {}}
    for name in args.scenes.split(","):
        if name not in WORKLOADS:
            ap.error(f"unknown scene {name}")
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", name,
               "--log2-rays", str(args.log2_rays), "--launches", str(args.launches), "--warmup", str(args.warmup), "--batches", args.batches]
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
