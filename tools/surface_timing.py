"""Cost of the surface query against the closest-hit query on identical ray batches; prints one JSON object.

  python tools/surface_timing.py [--scenes cornell-box,bathroom2,soup8m] [--batches s0,shadow] [--log2-rays 24]
                                 [--launches 11] [--out profiles/surface_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept (tools/timing_common.py).  Per scene, on the
device-resident batches of 2^log2-rays rays that tools/occlusion_timing.py uses:
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
import sys

import timing_common as tc

SCENES = ("cornell-box", "bathroom2", "soup8m")
GROUPS = {"batch": ("batches", "variant")}
RECORD_BYTES, HIT_BYTES = 192, 32


def child(name, args, batches):
    import numpy as np
    import torch
    from pooraytracer_amd import api, scenes
    data, device_bvh = tc.load(name)
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    n_max = 1 << args.log2_rays
    lo, hi = data.bounds()
    textured = torch.tensor([m.texture >= 0 and m.type in (0, 1, 5) for m in data.materials] + [False], device="cuda")  # [-1]: a miss
    tc.emit(n_tris=int(data.n_tris), launches=args.launches)
    d_h = torch.zeros((n_max, HIT_BYTES // 8), dtype=torch.float64, device="cuda")
    d_s = torch.zeros((n_max, RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
    for kind in batches:
        rays = scenes.shadow_segments(data, n_max, seed=777) if kind == "shadow" else scenes.random_rays(n_max, lo, hi, seed=12345)
        n = int(rays.shape[0])
        d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
        del rays
        for prec, pname in ((0, "f64"), (1, "f32")):
            for sort in (False, True):
                closest = tc.launcher(sc, sc.trace_closest_device, d_r.data_ptr(), n, d_h.data_ptr(), precision=prec, sort=sort)
                surface = tc.launcher(sc, sc.trace_surface_device, d_r.data_ptr(), n, d_s.data_ptr(), precision=prec, sort=sort)
                t, _ = tc.interleaved([("closest", closest), ("surface", surface)], args.launches, args.warmup)
                words = d_s.view(torch.int64)[:n]
                mat = d_s.view(torch.int32).reshape(n_max, RECORD_BYTES // 4)[:n, 42].long()
                r = {"rays": n, "closest": tc.stats(t["closest"]), "surface": tc.stats(t["surface"]),
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
                variant = pname + ("-sorted" if sort else "")
                tc.emit(f"{name} {kind} {variant}: x{r['ratio']}", batch=kind, variant=variant, result=r)
        del d_r
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--batches", default="s0,shadow")
    ap.add_argument("--log2-rays", type=int, default=24)
    tc.common_args(ap)
    args = ap.parse_args()
    batches = args.batches.split(",")
    if any(b not in ("s0", "shadow") for b in batches):
        ap.error("--batches: s0, shadow")
    if args.child:
        return child(args.child, args, batches)
    names = tc.scene_names(ap, args.scenes, SCENES)
    from pooraytracer_amd import build
    build.build()
    out = {"log2_rays": args.log2_rays, "method": "median kernel_ms of alternating launches after warm-up; ratio = surface / closest"}
    out.update(tc.run_children(__file__, names, tc.flags(args, "log2_rays", "launches", "warmup", "batches"), None, GROUPS))
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
