"""Cost of the any-hit occlusion query against the closest-hit query on identical ray batches; prints one JSON object.

  python tools/occlusion_timing.py [--scenes cornell-box,bathroom2,soup8m] [--log2-rays 24] [--launches 11]
                                   [--out profiles/occlusion_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept (tools/timing_common.py).  Per scene, on device-resident batches of
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
import sys

import timing_common as tc

SCENES = ("cornell-box", "bathroom2", "soup8m")  # the soup also through the sorted calls
GROUPS = {"batch": ("batches", "variant")}


def child(name, args):
    import numpy as np
    import torch
    from pooraytracer_amd import api, scenes
    data, device_bvh = tc.load(name)
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    n_max = 1 << args.log2_rays
    lo, hi = data.bounds()
    tc.emit(n_tris=int(data.n_tris), launches=args.launches)
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
            for sort in ((False, True) if name == "soup8m" else (False,)):
                closest = tc.launcher(sc, sc.trace_closest_device, d_r.data_ptr(), n, d_h.data_ptr(), precision=prec, sort=sort)
                occluded = tc.launcher(sc, sc.trace_occluded_device, d_r.data_ptr(), n, d_o.data_ptr(), precision=prec, sort=sort)
                t, _ = tc.interleaved([("closest", closest), ("occluded", occluded)], args.launches, args.warmup)
                prim = d_h.view(torch.int32).reshape(n_max, 8)[:n, 6]
                r = {"rays": n, "closest": tc.stats(t["closest"]), "occluded": tc.stats(t["occluded"]),
                     "occluded_fraction": round(float((d_o[:n] != 0).float().mean().item()), 4),
                     "mismatches": int(((prim >= 0) != (d_o[:n] != 0)).sum().item())}
                r["ratio"] = round(r["closest"]["median_ms"] / r["occluded"]["median_ms"], 4)
                r["closest"]["mrays_s"] = round(n / r["closest"]["median_ms"] / 1e3, 1)
                r["occluded"]["mrays_s"] = round(n / r["occluded"]["median_ms"] / 1e3, 1)
                if not sort:
                    cc, co = closest(count_work=True), occluded(count_work=True)
                    r["per_ray"] = {"closest": {"node_fetches": round(cc["node_fetches"] / n, 3), "tri_tests": round(cc["tri_tests"] / n, 3)},
                                    "occluded": {"node_fetches": round(co["node_fetches"] / n, 3), "tri_tests": round(co["tri_tests"] / n, 3)}}
                variant = pname + ("-sorted" if sort else "")
                tc.emit(f"{name} {kind} {variant}: x{r['ratio']}", batch=kind, variant=variant, result=r)
        del d_r
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--log2-rays", type=int, default=24)
    tc.common_args(ap)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    names = tc.scene_names(ap, args.scenes, SCENES)
    from pooraytracer_amd import build
    build.build()
    out = {"log2_rays": args.log2_rays, "method": "median kernel_ms of alternating launches after warm-up; ratio = closest / occluded"}
    out.update(tc.run_children(__file__, names, tc.flags(args, "log2_rays", "launches", "warmup"), None, GROUPS))
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
