"""Cost of the multi-hit query against the closest-hit query on identical ray batches; prints one JSON object.

  python tools/multi_hit_timing.py [--scenes cornell-box,bathroom2,soup1m] [--log2-rays 24] [--launches 11]
                                   [--out profiles/multi_hit_timing.json]

Every scene is one child process under its own `timeout` (the scene is built and uploaded once per child); the first
child that fails ends the run (nothing more is started on the GPU after a fault).  A child prints each figure as one JSON
line as soon as it has it, so what a failed child had measured is kept (tools/timing_common.py).  Per scene, on one
device-resident batch of 2^log2-rays S0 rays (origin uniform in the scene's box, direction uniform on the sphere,
tmax = inf), in fp64 and fp32:
  closest      trace_closest_device: one hit per ray
  multi[k]     trace_multi_device, k = 1, 2, 4, 8: ONE call
  peel[k]      the only way to the first k hits without the multi-hit call: k calls of trace_closest_device, tmin of
               every ray moved to the float just past its previous t between them (a ray that missed gets tmin = inf).  The
               figure is the sum of the k launches' kernel_ms; the pass that moves tmin is not charged.  A peel drops every
               hit that ties its predecessor's t exactly: `peel_short[k]` is the share of rays whose peel holds fewer hits
               than the multi-hit list.
The three forms take turns repetition by repetition after a warm-up; a figure is the median kernel_ms (hipEvents around
the launch) of --launches repetitions, with min and max beside it.  `multi_over_closest[k]` = multi[k] / closest (above 1:
the list costs more than one closest hit), `peel_over_multi[k]` = peel[k] / multi[k] (above 1: the one call wins).  One
counting launch of closest and of multi[8] gives the node fetches and triangle tests per ray; `hits_per_ray` is the mean
number of non-miss records of multi[8].
"""
import argparse
import sys

import timing_common as tc

SCENES = ("cornell-box", "bathroom2", "soup1m")
GROUPS = {"variant": "variants"}
KS = (1, 2, 4, 8)


def child(name, args):
    import numpy as np
    import torch
    from pooraytracer_amd import api, scenes
    data, device_bvh = tc.load(name)
    sc = api.Scene(data, device_bvh=device_bvh).upload(0)
    n = 1 << args.log2_rays
    lo, hi = data.bounds()
    tc.emit(n_tris=int(data.n_tris), launches=args.launches, rays=n)
    rays = scenes.random_rays(n, lo, hi, seed=12345)
    d_r = torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()
    del rays
    d_p = d_r.clone()  # the peel's rays: column 3 is tmin
    d_h = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d_m = torch.zeros((n * KS[-1], 4), dtype=torch.float64, device="cuda")
    inf = torch.tensor(float("inf"), dtype=torch.float64, device="cuda")

    def prims(buf, rows, k):
        return buf.view(torch.int32).reshape(-1, 8)[:rows * k, 6].reshape(rows, k)

    for prec, pname in ((0, "f64"), (1, "f32")):
        closest = tc.launcher(sc, sc.trace_closest_device, d_r.data_ptr(), n, d_h.data_ptr(), precision=prec)
        peel_step = tc.launcher(sc, sc.trace_closest_device, d_p.data_ptr(), n, d_h.data_ptr(), precision=prec)
        multi = {k: tc.launcher(sc, sc.trace_multi_device, d_r.data_ptr(), n, k, d_m.data_ptr(), precision=prec) for k in KS}

        def peel():
            """kernel_ms of each of the KS[-1] steps, and the number of hits every ray has after each."""
            d_p[:, 3] = d_r[:, 3]
            ms, found = [], torch.zeros(n, dtype=torch.int32, device="cuda")
            counts = []
            for _ in range(KS[-1]):
                ms.append(peel_step()["kernel_ms"])
                hit = prims(d_h, n, 1)[:, 0] >= 0
                found += hit.to(torch.int32)
                counts.append(found.clone())
                t = d_h[:, 0]
                past = torch.nextafter(t.float(), inf.float()).double() if prec else torch.nextafter(t, inf)  # the next t of the kernel's format
                d_p[:, 3] = torch.where(hit, past, inf)
            return {"kernel_ms": ms, "counts": counts}

        # the forms take turns: closest, multi[1..8], the peel
        t, last = tc.interleaved([("closest", closest)] + [(k, multi[k]) for k in KS] + [("peel", peel)], args.launches, args.warmup)
        counts = last["peel"]["counts"]
        r = {"closest": tc.stats(t["closest"]), "multi": {}, "peel": {}, "multi_over_closest": {}, "peel_over_multi": {}, "peel_short": {}}
        for k in KS:
            multi[k]()
            listed = (prims(d_m, n, k) >= 0).sum(1).to(torch.int32)
            r["multi"][k], r["peel"][k] = tc.stats(t[k]), tc.stats([sum(ms[:k]) for ms in t["peel"]])
            r["multi_over_closest"][k] = round(r["multi"][k]["median_ms"] / r["closest"]["median_ms"], 4)
            r["peel_over_multi"][k] = round(r["peel"][k]["median_ms"] / r["multi"][k]["median_ms"], 4)
            r["peel_short"][k] = round(float((counts[k - 1] < listed).float().mean().item()), 6)
            if k == KS[-1]:
                r["hits_per_ray"] = round(float(listed.float().mean().item()), 3)
        cc, cm = closest(count_work=True), multi[KS[-1]](count_work=True)
        r["per_ray"] = {"closest": {"node_fetches": round(cc["node_fetches"] / n, 3), "tri_tests": round(cc["tri_tests"] / n, 3)},
                        "multi8": {"node_fetches": round(cm["node_fetches"] / n, 3), "tri_tests": round(cm["tri_tests"] / n, 3)}}
        tc.emit(f"{name} {pname}: multi/closest {r['multi_over_closest']}, peel/multi {r['peel_over_multi']}", variant=pname, result=r)
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
    out = {"log2_rays": args.log2_rays,
           "method": "median kernel_ms of alternating launches after warm-up; peel[k] = sum of k closest-hit launches with tmin advanced"}
    out.update(tc.run_children(__file__, names, tc.flags(args, "log2_rays", "launches", "warmup"), None, GROUPS))
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
