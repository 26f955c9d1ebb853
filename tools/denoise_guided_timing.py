"""Quality and cost of the variance-guided a-trous filter (prt_accum_variance + prt_denoise_guided) against the plain one
on one GPU; prints one JSON object.

  python tools/denoise_guided_timing.py [--scenes cornell-box,veach-mis,bathroom2] [--ref-spp 8192]
                                        [--out profiles/denoise_guided.json]

Per scene (bench.py's configuration: cornell-box 1024^2 depth 20, veach-mis 1280x720 depth 100, bathroom2 1280x720 depth 50,
fp64):
  reference    a plain accumulator at --ref-spp samples, seed 2
  frames       seed 1 at 16 / 64 spp, sampled uniformly through an adaptive accumulator with min_spp == max_spp and batch 4
               (bit for bit a uniform render, and it keeps the moments): relMSE raw, denoised with prt_denoise_defaults and
               denoised with prt_denoise_guided_defaults
  sweep        relMSE of the guided filter at sigma_color in {1, 2, 4, 8} x levels in {4, 5}, per frame
  sweep_best   the point with the lowest mean log relMSE over the scenes and both sample counts (the rule the plain
               defaults were chosen by): what prt_denoise_guided_defaults should be
  timing       hipEvent medians at 1024^2 (cornell-box): the guided filter by levels, the plain filter at the same levels,
               and k_accum_variance
relMSE = mean over pixels and channels of (x - ref)^2 / (ref^2 + 1e-2) (timing_common.rel_mse).
"""
import argparse
import json
import sys
import time

from timing_common import event as ev, load, rel_mse, write_result

DEPTH = {"cornell-box": 20, "veach-mis": 100, "bathroom2": 50}  # bench.py's path depths
SWEEP = [dict(iterations=it, sigma_color=sc) for it in (4, 5) for sc in (1.0, 2.0, 4.0, 8.0)]
BATCH = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis,bathroom2")
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--spps", default="16,64")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from pooraytracer_amd import api, build
    build.build()
    out = {"ref_spp": args.ref_spp, "batch": BATCH, "plain_defaults": api.denoise_defaults(),
           "guided_defaults": api.denoise_guided_defaults(), "scenes": {}}
    dev = torch.device("cuda", 0)
    spps = [int(s) for s in args.spps.split(",")]
    for name in args.scenes.split(","):
        depth = DEPTH[name]
        data, _ = load(name)
        cam = data.camera
        H, W = cam.height, cam.width
        sc = api.Scene(data).upload(0)
        res = {"width": W, "height": H, "depth": depth}
        t0 = time.perf_counter()
        with api.Accumulator(sc, max_depth=depth, seed=2) as acc:
            for _ in range(max(1, args.ref_spp // 1024)):
                acc.add(min(1024, args.ref_spp))
            ref = acc.image()
        res["reference_s"] = round(time.perf_counter() - t0, 3)
        al, nr = (torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
        dp = torch.empty((H, W), dtype=torch.float32, device=dev)
        den = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        var = torch.empty((H, W), dtype=torch.float32, device=dev)
        f32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        sc.features_device(al.data_ptr(), nr.data_ptr(), dp.data_ptr(), None, max_depth=depth, seed=1)
        frames = {}
        for spp in spps:
            with api.AdaptiveAccumulator(sc, rel_tol=0.0, abs_tol=0.0, min_spp=spp, max_spp=spp, batch=BATCH, max_depth=depth,
                                         seed=1) as acc:
                acc.run(spp)
                raw = acc.image()
                acc.resolve(d_f32_ptr=f32.data_ptr())
                acc.variance(d_f32_ptr=var.data_ptr())
                torch.cuda.synchronize()
            v = var.cpu().numpy()
            r = {"rel_mse_raw": rel_mse(raw, ref), "variance_mean": float(v.mean()), "variance_max": float(v.max())}
            sc.denoise_device(W, H, f32.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), den.data_ptr())
            torch.cuda.synchronize()
            r["rel_mse_plain"] = rel_mse(den.cpu().numpy(), ref)
            sc.denoise_guided_device(W, H, f32.data_ptr(), var.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), den.data_ptr())
            torch.cuda.synchronize()
            r["rel_mse_guided"] = rel_mse(den.cpu().numpy(), ref)
            r["plain_over_raw"] = round(r["rel_mse_plain"] / r["rel_mse_raw"], 4)
            r["guided_over_raw"] = round(r["rel_mse_guided"] / r["rel_mse_raw"], 4)
            sweep = []
            for p in SWEEP:
                sc.denoise_guided_device(W, H, f32.data_ptr(), var.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(),
                                         den.data_ptr(), **p)
                torch.cuda.synchronize()
                sweep.append(dict(p, rel_mse=rel_mse(den.cpu().numpy(), ref)))
            r["sweep"] = sweep
            frames[spp] = r
        res["frames"] = frames
        out["scenes"][name] = res
        sc.close()
        print(json.dumps({name: res}), file=sys.stderr, flush=True)
    score = [float(np.mean([np.log(f["sweep"][i]["rel_mse"]) for s in out["scenes"].values() for f in s["frames"].values()]))
             for i in range(len(SWEEP))]
    out["sweep_mean_log_rel_mse"] = [dict(p, score=round(s, 5)) for p, s in zip(SWEEP, score)]
    out["sweep_best"] = SWEEP[int(np.argmin(score))]
    # cost at 1024^2: cornell-box, a 16-spp frame and its variance
    data, _ = load("cornell-box")
    sc = api.Scene(data).upload(0)
    feat = {k: torch.from_numpy(v).to(dev) for k, v in sc.features(max_depth=20, seed=1).items() if k != "prim"}
    x = torch.empty((1024, 1024, 3), dtype=torch.float32, device=dev)
    v = torch.empty((1024, 1024), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)

    def median_ms(fn, n=7):
        ts = []
        for _ in range(n):
            a, b = ev(), ev()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return round(sorted(ts)[len(ts) // 2], 4)
    with api.AdaptiveAccumulator(sc, rel_tol=0.0, abs_tol=0.0, min_spp=16, max_spp=16, batch=BATCH, max_depth=20, seed=1) as acc:
        acc.run(16)
        acc.resolve(d_f32_ptr=x.data_ptr())
        acc.variance(d_f32_ptr=v.data_ptr())
        torch.cuda.synchronize()
        timing = {"accum_variance_ms": median_ms(lambda: acc.variance(d_f32_ptr=v.data_ptr()))}
    ptrs = (feat["albedo"].data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr())
    timing["guided_ms_by_levels"] = {it: median_ms(lambda: sc.denoise_guided_device(1024, 1024, x.data_ptr(), v.data_ptr(), *ptrs, y.data_ptr(),
                                                                                       iterations=it)) for it in range(1, 6)}
    timing["plain_ms_by_levels"] = {it: median_ms(lambda: sc.denoise_device(1024, 1024, x.data_ptr(), *ptrs, y.data_ptr(), iterations=it))
                                    for it in range(1, 6)}
    out["timing_1024"] = timing
    sc.close()
    write_result(out, args.out)


if __name__ == "__main__":
    main()
