"""Quality and cost of the a-trous denoiser (prt_render_features + prt_denoise) on one GPU; prints one JSON object.

  python tools/denoise_timing.py [--scenes cornell-box,veach-mis,bathroom2] [--ref-spp 8192] [--out profiles/denoise.json]
                                 [--no-profile]

Per scene (bench.py's configuration: cornell-box 1024^2 depth 20, veach-mis 1280x720 depth 100, bathroom2 1280x720 depth 50,
fp64):
  reference    a plain accumulator at --ref-spp samples, seed 2 (the "truth" the errors are measured against)
  frames       seed 1 at 4 / 16 / 64 spp: seconds of the samples (one pass, synchronised), relMSE raw and denoised with
               prt_denoise_defaults, and the seconds of the features (1 sample) and of the filter (hipEvent, synchronised)
  equal_time   the raw spp that reaches the denoised relMSE (relMSE * spp is constant for unbiased Monte Carlo, taken from
               the 64-spp raw point) and the seconds it would take, against the denoised frame's own seconds
  sweep        relMSE of the 16-spp frame denoised with each point of a small parameter grid (the defaults come from it)
  levels       hipEvent time of the filter at 1024^2 with 1..5 levels (per-level cost = the differences)
  kernels      with profiling (default): a separate child run under `rocprofv3 --kernel-trace --stats` of the feature pass and
               the filter at 1024^2, and the per-kernel average times from its stats file
relMSE = mean over pixels and channels of (x - ref)^2 / (ref^2 + 1e-2) (timing_common.rel_mse).
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

from timing_common import event as ev, load, rel_mse, spawn, write_result

DEPTH = {"cornell-box": 20, "veach-mis": 100, "bathroom2": 50}  # bench.py's path depths
SWEEP = [dict(iterations=it, sigma_color=sc, sigma_normal=sn) for it in (4, 5) for sc in (0.5, 1.0, 2.0, 4.0) for sn in (0.2, 0.5)]


def kernels_only():
    """The work the profiled child runs: features + filter on cornell-box 1024^2, a few times each."""
    import numpy as np
    import torch
    from pooraytracer_amd import api
    data, _ = load("cornell-box")
    cam = data.camera
    sc = api.Scene(data).upload(0)
    H, W = cam.height, cam.width
    dev = torch.device("cuda", 0)
    al, nr = (torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
    dp = torch.empty((H, W), dtype=torch.float32, device=dev)
    rgb = torch.from_numpy(sc.render(spp=4, max_depth=20, seed=1).astype(np.float32)).to(dev)
    out = torch.empty_like(rgb)
    for _ in range(5):
        sc.features_device(al.data_ptr(), nr.data_ptr(), dp.data_ptr(), None, max_depth=20, seed=1)
        sc.denoise_device(W, H, rgb.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)


def profile_kernels():
    d = tempfile.mkdtemp(prefix="dn_prof_")
    rc, _ = spawn([os.path.abspath(__file__), "--kernels-only"], 600,
                  wrap=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "dn", "--"])
    res = {"returncode": rc}
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        res["error"] = "no kernel_stats.csv under " + d
        return res
    with open(stats[0]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for key in ("k_features", "k_dn_pack", "k_dn_level", "k_render"):
                if key in name:
                    res[key] = {"calls": int(row.get("Calls", 0)), "avg_us": round(float(row.get("AverageNs", 0)) / 1e3, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis,bathroom2")
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--spps", default="4,16,64")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only()
    import numpy as np
    import torch
    from pooraytracer_amd import api, build
    build.build()
    defaults = api.denoise_defaults()
    out = {"ref_spp": args.ref_spp, "defaults": defaults, "scenes": {}}
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
        dev = torch.device("cuda", 0)
        al, nr = (torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in range(2))
        dp = torch.empty((H, W), dtype=torch.float32, device=dev)
        den = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        sc.features_device(al.data_ptr(), nr.data_ptr(), dp.data_ptr(), None, max_depth=depth, seed=1)  # warm-up
        torch.cuda.synchronize()
        a, b = ev(), ev()
        a.record()
        sc.features_device(al.data_ptr(), nr.data_ptr(), dp.data_ptr(), None, max_depth=depth, seed=1)
        b.record()
        torch.cuda.synchronize()
        res["features_ms"] = round(a.elapsed_time(b), 4)
        frames = {}
        for spp in [int(s) for s in args.spps.split(",")]:
            with api.Accumulator(sc, max_depth=depth, seed=1) as acc:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                acc.add(spp)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                raw = acc.image()
                f32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
                acc.resolve(d_f32_ptr=f32.data_ptr())
                torch.cuda.synchronize()
                a, b = ev(), ev()
                a.record()
                sc.denoise_device(W, H, f32.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), den.data_ptr())
                b.record()
                torch.cuda.synchronize()
                img = den.cpu().numpy()
                r = {"s": round(dt, 4), "rel_mse_raw": rel_mse(raw, ref), "rel_mse_denoised": rel_mse(img, ref),
                     "filter_ms": round(a.elapsed_time(b), 4)}
                r["ratio"] = round(r["rel_mse_denoised"] / r["rel_mse_raw"], 4)
                if spp == 16:
                    sweep = []
                    for p in SWEEP:
                        sc.denoise_device(W, H, f32.data_ptr(), al.data_ptr(), nr.data_ptr(), dp.data_ptr(), den.data_ptr(), **p)
                        torch.cuda.synchronize()
                        sweep.append(dict(p, rel_mse=rel_mse(den.cpu().numpy(), ref)))
                    res["sweep_16spp"] = sweep
                frames[spp] = r
        top = max(frames)
        per_spp_s = frames[top]["s"] / top
        for spp, r in frames.items():
            eq_spp = top * frames[top]["rel_mse_raw"] / r["rel_mse_denoised"]
            r["equal_time"] = {"raw_spp_same_rel_mse": round(eq_spp, 1), "raw_s": round(eq_spp * per_spp_s, 4),
                               "denoised_s": round(r["s"] + (res["features_ms"] + r["filter_ms"]) * 1e-3, 4)}
        res["frames"] = frames
        out["scenes"][name] = res
        sc.close()
        print(json.dumps({name: res}), file=sys.stderr, flush=True)
    # per-level cost at 1024^2 (cornell-box features, a 4-spp frame)
    data, _ = load("cornell-box")
    sc = api.Scene(data).upload(0)
    rgb = sc.render(spp=4, max_depth=20, seed=1).astype(np.float32)
    feat = {k: torch.from_numpy(v).cuda() for k, v in sc.features(max_depth=20, seed=1).items() if k != "prim"}
    x = torch.from_numpy(rgb).cuda()
    y = torch.empty_like(x)
    levels = {}
    for it in range(1, 6):
        ts = []
        for _ in range(6):
            a, b = ev(), ev()
            a.record()
            sc.denoise_device(1024, 1024, x.data_ptr(), feat["albedo"].data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr(),
                              y.data_ptr(), iterations=it)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        levels[it] = round(sorted(ts)[len(ts) // 2], 4)
    out["filter_ms_by_levels_1024"] = levels
    sc.close()
    # the default parameters' rank in the sweep (mean log relMSE over the scenes)
    keys = [tuple(sorted((k, v) for k, v in p.items())) for p in SWEEP]
    score = {k: float(np.mean([np.log(s["sweep_16spp"][i]["rel_mse"]) for s in out["scenes"].values() if "sweep_16spp" in s]))
             for i, k in enumerate(keys)}
    out["sweep_best"] = dict(min(score, key=score.get))
    if not args.no_profile:
        out["kernels"] = profile_kernels()
    write_result(out, args.out)


if __name__ == "__main__":
    main()
