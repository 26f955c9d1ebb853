"""Timing and error of adaptive sampling (prt_accum_*_adaptive) against uniform sampling on one GPU; prints one JSON object.

  python tools/adaptive_timing.py [--scenes cornell-box,veach-mis] [--ref-spp 8192] [--out profiles/adaptive_timing.json]

Per scene (bench.py's configuration: cornell-box 1024^2 depth 20, veach-mis 1280x720 depth 100, seed 1, fp64):
  reference     a plain accumulator at --ref-spp samples (the "truth" the errors are measured against)
  uniform       spp 64 / 256 / 1024 on a plain accumulator: seconds (one pass, synchronised), total samples, relMSE
  adaptive      a rel_tol sweep at --rel-batch samples per batch, then a batch sweep (4, 8, 16, 32) at one rel_tol: seconds of the
                whole run (rounds of --round samples, min_spp --min-spp, max_spp --max-spp, abs_tol 0), total samples,
                relMSE, n_active per round; and from a second, instrumented run (synchronised after each round): the
                K3 time (prt_get_counters) against the rest of the round (select + read-back + accumulate + launch gaps),
                and how much of the time the rounds with fewer than 10 % of the pixels active take (the tail)
  equal_time    relMSE of uniform sampling at the adaptive run's time, from the uniform point nearest in time
                (relMSE * seconds is constant for unbiased Monte Carlo); ratio < 1 means adaptive wins
relMSE = mean over pixels and channels of (x - ref)^2 / (ref^2 + 1e-2).  Nothing else is written; bench.py is not involved.
"""
import argparse
import json
import sys
import time

from timing_common import load, rel_mse, write_result

DEPTH = {"cornell-box": 20, "veach-mis": 100}  # bench.py's path depths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--uniform", default="64,256,1024")
    ap.add_argument("--rel-tols", default="0.2,0.1,0.05,0.03")
    ap.add_argument("--rel-batch", type=int, default=16)  # the batch of profiles/adaptive_timing.json's rel_tol sweep
    ap.add_argument("--batches", default="4,8,16,32")
    ap.add_argument("--batch-sweep-rel", type=float, default=0.05)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--max-spp", type=int, default=4096)
    ap.add_argument("--round", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from pooraytracer_amd import api, build
    build.build()
    out = {"ref_spp": args.ref_spp, "min_spp": args.min_spp, "max_spp": args.max_spp, "round": args.round, "scenes": {}}
    for name in args.scenes.split(","):
        depth = DEPTH[name]
        data, _ = load(name)
        cam = data.camera
        npx = cam.width * cam.height
        sc = api.Scene(data).upload(0)
        kw = dict(max_depth=depth, seed=1)
        res = {"width": cam.width, "height": cam.height, "depth": depth}
        t0 = time.perf_counter()
        with api.Accumulator(sc, **kw) as acc:
            for _ in range(args.ref_spp // 1024):
                acc.add(1024)
            ref = acc.image()
        res["reference_s"] = round(time.perf_counter() - t0, 3)
        with api.Accumulator(sc, **kw) as acc:  # warm-up: first launches, kernel loading
            acc.add(16)
            torch.cuda.synchronize()
        uni = {}
        for spp in [int(s) for s in args.uniform.split(",")]:
            with api.Accumulator(sc, seed=7, max_depth=depth) as acc:  # another seed: independent of the reference
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                acc.add(spp)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                uni[spp] = {"s": round(dt, 4), "samples": spp * npx, "rel_mse": rel_mse(acc.image(), ref)}
        res["uniform"] = uni

        def equal_time(dt, err):
            spp = min(uni, key=lambda s: abs(np.log(uni[s]["s"] / dt)))
            u = uni[spp]["rel_mse"] * uni[spp]["s"] / dt
            return {"uniform_rel_mse": u, "ratio": err / u, "from_uniform_spp": spp}

        def adaptive(rel, batch):
            a = dict(rel_tol=rel, abs_tol=0.0, min_spp=args.min_spp, max_spp=args.max_spp, batch=batch)
            with api.AdaptiveAccumulator(sc, seed=7, max_depth=depth, **a) as acc:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hist = []
                acc.run(args.round, on_round=lambda k, n: hist.append(k))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                img, cnt = acc.image(), acc.pixel_samples()
            r = {"rel_tol": rel, "batch": batch, "s": round(dt, 4), "samples": int(cnt.astype(np.int64).sum()),
                 "mean_spp": round(float(cnt.mean()), 1), "rel_mse": rel_mse(img, ref), "rounds": len(hist), "n_active": hist}
            r["equal_time"] = equal_time(dt, r["rel_mse"])
            # instrumented repeat: per-round wall time (synchronised) against K3's own time
            k3 = wall = tail = 0.0
            with api.AdaptiveAccumulator(sc, seed=7, max_depth=depth, **a) as acc:
                while True:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    k = acc.step(args.round)
                    torch.cuda.synchronize()
                    dt1 = time.perf_counter() - t0
                    if k == 0:
                        wall += dt1
                        break
                    k3 += sc.counters()["kernel_ms"] * 1e-3  # the round's last K3 launch (all of it up to 64 batches a round)
                    wall += dt1
                    if k < 0.1 * npx:
                        tail += dt1
            r["instrumented"] = {"wall_s": round(wall, 4), "k3_s": round(k3, 4), "other_s": round(wall - k3, 4),
                                 "tail_s_below_10pct_active": round(tail, 4)}
            return r

        res["adaptive_rel_tol"] = [adaptive(float(r), args.rel_batch) for r in args.rel_tols.split(",")]
        res["adaptive_batch"] = [adaptive(args.batch_sweep_rel, int(b)) for b in args.batches.split(",")]
        out["scenes"][name] = res
        sc.close()
        print(json.dumps({name: res}), file=sys.stderr, flush=True)
    write_result(out, args.out)


if __name__ == "__main__":
    main()
