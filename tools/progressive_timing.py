"""Timing of progressive rendering (prt_accum_*) on one GPU; prints one JSON object.

  python tools/progressive_timing.py [--width 1024] [--ladder 10,50,100,500] [--reps 3]

On the bench's cornell-box frame (bench.py WORKLOADS["cornell-box"]: 1024^2, depth 20, seed 1):
  one_shot_s      prt_render_device of the ladder's last rung in one call (fp32 framebuffer, like bench.py), median
  ladder_s        the whole ladder on one accumulator: one pass per rung + one fp32 resolve per rung, median
  ladder_ratio    ladder_s / one_shot_s
  resolve_us      k_resolve alone (HIP events around back-to-back resolves): f32 output, and f64 + f32 + sRGB8 outputs,
                  with the bytes each moves and the GB/s that is
  accumulate      k_accumulate's bytes per pass (its time is in a kernel trace: rocprofv3 --kernel-trace --stats)
  preview         per-pass wall time (events around the pass: K3 + k_accumulate) and K3 time (prt_get_counters) of
                  1-, 4- and 16-sample passes, and the same per sample next to the one-shot frame's per-sample cost
Nothing is written; bench.py is not involved.
"""
import argparse
import statistics

from timing_common import event, load, write_result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--ladder", default="10,50,100,500")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from pooraytracer_amd import api, build
    build.build()
    ladder = [int(x) for x in args.ladder.split(",")]
    data, _ = load("cornell-box", width=args.width, height=args.width)
    cam = data.camera
    sc = api.Scene(data).upload(0)
    kw = dict(max_depth=args.depth, seed=1)
    shape = (cam.height, cam.width, 3)
    npx = cam.height * cam.width
    fb = torch.zeros(shape, dtype=torch.float32, device="cuda")
    f64 = torch.zeros(shape, dtype=torch.float64, device="cuda")
    u8 = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def timed(fn):
        a, b = event(), event()
        torch.cuda.synchronize()
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 1e3

    # one-shot frame at the last rung (warm-up call first)
    sc.render_device(None, fb.data_ptr(), stream=st, spp=ladder[-1], **kw)
    one = [timed(lambda: sc.render_device(None, fb.data_ptr(), stream=st, spp=ladder[-1], **kw)) for _ in range(args.reps)]
    one_shot = statistics.median(one)

    acc = api.Accumulator(sc, **kw)
    acc.add(1)  # warm-up
    acc.resolve(d_f32_ptr=fb.data_ptr(), stream=st)

    def run_ladder():
        done = 0
        for rung in ladder:
            acc.add(rung - done, stream=st)
            done = rung
            acc.resolve(d_f32_ptr=fb.data_ptr(), stream=st)

    lad = []
    for _ in range(args.reps):
        acc.reset()
        lad.append(timed(run_ladder))
    ladder_s = statistics.median(lad)
    passes = [b - a for a, b in zip([0] + ladder[:-1], ladder)]

    # resolve alone: many back-to-back launches between two events
    reps = 200

    def resolves(**outs):
        for _ in range(reps):
            acc.resolve(stream=st, **outs)

    r32 = timed(lambda: resolves(d_f32_ptr=fb.data_ptr())) / reps
    rall = timed(lambda: resolves(d_f64_ptr=f64.data_ptr(), d_f32_ptr=fb.data_ptr(), d_u8_ptr=u8.data_ptr())) / reps
    b32 = npx * 3 * (8 + 4)
    ball = npx * 3 * (8 + 8 + 4 + 1)

    # preview passes
    preview = {}
    per_sample_one_shot_ms = one_shot * 1e3 / ladder[-1]
    for n in (1, 4, 16):
        acc.reset()
        acc.add(n, stream=st)  # warm-up of this pass size
        walls, k3 = [], []
        for _ in range(max(3, args.reps)):
            walls.append(timed(lambda: acc.add(n, stream=st)))
            k3.append(sc.counters()["kernel_ms"])
        w = statistics.median(walls) * 1e3
        preview[str(n)] = {"pass_ms": round(w, 4), "k3_ms": round(statistics.median(k3), 4),
                           "ms_per_sample": round(w / n, 4),
                           "per_sample_vs_one_shot": round(w / n / per_sample_one_shot_ms, 3)}
    c = sc.counters()
    acc.close()
    out = {
        "scene": "cornell-box", "width": cam.width, "height": cam.height, "depth": args.depth, "ladder": ladder, "passes": passes,
        "reps": args.reps,
        "one_shot_s": round(one_shot, 5), "one_shot_all_s": [round(x, 5) for x in one],
        "ladder_s": round(ladder_s, 5), "ladder_all_s": [round(x, 5) for x in lad],
        "ladder_ratio": round(ladder_s / one_shot, 4),
        "resolve_us": {"f32": round(r32 * 1e6, 2), "f32_GBps": round(b32 / r32 / 1e9, 1),
                       "f64_f32_srgb8": round(rall * 1e6, 2), "f64_f32_srgb8_GBps": round(ball / rall / 1e9, 1)},
        "accumulate": {"bytes_per_pass_one_chunk": npx * 3 * (8 + 8 + 8),
                       "note": "reads each chunk's item partials (24 B per pixel per chunk) and reads + writes the sums"},
        "preview": preview,
        "last_pass_counters": {k: c[k] for k in ("samples", "rays_closest", "rays_shadow", "kernel_ms")},
    }
    write_result(out, "")  # nothing is written: the line is the result


if __name__ == "__main__":
    main()
