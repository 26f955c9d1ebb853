"""Cost of the radiance query (prt_ray_color_device) against the frame it can reproduce; prints one JSON object.

  python tools/ray_color_timing.py [--spp 16] [--chunks 2] [--size 1024] [--log2-probes 20] [--launches 11]
                                   [--out profiles/ray_color_timing.json]

The work runs in one child process under its own `timeout`; the child prints each figure as one JSON line as soon as it has
it, so what a failed child had measured is kept, and nothing more is started on the GPU after a failure
(tools/timing_common.py).  On the cornell box:
  A  camera   the size x size pinhole frame's own rays (pixel centres, Camera::Initialize / GetRay arithmetic in numpy) as a
              device-resident batch keyed j*W+i, through ray_color_device, against render_device of the same camera at the same
              spp and the same explicit sample_chunks, in fp64 and fp32.  The two calls alternate launch by launch after a
              warm-up of both; a figure is the median kernel_ms (hipEvents around K3) of --launches launches with min and max
              beside it.  `ratio` = batch / frame (above 1: what reading rays costs over evaluating a camera);
              `max_abs_diff` = the largest difference between the two fp64 results (rounding of the ray directions only).
  B  probes   2^log2-probes incoherent interior probe rays (origin uniform in the scene's box, direction uniform on the
              sphere) at the same spp, automatic chunking: median kernel_ms, rays and samples per second.
"""
import argparse
import sys

import timing_common as tc

SCENE = "cornell-box"  # the one child's scene
GROUPS = {"workload": ("workloads", "variant")}


def pixel_centre_rays(cam):
    """The camera's rays in pixel order (Camera.cpp:75-117), directions left unnormalised like the reference's."""
    import numpy as np
    from pooraytracer_amd import _abi
    W, H = cam.width, cam.height
    eye, look, up = (np.asarray(v, dtype=np.float64) for v in (cam.eye, cam.look_at, cam.up))
    el = eye - look
    focal = np.sqrt(el @ el)
    vh = 2.0 * np.tan(np.radians(cam.fovy) / 2.0) * focal
    vw = vh * (W / H)
    w = el / focal
    u = np.cross(up, w)
    u /= np.sqrt(u @ u)
    v = np.cross(w, u)
    du, dv = vw * u / W, vh * (-v) / H
    p00 = eye - focal * w - vw * u / 2.0 - vh * (-v) / 2.0 + 0.5 * (du + dv)
    k = np.arange(W * H)
    rays = np.zeros(W * H, dtype=_abi.RAY_DTYPE)
    rays["o"] = eye
    rays["d"] = p00 + (k % W)[:, None] * du + (k // W)[:, None] * dv - eye
    rays["tmin"], rays["tmax"] = 1e-4, np.inf
    return rays


def child(name, args):
    import numpy as np
    import torch
    from pooraytracer_amd import api, scenes
    data, _ = tc.load(name, width=args.size, height=args.size)
    cam = data.camera
    sc = api.Scene(data).upload(0)
    tc.emit(scene=data.name, n_tris=int(data.n_tris), size=args.size, spp=args.spp, launches=args.launches)

    def upload_rays(rays):
        return torch.from_numpy(rays.view(np.float64).reshape(-1, 8)).cuda()

    # ---- A: the frame's own rays
    rays = pixel_centre_rays(cam)
    n = int(rays.shape[0])
    d_r = upload_rays(rays)
    d_k = torch.arange(n, dtype=torch.int32, device="cuda")
    d_batch = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_frame = torch.zeros((cam.height, cam.width, 3), dtype=torch.float64, device="cuda")
    for prec, pname in ((0, "f64"), (1, "f32")):
        kw = dict(spp=args.spp, max_depth=10, seed=1, sample_chunks=args.chunks, precision=prec)
        frame = tc.launcher(sc, sc.render_device, d_frame.data_ptr(), None, **kw)
        batch = tc.launcher(sc, sc.ray_color_device, d_r.data_ptr(), n, d_batch.data_ptr(), None, d_keys_ptr=d_k.data_ptr(), **kw)
        t, c = tc.interleaved([("frame", frame), ("batch", batch)], args.launches, args.warmup)
        cf, cb = c["frame"], c["batch"]
        r = {"rays": n, "frame": tc.stats(t["frame"]), "batch": tc.stats(t["batch"]), "sample_chunks": args.chunks,
             "frame_rays_traced": int(cf["rays_closest"] + cf["rays_shadow"]), "batch_rays_traced": int(cb["rays_closest"] + cb["rays_shadow"]),
             "max_abs_diff": float((d_batch.reshape(-1) - d_frame.reshape(-1)).abs().max().item())}
        r["ratio"] = round(r["batch"]["median_ms"] / r["frame"]["median_ms"], 4)
        r["batch"]["msamples_s"] = round(n * args.spp / r["batch"]["median_ms"] / 1e3, 1)
        r["frame"]["msamples_s"] = round(n * args.spp / r["frame"]["median_ms"] / 1e3, 1)
        tc.emit(f"camera {pname}: x{r['ratio']}", workload="camera", variant=pname, result=r)
    del d_r, d_k, d_batch, d_frame

    # ---- B: incoherent interior probes
    n = 1 << args.log2_probes
    lo, hi = data.bounds()
    d_r = upload_rays(scenes.random_rays(n, lo, hi, seed=12345))
    d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    for prec, pname in ((0, "f64"), (1, "f32")):
        probes = tc.launcher(sc, sc.ray_color_device, d_r.data_ptr(), n, d_out.data_ptr(), None, spp=args.spp, max_depth=10, seed=1,
                             precision=prec)
        t, c = tc.interleaved([("probes", probes)], args.launches, args.warmup)
        c = c["probes"]
        r = {"rays": n, "probes": tc.stats(t["probes"]), "rays_traced": int(c["rays_closest"] + c["rays_shadow"]),
             "mean_radiance": float(d_out.mean().item())}
        r["probes"]["msamples_s"] = round(n * args.spp / r["probes"]["median_ms"] / 1e3, 1)
        r["probes"]["mrays_traced_s"] = round(r["rays_traced"] / r["probes"]["median_ms"] / 1e3, 1)
        tc.emit(f"probes {pname}: {r['probes']['median_ms']} ms", workload="probes", variant=pname, result=r)
    sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--log2-probes", type=int, default=20)
    tc.common_args(ap)
    args = ap.parse_args()
    if args.chunks < 1:
        ap.error("--chunks: explicit sample chunks, at least 1")
    if args.child:
        return child(args.child, args)
    from pooraytracer_amd import build
    build.build()
    res = tc.run_children(__file__, [SCENE], tc.flags(args, "spp", "chunks", "size", "log2_probes", "launches", "warmup"), None, GROUPS)
    out = {"method": "median kernel_ms of alternating launches after warm-up; ratio = ray batch / frame", **res.pop("scenes")[SCENE], **res}
    return tc.write_result(out, args.out)


if __name__ == "__main__":
    sys.exit(main())
