"""numpy float64 restatement of the feature buffers and the a-trous filter of include/prt.h (prt_render_features,
prt_denoise).  The device computes the filter in fp32, so the two agree within rounding (about 1e-6 relative), not bit
for bit; the features agree to the fp32 rounding of the fp64 values."""
import numpy as np

EPS = 1e-3  # demodulation floor
B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
MAT_LAMBERTIAN, MAT_PHONG, MAT_DEBUG = 0, 1, 5


def _inv2(s):
    """1 / s^2, or 0 (term off) for s <= 0 or +inf."""
    s = float(s)
    return 0.0 if not (0.0 < s < np.inf) else min(1.0 / (s * s), 3.4e38)


def atrous(rgb, albedo, normal, depth, iterations=5, demodulate=1, sigma_color=1.0, sigma_normal=0.5, sigma_depth=0.1,
           sigma_albedo=0.1, **_):
    """The filter of prt_denoise in float64.  rgb / albedo / normal (H, W, 3), depth (H, W); returns (H, W, 3)."""
    c = np.asarray(rgb, np.float64)
    if iterations == 0:
        return c.copy()
    a = np.asarray(albedo, np.float64)
    n = np.asarray(normal, np.float64)
    z = np.asarray(depth, np.float64)
    H, W = c.shape[:2]
    mod = np.fmax(a, EPS)
    if demodulate:
        c = c / mod
    i_n, i_z, i_a = _inv2(sigma_normal), _inv2(sigma_depth), _inv2(sigma_albedo)
    hit = np.isfinite(z)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iz_p = i_z / (z * z)
    for lv in range(iterations):
        step = 1 << lv
        i_c = _inv2(float(sigma_color) * 2.0 ** -lv)
        fin_p = np.isfinite(c).all(-1)
        num = np.zeros_like(c)
        den = np.zeros((H, W))
        for j in range(5):
            dy = (j - 2) * step
            for i in range(5):
                dx = (i - 2) * step
                # the tap q = (x + dx, y + dy) of every centre p whose tap lies inside the image
                ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H - max(0, dy))
                xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W - max(0, dx))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                cq, cp = c[ys, xs], c[yd, xd]
                ok = np.isfinite(cq).all(-1)
                e = np.zeros(ok.shape)
                with np.errstate(invalid="ignore", over="ignore"):
                    if i_c > 0:
                        e += ((cp - cq) ** 2).sum(-1) * i_c
                    if i_n > 0:
                        e += ((n[yd, xd] - n[ys, xs]) ** 2).sum(-1) * i_n
                    if i_a > 0:
                        e += ((a[yd, xd] - a[ys, xs]) ** 2).sum(-1) * i_a
                    if i_z > 0:
                        hp, hq = hit[yd, xd], hit[ys, xs]
                        ok &= hp == hq
                        dz = z[yd, xd] - z[ys, xs]
                        both = hp & hq & (dz != 0)
                        e = np.where(both, e + np.where(both, dz * dz, 0.0) * np.where(both, iz_p[yd, xd], 0.0), e)
                    w = np.where(ok, B3[i] * B3[j] * np.exp(-e), 0.0)
                    num[yd, xd] += w[..., None] * np.where(ok[..., None], cq, 0.0)
                    den[yd, xd] += w
        with np.errstate(invalid="ignore", divide="ignore"):
            out = num / den[..., None]
        c = np.where(fin_p[..., None], out, 0.0)
    return c * mod if demodulate else c


def b3_convolution(rgb, iterations):
    """The filter with every sigma off: `iterations` dilated B3 convolutions, renormalised at the border (taps outside the
    image skipped) — written as explicit loops over pixels and taps."""
    c = np.asarray(rgb, np.float64).copy()
    H, W = c.shape[:2]
    for lv in range(iterations):
        s = 1 << lv
        out = np.zeros_like(c)
        for y in range(H):
            for x in range(W):
                acc, wsum = np.zeros(3), 0.0
                for j in range(5):
                    for i in range(5):
                        yy, xx = y + (j - 2) * s, x + (i - 2) * s
                        if 0 <= yy < H and 0 <= xx < W:
                            acc += B3[i] * B3[j] * c[yy, xx]
                            wsum += B3[i] * B3[j]
                out[y, x] = acc / wsum
        c = out
    return c


def camera_setup(cam):
    """Camera::Initialize (Camera.cpp:75-106) as the library computes it: center, pixel00, du, dv."""
    W, H = max(1, cam.width), max(1, cam.height)
    eye, look, up = (np.array(v, np.float64) for v in (cam.eye, cam.look_at, cam.up))
    el = eye - look
    focal = np.sqrt(np.dot(el, el))
    h = np.tan(cam.fovy * 0.01745329251994329576923690768489 / 2.0)
    vh = 2.0 * h * focal
    vw = vh * (W / H)

    def unit(v):
        return v / np.sqrt(np.dot(v, v))
    w = unit(el)
    u = unit(np.cross(up, w))
    v = np.cross(w, u)
    vu, vv = vw * u, vh * -v
    du, dv = vu / W, vv / H
    ul = eye - focal * w - vu / 2.0 - vv / 2.0
    return eye, ul + 0.5 * (du + dv), du, dv


def jittered_rays(cam, seed, sample, rng_stream, pixels=None):
    """Directions of sample `sample` of every pixel with pixel_jitter on: (H, W, 3); or, with pixels = (N, 2) (x, y)
    pairs, of those pixels only: (N, 3).  rng_stream(seed, pixel, sample, n) is the library's keyed stream
    (oracle.rng_stream); offset.y is the first number, offset.x the second."""
    center, p00, du, dv = camera_setup(cam)
    if pixels is None:
        pixels = np.stack(np.meshgrid(np.arange(cam.width), np.arange(cam.height)), -1).reshape(-1, 2)
        shape = (cam.height, cam.width, 3)
    else:
        shape = (len(pixels), 3)
    d = np.zeros((len(pixels), 3))
    for k, (x, y) in enumerate(np.asarray(pixels, np.int64)):
        r = rng_stream(seed, y * cam.width + x, sample, 2)
        fy, fx = y + (r[0] - 0.5), x + (r[1] - 0.5)
        d[k] = p00 + fx * du + fy * dv - center
    return d.reshape(shape)


def hit_features(data, rays_d, hits, texture_value=None):
    """Features of one traced sample per pixel: rays_d (N, 3) directions, hits (N,) PrtHit records of those rays.
    texture_value(texture, uv) -> (n, 3): the scene's Kd map lookup (oracle.texture_value).  Returns albedo (N, 3),
    normal (N, 3), depth (N,) in float64 (miss: (1,1,1), 0, +inf)."""
    d = np.asarray(rays_d, np.float64).reshape(-1, 3)
    N = d.shape[0]
    albedo, normal, depth = np.ones((N, 3)), np.zeros((N, 3)), np.full(N, np.inf)
    prim = hits["prim"]
    hit = prim >= 0
    if not hit.any():
        return albedo, normal, depth
    first = np.asarray(data.mesh_first_tri, np.int64)
    mesh = np.searchsorted(first, prim[hit], side="right") - 1
    mats = np.asarray(data.mesh_material)[mesh]
    V = np.asarray(data.vertices, np.float64)[prim[hit]]
    gn = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    gn /= np.linalg.norm(gn, axis=1, keepdims=True)
    dh = d[hit]
    front = (dh * gn).sum(1) < 0
    normal[hit] = np.where(front[:, None], gn, -gn)
    depth[hit] = hits["t"][hit] * np.sqrt((dh * dh).sum(1))
    al, be = hits["alpha"][hit], hits["beta"][hit]
    if data.texcoords is not None:
        T = np.asarray(data.texcoords, np.float64)[prim[hit]]
        w0 = 1.0 - al - be
        uv = w0[:, None] * T[:, 0] + al[:, None] * T[:, 1] + be[:, None] * T[:, 2]
    else:
        uv = np.zeros((al.size, 2))
    alb = np.ones((al.size, 3))
    for k, mi in enumerate(mats):
        m = data.materials[mi]
        if m.type in (MAT_LAMBERTIAN, MAT_DEBUG, MAT_PHONG):
            kd = np.array(m.kd, np.float64)
            ks = np.array(m.ks, np.float64)
            if m.texture >= 0:
                kd = ks = texture_value(m.texture, uv[k:k + 1])[0]
            alb[k] = kd + ks if m.type == MAT_PHONG else kd
    albedo[hit] = alb
    return albedo, normal, depth


def mean_features(per_sample):
    """Means of a list of (albedo, normal, depth) per sample, as prt.h states them: albedo and normal over all samples,
    depth over the samples that hit (+inf if none did).  Returns float64 arrays."""
    a = np.mean([s[0] for s in per_sample], axis=0)
    n = np.mean([s[1] for s in per_sample], axis=0)
    z = np.array([s[2] for s in per_sample])
    hit = np.isfinite(z)
    cnt = hit.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        zm = np.where(cnt > 0, np.where(hit, z, 0.0).sum(0) / np.maximum(cnt, 1), np.inf)
    return a, n, zm


def rel_mse(img, ref, eps=1e-2):
    """relMSE as tools/adaptive_timing.py defines it: mean over pixels and channels of (x - r)^2 / (r^2 + eps)."""
    img, ref = np.asarray(img, np.float64), np.asarray(ref, np.float64)
    return float(np.mean((img - ref) ** 2 / (ref ** 2 + eps)))
