"""numpy float64 restatement of the variance-guided a-trous filter and the variance AOV of include/prt.h
(prt_denoise_guided, prt_accum_variance).  The device computes the filter in fp32, so the two agree within rounding; the
variance AOV is fp64 arithmetic without fused multiply-adds on both sides, so its fp32 rounding agrees bit for bit."""
import numpy as np

from tests import adaptive_model
from tests import denoise_model
from tests.denoise_model import B3, EPS, _inv2

B1 = np.array([1.0, 2.0, 1.0])  # the 3x3 variance blur, per axis (renormalised over the taps inside the image)


def luma(rgb):
    return adaptive_model.luma(rgb)


def accum_variance(sums, moments, counts, batch):
    """prt_accum_variance: the batch-means variance of each pixel's mean luminance as fp32; 0 where the count is 0."""
    counts = np.asarray(counts)
    with np.errstate(all="ignore"):
        v = adaptive_model.estimate(np.asarray(sums), np.asarray(moments), counts, batch)[1] / counts
    return np.where(counts == 0, 0.0, v).astype(np.float32)


def sanitise(variance):
    v = np.asarray(variance, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v) & (v >= 0.0), v, 0.0)


def blur3(v):
    """(1,2,1) x (1,2,1) blur with step 1, taps outside the image skipped and the rest renormalised."""
    H, W = v.shape
    num, den = np.zeros((H, W)), np.zeros((H, W))
    for j in range(3):
        dy = j - 1
        for i in range(3):
            dx = i - 1
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H - max(0, dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W - max(0, dx))
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            num[yd, xd] += B1[i] * B1[j] * v[ys, xs]
            den[yd, xd] += B1[i] * B1[j]
    return num / den


def atrous_guided(rgb, variance, albedo, normal, depth, iterations=5, demodulate=1, sigma_color=4.0, sigma_normal=0.2,
                  sigma_depth=0.1, sigma_albedo=0.1, **_):
    """The filter of prt_denoise_guided in float64.  rgb / albedo / normal (H, W, 3), variance / depth (H, W); returns the
    colour (H, W, 3) and the variance (H, W)."""
    c = np.asarray(rgb, np.float64)
    v = sanitise(variance)
    if iterations == 0:
        return c.copy(), v
    a = np.asarray(albedo, np.float64)
    n = np.asarray(normal, np.float64)
    z = np.asarray(depth, np.float64)
    H, W = c.shape[:2]
    mod = np.fmax(a, EPS)
    mod2 = luma(mod) ** 2
    if demodulate:
        c = c / mod
        v = v / mod2
    sc = float(sigma_color)
    colour_on = 0.0 < sc < np.inf
    i_n, i_z, i_a = _inv2(sigma_normal), _inv2(sigma_depth), _inv2(sigma_albedo)
    hit = np.isfinite(z)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iz_p = i_z / (z * z)
    for lv in range(iterations):
        step = 1 << lv
        fin_p = np.isfinite(c).all(-1)
        with np.errstate(invalid="ignore"):
            y = luma(c)
        i_c = 1.0 / (sc * np.sqrt(blur3(v)) + 1e-4) if colour_on else None
        num = np.zeros_like(c)
        vnum = np.zeros((H, W))
        den = np.zeros((H, W))
        for j in range(5):
            dy = (j - 2) * step
            for i in range(5):
                dx = (i - 2) * step
                ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H - max(0, dy))
                xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W - max(0, dx))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                cq = c[ys, xs]
                ok = np.isfinite(cq).all(-1)
                e = np.zeros(ok.shape)
                with np.errstate(invalid="ignore", over="ignore"):
                    if colour_on:
                        e += np.abs(y[yd, xd] - y[ys, xs]) * i_c[yd, xd]
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
                    vnum[yd, xd] += w * w * np.where(ok, v[ys, xs], 0.0)
                    den[yd, xd] += w
        with np.errstate(invalid="ignore", divide="ignore"):
            out = num / den[..., None]
            vout = vnum / (den * den)
        c = np.where(fin_p[..., None], out, 0.0)
        v = np.where(fin_p, vout, 0.0)
    return (c * mod, v * mod2) if demodulate else (c, v)


def firefly_frame(size=33, at=(13, 19), base=0.5, spike=100.0, var_base=1e-4, var_spike=1e4):
    """The firefly case of the tests: a flat frame with one interior pixel `spike` whose variance says so.  Returns rgb,
    variance and neutral features (albedo 1, normal +z, depth 1)."""
    rgb = np.full((size, size, 3), base, np.float32)
    var = np.full((size, size), var_base, np.float32)
    rgb[at] = spike
    var[at] = var_spike
    feat = {"albedo": np.ones((size, size, 3), np.float32), "normal": np.zeros((size, size, 3), np.float32),
            "depth": np.ones((size, size), np.float32)}
    feat["normal"][..., 2] = 1.0
    return rgb, var, feat


__all__ = ["accum_variance", "atrous_guided", "blur3", "sanitise", "firefly_frame", "luma", "denoise_model"]
