"""A numpy restatement of adaptive sampling (include/prt.h, prt_accum_*_adaptive), driven by per-sample radiance.

The tests run it on synthetic data and on the oracle's per-sample radiance, and compare the library against it.  It
follows the library's arithmetic step by step: a batch's partial is the sequential sum of its samples, a launch's
chunks are summed in order into the pixel's sum, and Y(partial)^2 / batch is added into the moment chunk by chunk."""
import numpy as np

PER_LAUNCH_BATCHES = 64  # PRT_MAX_CHUNKS: batches per launch of a round


def luma(rgb):
    rgb = np.asarray(rgb, dtype=np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def estimate(sums, moments, counts, batch):
    """(mean, var, se) of the luminance per pixel: the batch-means estimator of prt.h (nan where count < 2 batches)."""
    with np.errstate(all="ignore"):
        c = counts.astype(np.float64)
        S = luma(sums)
        d = moments - S * S / c
        var = np.where(d < 0.0, 0.0, d) / (counts // batch - 1).astype(np.float64)
        var = np.where(counts >= 2 * batch, var, np.nan)
        se = np.sqrt(var / c)
        return S / c, var, se


def threshold(mean, rel_tol, abs_tol):
    thr = rel_tol * np.abs(mean)
    return np.where(thr < abs_tol, abs_tol, thr)


def active(st, n, min_spp, max_spp, batch, rel_tol, abs_tol):
    """The activity rule of prt.h for every pixel of a state dict (sums, moments, counts)."""
    cnt = st["counts"]
    mean, _, se = estimate(st["sums"], st["moments"], cnt, batch)
    with np.errstate(invalid="ignore"):
        conv = se <= threshold(mean, rel_tol, abs_tol)
    return (cnt == n) & (cnt < max_spp) & ~((cnt >= min_spp) & conv)


def ratio(st, rel_tol, abs_tol, batch):
    """se / threshold per pixel (how close a pixel's last decision was to the other outcome)."""
    mean, _, se = estimate(st["sums"], st["moments"], st["counts"], batch)
    with np.errstate(all="ignore"):
        return se / threshold(mean, rel_tol, abs_tol)


def run(radiance, *, min_spp, max_spp, batch, rel_tol, abs_tol, rounds, owned=None):
    """A whole adaptive run.  radiance: (P, >= max_spp, 3) per-sample RGB of P pixels; rounds: samples per round (an int,
    or a function of the round index and the previous round's n_active).  Returns the state dict plus the per-round
    n_active list."""
    radiance = np.asarray(radiance, dtype=np.float64)
    P = radiance.shape[0]
    st = {"sums": np.zeros((P, 3)), "moments": np.zeros(P), "counts": np.zeros(P, dtype=np.uint32), "samples": 0}
    owned = np.ones(P, dtype=bool) if owned is None else np.asarray(owned, dtype=bool)
    n, history, r = 0, [], 0
    while True:
        act = active(st, n, min_spp, max_spp, batch, rel_tol, abs_tol) & owned
        if not act.any():
            break
        size = rounds if isinstance(rounds, int) else rounds(r, history[-1] if history else None)
        k = min(size, max_spp - n)
        idx = np.flatnonzero(act)
        for s0 in range(0, k, PER_LAUNCH_BATCHES * batch):
            kl = min(PER_LAUNCH_BATCHES * batch, k - s0)
            x = radiance[idx, n + s0:n + s0 + kl].reshape(len(idx), kl // batch, batch, 3)
            part = x[:, :, 0, :].copy()
            for j in range(1, batch):
                part = part + x[:, :, j, :]
            s = np.zeros((len(idx), 3))
            m = np.zeros(len(idx))
            for c in range(kl // batch):
                s = s + part[:, c]
                t = luma(part[:, c])
                m = m + t * t / float(batch)
            st["sums"][idx] += s
            st["moments"][idx] += m
            st["counts"][idx] += kl
        n += k
        history.append(len(idx))
        r += 1
    st["samples"] = n
    st["n_active"] = history
    return st


def frame(st):
    """sum / count per pixel (0 where the count is 0)."""
    c = st["counts"].astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        return np.where(c > 0, st["sums"] / np.where(c > 0, c, 1.0), 0.0)
