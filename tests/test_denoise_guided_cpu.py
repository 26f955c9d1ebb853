"""CPU tests of the numpy model of the variance-guided a-trous filter (tests/denoise_guided_model.py): the rule of
prt_denoise_guided in include/prt.h, checked against the plain filter's model, closed forms and the firefly property."""
import numpy as np

from tests import denoise_guided_model as G
from tests import denoise_model as M

# SVGF's published values, the starting point of prt_denoise_guided_defaults (the other sigmas as in prt_denoise_defaults)
PUBLISHED_GUIDED = dict(iterations=5, demodulate=1, sigma_color=4.0, sigma_normal=0.2, sigma_depth=0.1, sigma_albedo=0.1)
PLAIN_DEFAULTS = dict(iterations=4, demodulate=1, sigma_color=0.5, sigma_normal=0.2, sigma_depth=0.1, sigma_albedo=0.1)


def random_inputs(rng, h, w, miss=0.2, nan=0.0):
    rgb = rng.gamma(1.0, 0.5, (h, w, 3)).astype(np.float32)
    alb = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    z = rng.uniform(1.0, 3.0, (h, w)).astype(np.float32)
    z[rng.random((h, w)) < miss] = np.inf
    if nan:
        rgb[rng.random((h, w)) < nan, 0] = np.nan
    return rgb, {"albedo": alb, "normal": nrm, "depth": z}


def random_variance(rng, h, w):
    """gamma(1, 0.05) with about 5 % of the pixels set to each of 0, a negative number, NaN, +inf and 1e4."""
    v = rng.gamma(1.0, 0.05, (h, w)).astype(np.float32)
    u = rng.random((h, w))
    for k, bad in enumerate((0.0, -0.3, np.nan, np.inf, 1e4)):
        v[(u >= 0.05 * k) & (u < 0.05 * (k + 1))] = bad
    return v


def test_colour_term_off_is_the_plain_model():
    rng = np.random.default_rng(3)
    for (h, w) in [(1, 1), (9, 1), (23, 31)]:
        rgb, f = random_inputs(rng, h, w, nan=0.03)
        var = random_variance(rng, h, w)
        for params in (dict(PUBLISHED_GUIDED), dict(iterations=3, demodulate=0, sigma_normal=0.7, sigma_depth=0.0, sigma_albedo=0.3)):
            for off in (0.0, -1.0, np.inf):
                got, _ = G.atrous_guided(rgb, var, f["albedo"], f["normal"], f["depth"], **dict(params, sigma_color=off))
                ref = M.atrous(rgb, f["albedo"], f["normal"], f["depth"], **dict(params, sigma_color=0.0))
                np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_variance_of_one_unweighted_level():
    """All sigmas off, constant variance v, one level on 9x9: the centre's variance is v (70/256)^2 (sum h^2 of the B3
    kernel is 70/256 per axis); a corner sees the taps k >= 2 of each axis only, renormalised."""
    v = 0.37
    rng = np.random.default_rng(4)
    rgb, f = random_inputs(rng, 9, 9, miss=0.0)
    off = dict(sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    for demod in (0, 1):
        alb = np.ones_like(f["albedo"]) if demod else f["albedo"]  # (demodulation by albedo 1 divides the variance by 1)
        _, vo = G.atrous_guided(rgb, np.full((9, 9), v), alb, f["normal"], f["depth"], iterations=1, demodulate=demod, **off)
        assert abs(vo[4, 4] - v * (70.0 / 256.0) ** 2) <= 1e-12
        hk = M.B3[2:]
        corner = v * (hk ** 2).sum() ** 2 / hk.sum() ** 4
        for y, x in ((0, 0), (0, 8), (8, 0), (8, 8)):
            assert abs(vo[y, x] - corner) <= 1e-12


def test_constant_after_demodulation_is_a_fixed_point():
    rng = np.random.default_rng(5)
    _, f = random_inputs(rng, 21, 17)
    f["albedo"][:2] = 0.0
    for k in (0.5, 7.0):
        rgb = k * np.fmax(f["albedo"].astype(np.float64), M.EPS)
        for var in (random_variance(rng, 21, 17), np.zeros((21, 17)), np.full((21, 17), 1e6)):
            for params in (PUBLISHED_GUIDED, dict(iterations=7, demodulate=1, sigma_color=0.01, sigma_normal=0.05, sigma_depth=0.01,
                                                  sigma_albedo=0.02)):
                got, vo = G.atrous_guided(rgb, var, f["albedo"], f["normal"], f["depth"], **params)
                np.testing.assert_allclose(got, rgb, rtol=1e-12, atol=0)
                assert np.isfinite(vo).all() and (vo >= 0).all()


def test_zero_iterations_copy_the_colour_and_sanitise_the_variance():
    rng = np.random.default_rng(6)
    rgb, f = random_inputs(rng, 7, 11, nan=0.1)
    var = random_variance(rng, 7, 11)
    got, vo = G.atrous_guided(rgb, var, f["albedo"], f["normal"], f["depth"], iterations=0)
    assert np.array_equal(got, rgb.astype(np.float64), equal_nan=True)
    ok = np.isfinite(var) & (var >= 0)
    assert np.array_equal(vo, np.where(ok, var, 0).astype(np.float64))
    assert (~ok).sum() > 0


def test_firefly_is_pulled_down_and_its_energy_spread():
    """One pixel at 100 in a frame of 0.5, with a variance that says so: the published guided defaults bring it below half
    its input while the plain filter at its defaults keeps it.  The weights are normalised per centre, not per source: the
    calm neighbours (small variance) reject the firefly as a tap while the firefly accepts them, so its excess is mostly
    removed, not spread.  The model's own figure for the change of the frame's sum is 15.40 % (the excess is 15.45 % of the
    sum), above the 1 % one might hope for; the bound is that figure x 1.5."""
    rgb, var, f = G.firefly_frame()
    at = (13, 19)
    off = dict(demodulate=0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    got, vo = G.atrous_guided(rgb, var, f["albedo"], f["normal"], f["depth"], **dict(PUBLISHED_GUIDED, **off))
    plain = M.atrous(rgb, f["albedo"], f["normal"], f["depth"], **dict(PLAIN_DEFAULTS, **off))
    change = abs(got.sum() - rgb.astype(np.float64).sum()) / rgb.astype(np.float64).sum()
    print(f"firefly: guided {got[at][0]:.4f}, plain {plain[at][0]:.4f} of 100; frame sum changes by {change:.3%}; "
          f"variance there {vo[at]:.4g}")
    assert (got[at] < 50.0).all()
    assert (plain[at] > 99.0).all()
    assert change < 1.5 * 0.1540
