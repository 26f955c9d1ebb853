"""References for the device primitives of pooraytracer_amd/csrc/prt_device.h (tests/test_gpu_device_math.py compares
the probe library tests/probe/libprt_probe.so with them; tests/test_device_math_cpu.py checks them against each other).

* mpmath at 60 digits: sqrt, reciprocal, division, sin, cos, pow, the complex square root, Fresnel, the Shirley-Chiu
  concentric map and the visible-normal sampler (Material.h:412-435 restated);
* fractions.Fraction for the FMA helpers: float(Fraction(a) * Fraction(b) + Fraction(k)) IS the correctly rounded result;
* numpy longdouble (64-bit mantissa) where 10^6-point grids make mpmath too slow (checked against mpmath on subsets);
* a model of Rng::next and its inverse: any pair of 31-bit draws is one 64-bit state;
* the exact box test and the case generators of tests/test_slab_cpu.py;
* the BSDF layer (ct_*, mat_eval, mat_scatter): the header's expressions once, over an mpmath backend that carries a running
  error bound and a numpy backend of IEEE operations; inputs by stratum; the comparison both test files use (second half).
"""
import ctypes as C
import glob
import os
import re
from fractions import Fraction

import mpmath
import numpy as np

from tests import test_slab_cpu as slab

mpmath.mp.dps = 60
mpf = mpmath.mpf
LD = np.longdouble

# ------------------------------------------------------------------ the probe library
# launchers over `real` records: name -> (reals in, reals out) per element
REAL_OPS = {
    "fast_rsqrt": (1, 1), "fast_sqrt": (1, 1), "fast_rcp": (1, 1), "fast_div": (2, 1), "ieee_sqrt": (1, 1),
    "ieee_div": (2, 1), "normalize": (3, 3), "normalize_len": (3, 4), "fma_ks": (2, 5), "sincos_quarter": (1, 2),
    "sincos_turns": (1, 2), "sincos_any": (1, 2), "pow_pos": (2, 1), "csqrt": (2, 2), "fr_complex": (3, 1),
    "disk_concentric": (2, 2), "ct_sample_wm": (7, 3),
    # the BSDF layer (inputs: alpha_x, alpha_y / eta[3], k[3], then the directions)
    "tan2theta": (3, 1), "cosphi": (3, 1), "sinphi": (3, 1), "ct_D": (5, 1), "ct_lambda": (5, 1), "ct_G1": (5, 1),
    "ct_G": (8, 1), "ct_Dv": (8, 1), "ct_fresnel": (12, 3),
}
F64_ONLY_OPS = {"fma_sk": (2, 5), "mul_ks": (1, 5)}  # prt_device.h has no fp32 overload of these
F32_ONLY_OPS = {"v_log": (1, 1), "v_exp": (1, 1)}    # the raw v_log_f32 / v_exp_f32 (base 2) of the fp32 pow_pos
OTHER_OPS = ["rng_next", "cosine_hemisphere", "f32_updown", "box4", "mat_eval", "mat_scatter"]
# mat_eval / mat_scatter: (reals in, reals out) per element beside the 64-bit RNG state in and out; the first MAT_NI reals
# are the material's raw fields: type, kd[3], ks[3], ns, eta[3], k[3], alpha_x, alpha_y, pkd override (< 0: none)
MAT_NI = 17
STATE_OPS = {"mat_eval": (MAT_NI + 6, 3), "mat_scatter": (MAT_NI + 9, 7)}
RNG_DRAWS = 4
# the literals of the FMA-helper probes (PROBE_K0..K4 of tests/probe/prt_probe.hip)
FMA_K = [8.33333333332248946124e-03, 6.666666666666735130e-01, -1.66666666666666324348e-01, 1.90821492927058770002e-10,
         1.44269504088896338700e+00]


def probe_symbols():
    """Every launcher the probe library must export."""
    names = []
    for sfx in ("f64", "f32"):
        names += [f"prtprobe_{n}_{sfx}" for n in list(REAL_OPS) + OTHER_OPS]
    names += [f"prtprobe_{n}_f64" for n in F64_ONLY_OPS]
    names += [f"prtprobe_{n}_f32" for n in F32_ONLY_OPS]
    names.append("prtprobe_exhaust_f32")
    return names


def probe_lib():
    """tests/probe/libprt_probe.so, built if stale (a no-op when fresh), with argument types set."""
    from pooraytracer_amd import build
    L = C.CDLL(build.build_probe())
    vp = C.c_void_p
    for name in probe_symbols():
        fn = getattr(L, name)
        fn.restype = C.c_int
        if name.startswith("prtprobe_box4"):
            fn.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
        elif name.startswith("prtprobe_mat_"):
            fn.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
        elif name == "prtprobe_exhaust_f32":
            fn.argtypes = [C.c_int, C.c_uint32, C.c_ulonglong, vp, vp]
        else:
            fn.argtypes = [vp, vp, C.c_size_t, vp]
    return L


# ------------------------------------------------------------------ material parameters that occur in the repository
def _material_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [os.path.join(root, "pooraytracer_amd", "scenes.py")] + sorted(glob.glob(os.path.join(root, "tests", "*.py")))
    return [open(f).read() for f in files if os.path.basename(f) not in ("device_math_model.py", "test_gpu_device_math.py")]


_NUM = r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?"
_TRIPLE = r"\(\s*(%s)\s*,\s*(%s)\s*,\s*(%s)\s*\)" % (_NUM, _NUM, _NUM)


def ns_values_in_sources():
    """Every Phong exponent written in scenes.py and tests/: `ns=<number>`, `ns=float(rng.choice([...]))`, `ns_values = [...]`."""
    found = set()
    for text in _material_sources():
        found |= {float(v) for v in re.findall(r"\bns=(%s)" % _NUM, text)}
        for lst in re.findall(r"\bns=float\(rng\.choice\(\[([^\]]*)\]", text) + re.findall(r"\bns_values\s*=\s*\[([^\]]*)\]", text):
            found |= {float(v) for v in re.findall(_NUM, lst)}
    return sorted(found)


def eta_k_in_sources():
    """Every (eta, k) channel pair of a CookTorrance material written in scenes.py and tests/: `eta=(..), k=(..)` literals and
    the GOLD_ETA, GOLD_K = (..), (..) constants."""
    found = set()
    for text in _material_sources():
        pats = re.findall(r"\beta=%s\s*,\s*k=%s" % (_TRIPLE, _TRIPLE), text) + re.findall(r"GOLD_ETA, GOLD_K = %s\s*,\s*%s" % (_TRIPLE, _TRIPLE), text)
        for m in pats:
            found |= {(float(e), float(k)) for e, k in zip(m[:3], m[3:])}
    return sorted(found)


# ------------------------------------------------------------------ ulps
def ulp_of(ref, dtype=np.float64):
    """Spacing of `dtype` at |ref| (ref: longdouble or float array)."""
    r = np.abs(np.asarray(ref).astype(dtype))
    return np.spacing(r).astype(LD)


def ulp_err(got, ref, dtype=np.float64):
    """|got - ref| in ulps of `dtype` at ref; ref in longdouble."""
    ref = np.asarray(ref, dtype=LD)
    return np.abs(np.asarray(got).astype(LD) - ref) / ulp_of(ref, dtype)


def mp_of(x):
    """Exact mpf of a Python / numpy binary float (a longdouble as its float64 head plus the exact remainder)."""
    if isinstance(x, np.longdouble):
        hi = float(x)
        return mpf(hi) + mpf(float(x - LD(hi)))
    return mpf(float(x))


# ------------------------------------------------------------------ FMA helpers: correctly rounded by construction
def fma_exact(a, b, c):
    """round-to-nearest-even of a * b + c for binary64 a, b, c (finite)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma_exact_many(a, b, c):
    """fma_exact over arrays, through integers: every binary64 is n / 2^e, and Python's int / int is correctly rounded."""
    out = np.empty(len(a))
    for i, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), np.broadcast_to(c, a.shape).tolist())):
        xn, xd = x.as_integer_ratio()
        yn, yd = y.as_integer_ratio()
        zn, zd = z.as_integer_ratio()
        out[i] = (xn * yn * zd + zn * xd * yd) / (xd * yd * zd)
    return out


def fma_exact32(a, b, c):
    """... for binary32 operands: a * b + c is exact in Fraction, numpy rounds the (exactly representable as a ratio)
    value once.  float(Fraction) rounds to binary64 first, which could double-round; round directly instead."""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return round_fraction_f32(v)


def round_fraction_f32(v):
    if v == 0:
        return np.float32(0.0)
    f = np.float32(float(v))  # candidate; fix a double rounding by looking at its neighbours
    best = f
    for cand in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        if np.isfinite(cand):
            dc, db = abs(Fraction(float(cand)) - v), abs(Fraction(float(best)) - v)
            if dc < db or (dc == db and (int(np.float32(cand).view(np.uint32)) & 1) == 0):
                best = cand
    return np.float32(best)


def unfused_differs(a, b, c):
    """True where round(round(a*b) + c) != round(a*b + c): the operands a dropped fusion would expose."""
    return float(np.float64(a) * np.float64(b) + np.float64(c)) != fma_exact(a, b, c)


# ------------------------------------------------------------------ the RNG: xoroshiro64*, 31 (24) bits per draw
M32 = np.uint64(0xFFFFFFFF)
MULT = 0x9E3779BB
MULT_INV = pow(MULT, -1, 1 << 32)


def _rotl(x, k):
    x = x & M32
    return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & M32


def rng_next(state):
    """One step of Rng::next on uint64 states: returns (r, new state) with r the 32-bit product (draw = r >> 1 over 2^31
    in fp64, r >> 8 over 2^24 in fp32)."""
    state = np.asarray(state, dtype=np.uint64)
    s0, s1 = state & M32, state >> np.uint64(32)
    r = (s0 * np.uint64(MULT)) & M32
    s1 = s1 ^ s0
    s0 = _rotl(s0, 26) ^ s1 ^ ((s1 << np.uint64(9)) & M32)
    s1 = _rotl(s1, 13)
    return r, (s1 << np.uint64(32)) | s0


def rng_draws(state, k, f32=False):
    """The first k draws of the stream started at `state`, as the device returns them."""
    out = []
    for _ in range(k):
        r, state = rng_next(state)
        out.append((r >> np.uint64(8)).astype(np.float64) / 2.0 ** 24 if f32 else (r >> np.uint64(1)).astype(np.float64) / 2.0 ** 31)
    return np.stack(out, axis=-1), state


def craft_state(first, second, shift=1):
    """The 64-bit state whose first two draws are first / 2^31 and second / 2^31 (shift = 1; the fp32 unit's k / 2^24 with
    shift = 8).  The multiplier is odd, so s0 = r * inv mod 2^32 yields any first product r = first << shift; the next s0
    is rotl(s0, 26) ^ t ^ (t << 9) with t = s0 ^ s1, and y -> y ^ (y << 9) is inverted by y ^ y<<9 ^ y<<18 ^ y<<27."""
    first = np.asarray(first, dtype=np.uint64)
    second = np.asarray(second, dtype=np.uint64)
    inv = np.uint64(MULT_INV)
    s0 = (((first << np.uint64(shift)) & M32) * inv) & M32
    s0n = (((second << np.uint64(shift)) & M32) * inv) & M32
    y = s0n ^ _rotl(s0, 26)
    t = (y ^ (y << np.uint64(9)) ^ (y << np.uint64(18)) ^ (y << np.uint64(27))) & M32
    s1 = t ^ s0
    return (s1 << np.uint64(32)) | s0


# ------------------------------------------------------------------ concentric map (Shirley-Chiu), cosine hemisphere
def disk_concentric_ld(ux, uy):
    """RandomNumberGenerator.h:39-56 in longdouble on exact lattice inputs (2u - 1 is exact)."""
    ux, uy = np.asarray(ux, dtype=LD), np.asarray(uy, dtype=LD)
    ox, oy = 2 * ux - 1, 2 * uy - 1
    pi4 = LD(mpmath.nstr(mpmath.pi / 4, 30))
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        th = np.where(first, pi4 * (oy / np.where(ox == 0, 1, ox)), 2 * pi4 - pi4 * (ox / np.where(oy == 0, 1, oy)))
    r = np.where(first, ox, oy)
    x, y = r * np.cos(th), r * np.sin(th)
    zero = (ox == 0) & (oy == 0)
    return np.where(zero, 0, x), np.where(zero, 0, y)


def disk_concentric_mp(ux, uy, force_first=None):
    """One point in mpmath; `force_first` picks the branch regardless of the comparison (the map is continuous across
    |off.x| == |off.y|, so both branches are valid references there)."""
    ox, oy = 2 * mpf(float(ux)) - 1, 2 * mpf(float(uy)) - 1
    if ox == 0 and oy == 0:
        return mpf(0), mpf(0)
    first = abs(ox) > abs(oy) if force_first is None else force_first
    if first:
        th, r = mpmath.pi / 4 * (oy / ox), ox
    else:
        th, r = mpmath.pi / 2 - mpmath.pi / 4 * (ox / oy), oy
    return r * mpmath.cos(th), r * mpmath.sin(th)


def cosine_hemisphere_ld(first, second):
    """SampleCosineHemisphere with B20's order: u.y = first draw, u.x = second."""
    x, y = disk_concentric_ld(second, first)
    z = np.sqrt(np.maximum(LD(0), 1 - x * x - y * y))
    return x, y, z


# ------------------------------------------------------------------ Fresnel (MaterialUtils.h:54-65, 100-111) in mpmath
def csqrt_mp(re, im):
    return mpmath.sqrt(mpmath.mpc(mpf(float(re)), mpf(float(im))))


def fr_complex_mp(cos_i, eta, k):
    """Returns None where the formula is 0/0."""
    c = min(max(mpf(float(cos_i)), mpf(0)), mpf(1))
    e = mpmath.mpc(mpf(float(eta)), mpf(float(k)))
    s2 = 1 - c * c
    ct = mpmath.sqrt(1 - s2 / (e * e))
    d1, d2 = e * c + ct, c + e * ct
    if d1 == 0 or d2 == 0:
        return None
    rp, rs = (e * c - ct) / d1, (c - e * ct) / d2
    return (abs(rp) ** 2 + abs(rs) ** 2) / 2


# ------------------------------------------------------------------ visible-normal sampler (Material.h:412-435) in mpmath
WM_SWITCH = mpf(0.99999)  # the double the source literal rounds to


def _mp_norm(v):
    n = mpmath.sqrt(sum(c * c for c in v))
    return [c / n for c in v]


def _mp_cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def ct_sample_wm_mp(ax, ay, w, u, force_basis=None):
    """The sampler in the reference's own expressions, which are exact here (the device evaluates h and pz through
    algebraically equal, cancellation-free forms).  Returns (wm, info): wm the sampled micro-normal, info the condition
    numbers the test's bound is built from.
    `force_basis`: True = the cross-product basis, False = T1 = (1, 0, 0), None = by the wh.z < 0.99999 switch."""
    ax, ay = mpf(float(ax)), mpf(float(ay))
    w = [mpf(float(c)) for c in w]
    u = [mpf(float(c)) for c in u]
    wh = _mp_norm([ax * w[0], ay * w[1], w[2]])
    if wh[2] < 0:
        wh = [-c for c in wh]
    basis = wh[2] < WM_SWITCH if force_basis is None else force_basis
    T1 = _mp_norm(_mp_cross([mpf(0), mpf(0), mpf(1)], wh)) if basis else [mpf(1), mpf(0), mpf(0)]
    T2 = _mp_cross(wh, T1)
    r, th = mpmath.sqrt(u[0]), 2 * mpmath.pi * u[1]
    px, py = r * mpmath.cos(th), r * mpmath.sin(th)
    h = mpmath.sqrt(1 - px * px)
    lx = (1 + wh[2]) / 2
    py = (1 - lx) * h + lx * py
    q = max(mpf(0), 1 - (px * px + py * py))
    pz = mpmath.sqrt(q)
    nh = [px * T1[i] + py * T2[i] + pz * wh[i] for i in range(3)]
    v = [ax * nh[0], ay * nh[1], max(mpf("1e-6"), nh[2])]
    vlen = mpmath.sqrt(sum(c * c for c in v))
    sin_h = mpmath.sqrt(max(mpf(0), 1 - wh[2] * wh[2]))
    info = {"sin_h": float(sin_h), "pz": float(pz), "vlen": float(vlen), "basis": bool(basis), "whz": float(wh[2]),
            "px": float(px), "py": float(py), "h": float(h), "q": float(q), "amax": float(max(ax, ay, 1)), "whz_mp": wh[2]}
    return [c / vlen for c in v], info


# ------------------------------------------------------------------ the box test: cases, exact quantities
def exact_interval(o, d, lo, hi, tmin=1e-4, tmax=np.inf):
    """Entry and exit of the exact slab test (tests/test_slab_cpu.py:exact_test's t0, t1, with a finite tmax as well)."""
    t0 = np.full(o.shape[0], tmin)
    t1 = np.full(o.shape[0], np.inf) if np.isscalar(tmax) else np.asarray(tmax, dtype=np.float64).copy()
    if np.isscalar(tmax):
        t1[:] = tmax
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            inv = 1.0 / d[:, a]
            ta, tb = (lo[:, a] - o[:, a]) * inv, (hi[:, a] - o[:, a]) * inv
            t0 = np.maximum(t0, np.minimum(ta, tb))
            t1 = np.minimum(t1, np.maximum(ta, tb))
    return t0, t1


TMIN = 1e-4
TMAX_VALUES = (1e30, 1e300, np.inf)  # what the kernels pass


def box_cases(seed=5, per_config=1 << 16):
    """~2^20 (ray, box) pairs from the generators of tests/test_slab_cpu.py: scenes at the origin and translated to 1e6,
    extents 2 and 1e-2, rays from inside, nearby, 3e6 and 1e9 away; zero / -0 / subnormal / NaN / +-tiny direction
    components, origins exactly on a box plane, grid indices 0 and 65535, degenerate ranges.  (The inverted empty-slot
    range is not a box — exact_test would un-invert it — and has its own cases: empty_slot_cases.)"""
    rng = np.random.default_rng(seed)
    parts = []
    n = per_config
    for center in ((0.0, 0.0, 0.0), (1e6, -3e5, 2e6)):
        center = np.asarray(center)
        for extent in (2.0, 1e-2):
            g0, gs, E = slab.grid_for(center, extent)
            for dist in (0.0, 10 * extent, 3e6, 1e9):
                o, d = slab.rays_towards(rng, n, center, extent, dist)
                lo_q = rng.integers(0, 65000, size=(n, 3))
                hi_q = lo_q + rng.integers(1, 535, size=(n, 3))
                kind = rng.integers(0, 16, size=n)
                big = kind == 0  # large boxes: most accepted pairs come from these
                lo_q[big] = rng.integers(0, 30000, size=(int(big.sum()), 3))
                hi_q[big] = lo_q[big] + rng.integers(1000, 35535, size=(int(big.sum()), 3))
                edge0, edge1 = kind == 1, kind == 2  # grid indices 0 and 65535
                lo_q[edge0, :] = 0
                hi_q[edge0] = rng.integers(1, 65536, size=(int(edge0.sum()), 3))
                hi_q[edge1, :] = 65535
                lo_q[edge1] = rng.integers(0, 65535, size=(int(edge1.sum()), 3))
                deg = kind == 3  # degenerate on one axis
                ax_ = rng.integers(0, 3, size=n)
                rows = np.nonzero(deg)[0]
                hi_q[rows, ax_[rows]] = lo_q[rows, ax_[rows]]
                lo = g0.astype(np.float64) + lo_q * gs.astype(np.float64)
                hi = g0.astype(np.float64) + hi_q * gs.astype(np.float64)
                onp = np.nonzero((kind == 4) | (kind == 5))[0]  # origin exactly on a box plane
                o[onp, ax_[onp]] = np.where(kind[onp] == 4, lo[onp, ax_[onp]], hi[onp, ax_[onp]])
                sp = np.nonzero(kind >= 12)[0]  # special direction component on one axis
                vals = np.array([0.0, -0.0, 5e-324, -1e-310, np.nan, 1e-30, -1e-30, 1e-45, -1e-38, 1e-20])
                d[sp, ax_[sp]] = vals[rng.integers(0, len(vals), size=len(sp))]
                tmax = np.asarray(TMAX_VALUES)[rng.integers(0, 3, size=n)]
                grid = np.empty((n, 7), dtype=np.float32)
                grid[:, 0], grid[:, 1:4], grid[:, 4:7] = E, g0, gs
                parts.append(dict(o=o, d=d, lo=lo, hi=hi, lo_q=lo_q, hi_q=hi_q, tmax=tmax, grid=grid,
                                  r=g0.astype(np.float64)[None, :] - o, E=np.full(n, float(E))))
    c = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    c["packed"] = (c["lo_q"].astype(np.uint32) | (c["hi_q"].astype(np.uint32) << np.uint32(16))).astype(np.uint32)
    c["tmin"] = np.full(c["o"].shape[0], TMIN)
    return c


def box_expectations(c):
    """must_accept: the exact test accepts.  must_reject: the exact entry exceeds the exact exit by more than
    2^-18 * max_a((|r_a| + E) |1/d_a|) — four pads: the two planes' pads plus their <= 6 * 2^-24 roundings."""
    t0, t1 = exact_interval(c["o"], c["d"], c["lo"], c["hi"], TMIN, c["tmax"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        thr = 2.0 ** -18 * np.max((np.abs(c["r"]) + c["E"][:, None]) * np.abs(1.0 / c["d"]), axis=1)
        must_accept = t1 > t0
        must_reject = (t0 - t1) > thr
    return must_accept, must_reject & np.isfinite(thr)


def empty_slot_cases(seed=11, n=1 << 14):
    """The inverted range (lo = 0xffff, hi = 0 on every axis) against rays inside the scene, 100 away and 2^17 extents away."""
    rng = np.random.default_rng(seed)
    center, extent = np.array([1e6, 1e6, 1e6]), 2.0
    g0, gs, E = slab.grid_for(center, extent)
    os_, ds_ = [], []
    for dist in (0.0, 100.0, 2.0 ** 17 * extent):
        o, d = slab.rays_towards(rng, n, center, extent, dist)
        os_.append(o)
        ds_.append(d)
    o, d = np.concatenate(os_), np.concatenate(ds_)
    m = o.shape[0]
    grid = np.empty((m, 7), dtype=np.float32)
    grid[:, 0], grid[:, 1:4], grid[:, 4:7] = E, g0, gs
    return dict(o=o, d=d, grid=grid, packed=np.full((m, 3), 0x0000FFFF, dtype=np.uint32), tmin=np.full(m, TMIN),
                tmax=np.full(m, np.inf), lo_q=np.full((m, 3), 0xFFFF), hi_q=np.zeros((m, 3), dtype=np.int64), E=E, g0=g0, gs=gs)


# ------------------------------------------------------------------ input sets shared by the GPU tests
def binade_inputs(rng, lo_exp=-1022, hi_exp=1023, n_random=64):
    """Every binade 2^lo_exp .. 2^hi_exp with mantissas {1, 1 + ulp, 2 - ulp, the neighbours of sqrt 2, n_random random}."""
    sq2 = np.float64(np.sqrt(2.0))
    fixed = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), np.nextafter(sq2, 1.0), sq2, np.nextafter(sq2, 2.0)])
    e = np.arange(lo_exp, hi_exp + 1)
    m = np.concatenate([np.broadcast_to(fixed, (e.size, fixed.size)), 1.0 + rng.random((e.size, n_random))], axis=1)
    return np.ldexp(m, e[:, None]).ravel()


def lattice_ends(k_max=1 << 12, bits=31):
    k = np.arange(1, k_max + 1, dtype=np.float64)
    return np.concatenate([k, 2.0 ** bits - k]) / 2.0 ** bits


# ================================================================== the BSDF layer (prt_device.h: CookTorrance terms, mat_eval, mat_scatter)
# The header's expressions are written ONCE below (bsdf_*), in the header's algebraic form and operation order, over an
# arithmetic backend `A`:
#   * MpArith  — every value is a V: the exact result (mpmath, 60 digits) of the expression on the inputs rounded to the
#     probe's precision, and a RUNNING ERROR BOUND for what the device holds in its place;
#   * NpArith  — numpy scalars of float32 / float64, IEEE operations only: the "plain restatement" that
#     tests/test_device_math_cpu.py holds against the bound (and into which it injects its mutations).
#
# The bound is propagated operation by operation, to first order: an operation with exact result r adds k * u * |r| to the
# error carried in by its operands (u = 2^-53 / 2^-24; k counts ulps of the operation's documented or tested accuracy:
# 0.5 for + - * / sqrt fma, 2 for the fp64 fast_*, 1 for the fp32 hardware rcp / rsq / sqrt, 2 for the fp32 a * rcp(b)
# quotients, and the exhaustive maxima for v_log_f32 / v_exp_f32).  Since u is half an ulp at the bottom of a binade, k * u
# is HALF the worst case there; the asserted tolerance is twice the running bound plus one subnormal quantum.  Bounds that
# the repository's own tests state absolutely or relatively (normalize, the sincos functions, pow_pos fp64) enter in full.
# An operation on exact operands whose exact result is representable is exact (IEEE), as is scaling by a power of two.
# A result below the smallest normal adds an absolute term: one quantum in fp64 (gradual underflow), the smallest normal
# in fp32 (v_rcp / v_sqrt / v_log / v_exp_f32 flush, and the ISA leaves the rest to the denormal mode).  A result that may
# exceed the largest finite number makes the bound infinite from there on (the device may hold inf): such outputs are
# checked for finiteness and sign only — finiteness is required wherever the EXACT output is finite.
INF = mpf("inf")
K_LOG_F32, K_EXP_F32 = 1.5, 1.5  # v_log_f32 / v_exp_f32: exhaustive maximum distance (1 ulp each) + the reference's own half ulp


class Undefined(Exception):
    """The expression is 0/0, inf * 0 or sqrt of a negative number in exact arithmetic."""


class Prec:
    def __init__(self, name):
        self.name, self.f32 = name, name == "f32"
        self.dtype = np.float32 if self.f32 else np.float64
        self.u = mpf(2) ** (-24 if self.f32 else -53)
        self.tiny = mpf(2) ** (-126 if self.f32 else -1022)
        self.quantum = mpf(2) ** (-149 if self.f32 else -1074)
        self.under = self.tiny if self.f32 else self.quantum
        self.max = mpf(float(np.finfo(self.dtype).max))
        self.bits, self.shift = (24, 8) if self.f32 else (31, 1)
        self.k_fast = 1 if self.f32 else 2       # fast_rcp / fast_sqrt / fast_rsqrt
        self.k_fdiv = 2                          # fast_div
        self.k_idiv = 2 if self.f32 else 0.5     # ieee_div
        self.k_isqrt = 1 if self.f32 else 0.5    # ieee_sqrt

    def rnd(self, x):
        """x (a Python float or an mpf) rounded to the precision, as a Python float."""
        with np.errstate(all="ignore"):
            return float(self.dtype(float(x)))


PRECS = {"f64": Prec("f64"), "f32": Prec("f32")}


class V:
    """exact value v, running bound e; ef = the bound before a possible overflow made it infinite (isinf's decision)."""
    __slots__ = ("v", "e", "ef", "A")

    def __init__(self, A, v, e=0, ef=None):
        self.A, self.v, self.e = A, (v if isinstance(v, mpf) else mpf(v)), (e if isinstance(e, mpf) else mpf(e))
        self.ef = self.e if ef is None else ef

    def __add__(self, o):
        o = self.A.of(o)
        return self.A.fin(self.v + o.v, self.e + o.e, 0.5)
    __radd__ = __add__

    def __sub__(self, o):
        o = self.A.of(o)
        return self.A.fin(self.v - o.v, self.e + o.e, 0.5)

    def __rsub__(self, o):
        return self.A.of(o) - self

    def __neg__(self):
        return V(self.A, -self.v, self.e, self.ef)

    def __abs__(self):
        return V(self.A, abs(self.v), self.e, self.ef)

    def __mul__(self, o):
        o = self.A.of(o)
        v = self.v * o.v
        if mpmath.isnan(v):
            raise Undefined("inf * 0")
        if self.e == INF or o.e == INF:
            ein = INF
        else:
            ein = abs(self.v) * o.e + abs(o.v) * self.e
        for s in (self, o):  # scaling by a power of two is exact
            if s.e == 0 and s.v in _POW2:
                return self.A.fin(v, ein, 0)
        return self.A.fin(v, ein, 0.5)
    __rmul__ = __mul__

    def __truediv__(self, o):
        return self.A.div(self, o)

    def __rtruediv__(self, o):
        return self.A.div(self.A.of(o), self)


_POW2 = frozenset((mpf(1), mpf(2), mpf(4), mpf(0.5), mpf(-1), mpf(0.25), mpf(-2)))


class MpArith:
    exact = True

    def __init__(self, prec):
        self.P = PRECS[prec]
        self.knife = []  # names of the knife-edge comparisons met on this input
        self.mut = None

    # ---- values
    def of(self, x):
        return x if isinstance(x, V) else V(self, x)

    def c(self, x):
        """a literal of the header, RL(x): rounded to the precision, exact from there"""
        return V(self, self.P.rnd(x))
    inp = c

    def val(self, x):
        return x.v

    def representable(self, v):
        a = abs(v)
        if a > self.P.max:
            return False
        return mpf(self.P.rnd(v)) == v

    def fin(self, v, ein, k, absolute=0):
        P = self.P
        a = abs(v)
        if a == INF:
            return V(self, v)
        if ein == 0 and absolute == 0 and k <= 0.5 and self.representable(v):
            return V(self, v)
        ef = ein + k * P.u * a + absolute
        if 0 < a < P.tiny:
            ef = ef + P.under
        e = INF if a + 2 * ef >= P.max else ef
        return V(self, v, e, ef)

    # ---- operations
    def div(self, a, b, k=0.5):
        a, b = self.of(a), self.of(b)
        if b.v == 0 and b.e == 0:
            if a.v == 0:
                raise Undefined("0/0")
            return V(self, INF if a.v > 0 else -INF)
        if b.v == 0:
            raise Undefined("x / (0 +- e)")
        if abs(b.v) == INF:
            if abs(a.v) == INF:
                raise Undefined("inf/inf")
            return V(self, 0)
        v = a.v / b.v
        if a.e == INF or b.e == INF or 2 * b.e >= abs(b.v):
            ein = INF
        else:
            ein = a.e / abs(b.v) + abs(v) * b.e / abs(b.v)
        if b.e == 0 and b.v in _POW2:
            k = 0
        return self.fin(v, ein, k)

    def ieee_div(self, a, b):
        return self.div(a, b, self.P.k_idiv)

    def fast_div(self, a, b):
        return self.div(a, b, self.P.k_fdiv)

    def fast_rcp(self, b):
        return self.div(V(self, 1), b, self.P.k_fast)

    def _sqrt(self, a, k):
        a = self.of(a)
        if a.v < 0:
            if a.e > 0 and -a.v <= 2 * a.e:
                return V(self, 0, mpmath.sqrt(2 * a.e))
            raise Undefined("sqrt of a negative number")
        v = mpmath.sqrt(a.v)
        if a.e == INF:
            ein = INF
        elif a.e == 0:
            ein = mpf(0)
        elif 4 * a.e > a.v:  # first order does not hold this close to zero: |sqrt(x + d) - sqrt(x)| <= min(|d| / sqrt(x), sqrt|d|)
            ein = min(a.e / v, mpmath.sqrt(a.e)) if v > 0 else mpmath.sqrt(a.e)
        else:
            ein = a.e / (2 * v)
        return self.fin(v, ein, k)

    def ieee_sqrt(self, a):
        return self._sqrt(a, self.P.k_isqrt)

    def fast_sqrt(self, a):
        return self._sqrt(a, self.P.k_fast)

    def fmax(self, a, b):
        a, b = self.of(a), self.of(b)
        r = a if a.v >= b.v else b
        return V(self, r.v, max(a.e, b.e), max(a.ef, b.ef))

    def fmin(self, a, b):
        a, b = self.of(a), self.of(b)
        r = a if a.v <= b.v else b
        return V(self, r.v, max(a.e, b.e), max(a.ef, b.ef))

    def clamp(self, v, lo, hi):
        """Both the exact value and the device's lie in [lo, hi] (exact bounds): the error cannot exceed the interval's width."""
        r = self.fmin(self.fmax(v, lo), hi)
        w = self.of(hi).v - self.of(lo).v
        return V(self, r.v, min(r.e, w), min(r.ef, w))

    def at_pole(self, value, st):
        """cosphi / sinphi where the model's sin(theta) is exactly 0: exact if that zero is exact; otherwise the device may have
        taken the quotient branch and hold anything in [-1, 1]."""
        return V(self, value, 0 if self.of(st).e == 0 else 1 + abs(mpf(value)))

    def normalize(self, v):
        """v * fast_rsqrt(dot(v, v)), operation by operation: test_normalize_fp64_and_fp32's 4 ulp of the unit length is this
        count stated absolutely; a component far below 1 (a grazing z) keeps its RELATIVE accuracy, which the absolute figure
        would throw away.  An exactly zero component stays exactly zero (0 * r)."""
        v = [self.of(c) for c in v]
        q = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        if q.v == 0:
            raise Undefined("normalize(0)")
        rv = 1 / mpmath.sqrt(q.v)
        r = self.fin(rv, INF if (q.e == INF or 2 * q.e >= q.v) else rv * q.e / (2 * q.v), self.P.k_fast)
        return [c * r for c in v]

    def sincos_quarter(self, x):
        x = self.of(x)
        s, c = mpmath.sin(x.v), mpmath.cos(x.v)
        u = self.P.u
        if self.P.f32:  # cos <= 3 u absolute, sin <= 3 u |x| (test_sincos_quarter)
            return self.fin(s, abs(c) * x.e, 0, absolute=3 * u * abs(x.v)), self.fin(c, abs(s) * x.e, 0, absolute=3 * u)
        return self.fin(s, abs(c) * x.e, 1), self.fin(c, abs(s) * x.e, 1)  # < 1 ulp of the result

    def sincos_turns(self, uu):
        """u on the lattice (exact): <= 2^-52 absolute in fp64, <= 5 * 2^-24 in fp32; exactly 0 / +-1 on the quarter turns."""
        t = 2 * mpmath.pi * self.of(uu).v
        if 4 * self.of(uu).v == mpmath.floor(4 * self.of(uu).v):
            q = int(4 * self.of(uu).v) & 3
            return V(self, (0, 1, 0, -1)[q]), V(self, (1, 0, -1, 0)[q])
        b = (5 if self.P.f32 else 2) * self.P.u
        return self.fin(mpmath.sin(t), 0, 0, absolute=b), self.fin(mpmath.cos(t), 0, 0, absolute=b)

    def sincos_any(self, uu):
        """fp64: the library sincos (2 ulp) of theta = 2 * PRT_PI * u as the header rounds it; fp32: v_sin_f32 / v_cos_f32 of u
        in turns, 16 * 2^-24 absolute (the budget stated in prt_device.h)."""
        uu = self.of(uu)
        if self.P.f32:
            t = 2 * mpmath.pi * uu.v
            b = 16 * self.P.u
            return self.fin(mpmath.sin(t), 0, 0, absolute=b), self.fin(mpmath.cos(t), 0, 0, absolute=b)
        th = (2 * self.c(mpmath.pi)) * uu
        return self.fin(mpmath.sin(th.v), abs(mpmath.cos(th.v)) * th.e, 2), self.fin(mpmath.cos(th.v), abs(mpmath.sin(th.v)) * th.e, 2)

    def pow_pos(self, x, y):
        x, y = self.of(x), self.of(y)
        if x.v == 0 and x.e == 0:
            return V(self, 0)
        if x.v <= 0:
            raise Undefined("pow_pos of a non-positive number")
        lg = mpmath.log(x.v)
        if self.P.f32:  # v_exp_f32(y * v_log_f32(x)), base 2
            l2 = lg / mpmath.log(2)
            L = self.fin(l2, x.e / (x.v * mpmath.log(2)), K_LOG_F32)
            t = y * L
            v = mpmath.power(2, t.v)
            return self.fin(v, INF if t.e == INF else mpmath.log(2) * v * t.e, K_EXP_F32)
        v = mpmath.exp(y.v * lg)
        if abs(y.v * lg) > 50 or x.e == INF or y.e == INF:  # the comment's domain; no bound is stated beyond it
            return V(self, v, INF, INF)
        return self.fin(v, v * (abs(y.v) / x.v * x.e + abs(lg) * y.e), 0, absolute=mpf("1e-14") * v)

    def round_sum(self, a, b):
        """a + b of two exact numbers as the device rounds it (one IEEE addition: deterministic)"""
        return V(self, self.P.rnd(self.of(a).v + self.of(b).v))

    def nan_to_zero(self, a):
        return a  # the exact value is never NaN

    # ---- decisions
    def _mark(self, diff, e, name):
        if name and e > 0 and abs(diff) <= 2 * e:
            self.knife.append(name)

    def gt(self, a, b, name=None):
        a, b = self.of(a), self.of(b)
        self._mark(a.v - b.v, a.e + b.e, name)
        return a.v > b.v

    def lt(self, a, b, name=None):
        return self.gt(b, a, name)

    def ge(self, a, b):
        return self.of(a).v >= self.of(b).v

    def eq0(self, a, name=None):
        a = self.of(a)
        self._mark(a.v, a.e, name)
        return a.v == 0

    def isinf(self, a, name="isinf(t2)"):
        thr = self.P.max * (1 + self.P.u)  # beyond this a rounded result is inf
        if abs(a.v) == INF:
            return True
        if a.ef == INF:
            self.knife.append(name)
            return abs(a.v) >= thr
        self._mark(abs(a.v) - thr, a.ef, name)
        return abs(a.v) >= thr


class NpArith:
    """The same expressions in numpy scalars: IEEE operations of the precision, library functions for the rest."""
    exact = False

    def __init__(self, prec, mut=None):
        self.P = PRECS[prec]
        self.t = self.P.dtype
        self.knife = []
        self.mut = mut

    def of(self, x):
        return self.t(x)

    def c(self, x):
        return self.t(float(x))
    inp = c

    def val(self, x):
        return mpf(float(x))

    def div(self, a, b):
        return self.t(a) / self.t(b)
    ieee_div = fast_div = div

    def fast_rcp(self, b):
        return self.t(1) / self.t(b)

    def ieee_sqrt(self, a):
        return np.sqrt(self.t(a))
    fast_sqrt = ieee_sqrt

    def fmax(self, a, b):
        return np.fmax(self.t(a), self.t(b))

    def fmin(self, a, b):
        return np.fmin(self.t(a), self.t(b))

    def clamp(self, v, lo, hi):
        v, lo, hi = self.t(v), self.t(lo), self.t(hi)
        return lo if v < lo else (hi if v > hi else v)

    def at_pole(self, value, st):
        return self.t(value)

    def normalize(self, v):
        v = [self.t(c) for c in v]
        r = self.t(1) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return [c * r for c in v]

    def sincos_quarter(self, x):
        return np.sin(self.t(x)), np.cos(self.t(x))

    def sincos_turns(self, uu):
        uu = float(uu)
        k = np.floor(4.0 * uu + 0.5)
        s, c = np.sin(2 * np.pi * (uu - 0.25 * k)), np.cos(2 * np.pi * (uu - 0.25 * k))
        q = int(k) & 3
        return self.t((s, c, -s, -c)[q]), self.t((c, -s, -c, s)[q])

    def sincos_any(self, uu):
        if self.P.f32:
            return self.t(np.sin(2 * np.pi * float(uu))), self.t(np.cos(2 * np.pi * float(uu)))
        th = (2 * self.t(np.pi)) * self.t(uu)
        return np.sin(th), np.cos(th)

    def pow_pos(self, x, y):
        x, y = self.t(x), self.t(y)
        if x == 0:
            return self.t(0)
        return np.exp2(y * np.log2(x)) if self.P.f32 else np.power(x, y)

    def round_sum(self, a, b):
        return self.t(a) + self.t(b)

    def nan_to_zero(self, a):
        return a if a == a else self.t(0)

    def gt(self, a, b, name=None):
        return bool(self.t(a) > self.t(b))

    def lt(self, a, b, name=None):
        return bool(self.t(a) < self.t(b))

    def ge(self, a, b):
        return bool(self.t(a) >= self.t(b))

    def eq0(self, a, name=None):
        return bool(self.t(a) == 0)

    def isinf(self, a, name=None):
        return bool(np.isinf(a))


# ------------------------------------------------------------------ the header's expressions
def _sqr(v):
    return v * v


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(x, y):
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def _vadd(a, b):
    return [p + q for p, q in zip(a, b)]


def _vscale(a, s):
    return [p * s for p in a]


def _vneg(a):
    return [-p for p in a]


def _vdiv(A, a, s):  # d3 / real: one fast_rcp, three products
    r = A.fast_rcp(s)
    return [p * r for p in a]


def bsdf_cos2theta(A, w):
    return _sqr(w[2])


def bsdf_sin2theta(A, w):
    return A.fmax(A.c(0), 1 - bsdf_cos2theta(A, w))


def bsdf_tan2theta(A, w):
    return A.div(bsdf_sin2theta(A, w), bsdf_cos2theta(A, w))


def bsdf_cosphi(A, w):
    # `st == 0` needs no knife-edge mark: the result is clamped to [-1, 1], so the bound is capped at the interval's width on
    # either side of the decision (MpArith.clamp / at_pole), and every user multiplies it by tan2theta, which is 0 to within
    # ITS bound wherever the decision is in doubt — the switch is continuous in ct_D and ct_lambda.
    st = A.ieee_sqrt(bsdf_sin2theta(A, w))
    return A.at_pole(1, st) if A.eq0(st) else A.clamp(A.div(w[0], st), A.c(-1), A.c(1))


def bsdf_sinphi(A, w):
    st = A.ieee_sqrt(bsdf_sin2theta(A, w))
    return A.at_pole(0, st) if A.eq0(st) else A.clamp(A.div(w[1], st), A.c(-1), A.c(1))


def bsdf_ct_D(A, ax, ay, wm):
    t2 = bsdf_tan2theta(A, wm)
    if A.isinf(t2):
        return A.c(0)
    cos4 = _sqr(bsdf_cos2theta(A, wm))
    ay_ = ax if A.mut == "alpha_x for both axes" else ay
    e = t2 * (_sqr(A.div(bsdf_cosphi(A, wm), ax)) + _sqr(A.div(bsdf_sinphi(A, wm), ay_)))
    tail = (1 + e) if A.mut == "(1 + e) not squared" else _sqr(1 + e)
    return A.nan_to_zero(A.div(A.c(1), A.c(mpmath.pi) * ax * ay * cos4 * tail))  # 0 * inf -> 0 (the header's guard)


def bsdf_ct_lambda(A, ax, ay, w):
    t2 = bsdf_tan2theta(A, w)
    if A.isinf(t2):
        return A.c(0)
    ay_ = ax if A.mut == "alpha_x for both axes" else ay
    alpha2 = _sqr(bsdf_cosphi(A, w) * ax) + _sqr(bsdf_sinphi(A, w) * ay_)
    return A.div(A.ieee_sqrt(1 + alpha2 * t2) - 1, A.c(2))


def bsdf_ct_G1(A, ax, ay, w):
    return A.div(A.c(1), 1 + bsdf_ct_lambda(A, ax, ay, w))


def bsdf_ct_G(A, ax, ay, wo, wi):
    if A.mut == "ct_G = G1 * G1":
        return bsdf_ct_G1(A, ax, ay, wo) * bsdf_ct_G1(A, ax, ay, wi)
    return A.div(A.c(1), 1 + bsdf_ct_lambda(A, ax, ay, wo) + bsdf_ct_lambda(A, ax, ay, wi))


def bsdf_ct_Dv(A, ax, ay, w, wm):
    return A.div(bsdf_ct_G1(A, ax, ay, w), abs(w[2])) * bsdf_ct_D(A, ax, ay, wm) * abs(_dot(w, wm))


def _cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _cdiv(A, a, z):
    scale = A.div(A.c(1), z[0] * z[0] + z[1] * z[1])
    return (scale * (a[0] * z[0] + a[1] * z[1]), scale * (a[1] * z[0] - a[0] * z[1]))


def _cnorm(z):
    return z[0] * z[0] + z[1] * z[1]


def bsdf_csqrt(A, z):
    n = A.ieee_sqrt(_cnorm(z))
    if A.eq0(n):
        return (A.c(0), A.c(0))
    t1 = A.ieee_sqrt(A.c(0.5) * (n + abs(z[0])))
    t2 = A.div(A.c(0.5) * z[1], t1)
    if A.ge(z[0], A.c(0)):
        return (t1, t2)
    return (abs(t2), t1 if A.ge(z[1], A.c(0)) else -t1)


def bsdf_fr_complex(A, cos_i, eta, k):
    c = A.clamp(cos_i, A.c(0), A.c(1))
    e = (eta, k)
    zero = A.c(0)
    s2 = 1 - _sqr(c)
    s2t = _cdiv(A, (s2, zero), _cmul(e, e))
    ct = bsdf_csqrt(A, (1 - s2t[0], zero - s2t[1]))
    ec = _cmul(e, (c, zero))
    r_parl = _cdiv(A, (ec[0] - ct[0], ec[1] - ct[1]), (ec[0] + ct[0], ec[1] + ct[1]))
    ect = _cmul(e, ct)
    r_perp = _cdiv(A, (c - ect[0], zero - ect[1]), (c + ect[0], zero + ect[1]))
    return A.div(_cnorm(r_parl) + _cnorm(r_perp), A.c(2))


def bsdf_ct_fresnel(A, eta, k, wo, wm):
    c = abs(_dot(wo, wm))
    out, seen = [], {}
    for ch in range(3):
        key = (A.val(eta[ch]), A.val(k[ch]))
        if key not in seen:
            seen[key] = bsdf_fr_complex(A, c, eta[ch], k[ch])
        out.append(seen[key])
    return out


def bsdf_ct_sample_wm(A, ax, ay, w, u):
    wh = A.normalize([ax * w[0], ay * w[1], w[2]])
    if A.lt(wh[2], A.c(0)):
        wh = _vneg(wh)
    zero, one = A.c(0), A.c(1)
    T1 = A.normalize(_cross([zero, zero, one], wh)) if A.lt(wh[2], A.c(0.99999)) else [one, zero, zero]
    T2 = _cross(wh, T1)
    r = A.ieee_sqrt(u[0])
    sn, cs = A.sincos_any(u[1])
    p = [r * cs, r * sn]
    om = 1 - u[0]
    h = A.ieee_sqrt(om + u[0] * _sqr(sn))
    lx = A.div(1 + wh[2], A.c(2))
    hp, hm = h + p[1], h - p[1]
    if A.ge(p[1], zero):
        hm = A.fast_div(om, hp)
    else:
        hp = A.fast_div(om, hm)
    pz = A.ieee_sqrt(A.fmax(zero, lx * hm * (2 * (1 - lx) * h + lx * hp)))
    p[1] = (1 - lx) * h + lx * p[1]
    nh = _vadd(_vadd(_vscale(T1, p[0]), _vscale(T2, p[1])), _vscale(wh, pz))
    return A.normalize([ax * nh[0], ay * nh[1], A.fmax(A.c(1e-6), nh[2])])


def _mix64(z):
    m = (1 << 64) - 1
    z &= m
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & m
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & m
    return z ^ (z >> 31)


def seed_state(seed, pixel, sample):
    """Rng::seed(seed, pixel, sample): the state the device and the oracle start a (pixel, sample) stream from."""
    key = _mix64(seed + 0x9E3779B97F4A7C15)
    return _mix64(((((key >> 32) ^ (pixel + 1)) & 0xFFFFFFFF) << 32) | ((key ^ (sample + 1)) & 0xFFFFFFFF)) or 0x9E3779B97F4A7C15


def raw_material(m):
    """The 17 raw fields of a scenes.Material (no lobe override)."""
    return (float(m.type),) + tuple(map(float, m.kd)) + tuple(map(float, m.ks)) + (float(m.ns),) + tuple(map(float, m.eta)) + \
        tuple(map(float, m.k)) + (float(m.alpha_x), float(m.alpha_y), -1.0)


class RngModel:
    """Rng::next on one 64-bit state: lattice values as Python floats, the number of draws, the state after them."""

    def __init__(self, state, f32):
        self.s, self.f32, self.n = np.uint64(state if state else 0x9E3779B97F4A7C15), f32, 0

    def next(self):
        r, self.s = rng_next(self.s)
        self.n += 1
        return float(int(r) >> 8) / 2.0 ** 24 if self.f32 else float(int(r) >> 1) / 2.0 ** 31


def bsdf_disk_concentric(A, ux, uy):
    ox, oy = 2 * ux - 1, 2 * uy - 1
    if A.eq0(ox) and A.eq0(oy):
        return [A.c(0), A.c(0)]
    if A.gt(abs(ox), abs(oy)):
        sn, cs = A.sincos_quarter(A.c(mpmath.pi / 4) * A.fast_div(oy, ox))
        return [ox * cs, ox * sn]
    cs, sn = A.sincos_quarter(A.c(mpmath.pi / 4) * A.fast_div(ox, oy))
    return [oy * cs, oy * sn]


def bsdf_cosine_hemisphere(A, rng):
    first = A.inp(rng.next())
    second = A.inp(rng.next())
    d = bsdf_disk_concentric(A, second, first)
    z = A.fast_sqrt(A.fmax(A.c(0), 1 - d[0] * d[0] - d[1] * d[1]))
    return [d[0], d[1], z]


def _cosine_above(A, rng):
    wi = bsdf_cosine_hemisphere(A, rng)
    for _ in range(16):
        if A.gt(wi[2], A.c(0), "wi.z > 0"):
            return wi
        wi = bsdf_cosine_hemisphere(A, rng)
    raise Undefined("sixteen cosine samples on the rim")


def _reflect_z(A, wo):
    zero, one = A.c(0), A.c(1)
    dn = wo[0] * zero + wo[1] * zero + wo[2] * one
    n2 = _vscale([zero, zero, one], 2 * dn)
    return _vadd(_vneg(wo), n2)


def _world_to_local(A, w, n, t):
    bit = _cross(t, n)
    return [_dot(w, t), _dot(w, bit), _dot(w, n)]


def _local_to_world(A, l, n, t):
    bit = _cross(t, n)
    return A.normalize(_vadd(_vadd(_vscale(t, l[0]), _vscale(bit, l[1])), _vscale(n, l[2])))


class Mat:
    """An untextured material from its raw fields; the derived ones as scene_setup.cpp fills them (in double, from ns),
    rounded to the precision as the fp32 material table is.  pkd >= 0 overrides the lobe probabilities with (pkd, 1 - pkd)."""

    def __init__(self, A, raw):
        raw = [A.P.rnd(x) for x in raw]
        self.type = int(raw[0])
        self.kd, self.ks = [A.inp(x) for x in raw[1:4]], [A.inp(x) for x in raw[4:7]]
        ns = raw[7]
        self.ns = A.inp(ns)
        self.inv_ns1 = A.inp(1.0 / (ns + 1.0))
        self.spec_scale = A.inp((ns + 2.0) / (ns + 1.0))
        self.pkd, self.pks = (A.inp(1.0), A.inp(0.0)) if ns <= 9.0 else (A.inp(0.6), A.inp(0.4))
        if raw[16] >= 0:
            self.pkd = A.inp(raw[16])
            self.pks = A.inp(A.P.rnd(A.P.rnd(1.0) - raw[16]))
        self.eta, self.k = [A.inp(x) for x in raw[8:11]], [A.inp(x) for x in raw[11:14]]
        self.ax, self.ay = A.inp(raw[14]), A.inp(raw[15])


def bsdf_mat_eval(A, m, wi, wo, rng):
    zero = A.c(0)
    z3 = [zero, zero, zero]
    if m.type == 0:
        return _vscale(m.kd, A.c(1 / mpmath.pi))
    if m.type == 1:
        u = A.inp(rng.next())
        if A.lt(u, m.pkd, "u < pkd"):
            if not A.gt(wi[2], zero):
                return z3
            return _vscale(m.kd, A.c(1 / mpmath.pi))
        if A.lt(u, A.round_sum(m.pkd, m.pks)):
            if not A.gt(wi[2], zero):
                return z3
            lr = A.normalize(_reflect_z(A, wo))
            ca = A.fmax(zero, _dot(wi, lr))
            if not A.gt(ca, zero):
                return z3
            return _vscale(_vscale(_vscale(m.ks, m.ns + A.c(2)), A.c(1 / (2 * mpmath.pi))), A.pow_pos(ca, m.ns))
        return z3
    if m.type == 3:
        if not A.gt(wo[2] * wi[2], zero, "wo.z * wi.z > 0"):
            return z3
        co, ci = abs(wo[2]), abs(wi[2])
        if A.eq0(ci, "ci == 0") or A.eq0(co):
            return z3
        wm = _vadd(wi, wo)
        if A.eq0(_sqr(wm[0]) + _sqr(wm[1]) + _sqr(wm[2]), "wm == 0"):
            return z3
        wm = A.normalize(wm)
        F = bsdf_ct_fresnel(A, m.eta, m.k, wo, wm)
        D = bsdf_ct_D(A, m.ax, m.ay, wm)
        return _vdiv(A, _vscale([D * f for f in F], bsdf_ct_G(A, m.ax, m.ay, wo, wi)), 4 * ci * co)
    return z3


def bsdf_mat_scatter(A, m, rd, n, t, rng):
    """(ok, wi_world, att, closed form of att or None, the local wi)"""
    zero, one = A.c(0), A.c(1)
    z3 = [zero, zero, zero]
    if m.type == 0:
        wi = _cosine_above(A, rng)
        pdf = wi[2] * A.c(1 / mpmath.pi)
        fr = _vscale(m.kd, A.c(1 / mpmath.pi))
        r = A.fast_rcp(pdf)
        return True, _local_to_world(A, wi, n, t), [(f * wi[2]) * r for f in fr], m.kd, wi
    if m.type == 1:
        wo = _world_to_local(A, _vneg(rd), n, t)
        u = A.inp(rng.next())
        if A.lt(u, m.pkd, "u < pkd"):
            wi = _cosine_above(A, rng)
            pdf = wi[2] * A.c(1 / mpmath.pi)
            fr = _vscale(m.kd, A.c(1 / mpmath.pi))
            ww = _local_to_world(A, wi, n, t)
            return True, ww, _vdiv(A, _vscale(fr, wi[2]), pdf), m.kd, wi  # pdf > 0 and wi.z > 0: the loop left with wi.z > 0
        if not A.lt(u, A.round_sum(m.pkd, m.pks)):
            raise Undefined("neither lobe: local_to_world normalizes the zero vector")
        u1, u2 = A.inp(rng.next()), A.inp(rng.next())
        ca = A.fmin(A.pow_pos(u1, m.inv_ns1), one)
        sa = A.ieee_sqrt(A.fmax(zero, 1 - ca * ca))
        sp, cp = A.sincos_turns(u2)
        rw = [sa * cp, sa * sp, ca]
        lr = A.normalize(_reflect_z(A, wo))
        Vv = [zero, one, zero] if A.gt(abs(lr[0]), A.c(0.9), "|lr.x| > 0.9") else [one, zero, zero]
        T = A.normalize(_cross(Vv, lr))
        B = _cross(lr, T)
        wi = _vadd(_vadd(_vscale(T, rw[0]), _vscale(B, rw[1])), _vscale(lr, rw[2]))
        up = A.gt(wi[2], zero, "wi.z > 0")
        ok = up and A.gt(u1, zero)
        fr = _vscale(m.ks, m.spec_scale)
        ww = _local_to_world(A, wi, n, t)
        return True, ww, (_vscale(fr, wi[2]) if ok else z3), ([f * wi[2] for f in fr] if ok else z3), wi
    if m.type == 2:
        wo = _world_to_local(A, _vneg(rd), n, t)
        wi = _reflect_z(A, wo)
        c = wi[2]
        fr = [A.div(one, c)] * 3
        return True, _local_to_world(A, wi, n, t), _vdiv(A, _vscale(fr, c), one), [one, one, one], wi
    if m.type == 3:
        wo = A.normalize(_world_to_local(A, _vneg(rd), n, t))
        if A.eq0(wo[2]):
            return False, z3, z3, None, z3
        first = A.inp(rng.next())
        second = A.inp(rng.next())
        wm = bsdf_ct_sample_wm(A, m.ax, m.ay, wo, [second, first])
        wi = _vadd(_vneg(wo), _vscale(wm, 2 * _dot(wo, wm)))
        if not A.gt(wo[2] * wi[2], zero, "wo.z * wi.z > 0"):
            return False, z3, z3, None, wi
        pdf = A.div(bsdf_ct_Dv(A, m.ax, m.ay, wo, wm), 4 * abs(_dot(wo, wm)))
        co, ci = abs(wo[2]), abs(wi[2])
        if A.eq0(ci, "ci == 0") or A.eq0(co):
            return False, z3, z3, None, wi
        F = bsdf_ct_fresnel(A, m.eta, m.k, wo, wm)
        D = bsdf_ct_D(A, m.ax, m.ay, wm)
        G = bsdf_ct_G(A, m.ax, m.ay, wo, wi)
        fr = _vdiv(A, _vscale([D * f for f in F], G), 4 * ci * co)
        att = _vdiv(A, _vscale(fr, wi[2]), pdf)
        closed = None
        if A.exact:  # F * G(wo, wi) / G1(wo) on the model's own (exact) directions
            closed = [f.v * G.v / bsdf_ct_G1(A, m.ax, m.ay, wo).v for f in F]
        return True, _local_to_world(A, wi, n, t), att, closed, wi
    return False, z3, z3, None, z3


# ------------------------------------------------------------------ material parameters, inputs by stratum
def alpha_values_in_sources():
    """Every (alpha_x, alpha_y) written in scenes.py and tests/: `alpha_x=<number>, alpha_y=<number>` literals and the
    dataclass defaults `alpha_x: float = <number>`."""
    found = set()
    for text in _material_sources():
        found |= {(float(a), float(b)) for a, b in re.findall(r"\balpha_x=(%s)\s*,\s*alpha_y=(%s)" % (_NUM, _NUM), text)}
        dx = re.findall(r"\balpha_x: float = (%s)" % _NUM, text)
        dy = re.findall(r"\balpha_y: float = (%s)" % _NUM, text)
        found |= {(float(a), float(b)) for a, b in zip(dx, dy)}
    return sorted(found)


def bsdf_alphas():
    return alpha_values_in_sources() + [(1e-3, 1e-3), (1.0, 1.0), (0.01, 1.0)]


def bsdf_materials():
    """Raw 17-field rows: one Lambertian, a mirror, Phong for every Ns in the sources with the real and the two forced lobe
    probabilities, CookTorrance for every alpha pair with the (eta, k) channels of the sources dealt round."""
    kd, ks = (0.7, 0.4, 0.2), (0.9, 0.5, 0.3)
    z3 = (0.0, 0.0, 0.0)
    mats = {"lambert": [(0.0,) + kd + z3 + (0.0,) + z3 + z3 + (0.3, 0.3, -1.0)],
            "mirror": [(2.0,) + kd + z3 + (0.0,) + z3 + z3 + (0.3, 0.3, -1.0)], "phong": [], "ct": []}
    for ns in ns_values_in_sources():
        for pkd in (-1.0, 0.0, 1.0):
            mats["phong"].append((1.0,) + kd + ks + (ns,) + z3 + z3 + (0.3, 0.3, pkd))
    ek = eta_k_in_sources()
    for i, (ax, ay) in enumerate(bsdf_alphas() * 2):
        ch = [ek[(3 * i + j) % len(ek)] for j in range(3)]
        mats["ct"].append((3.0,) + kd + z3 + (0.0,) + tuple(c[0] for c in ch) + tuple(c[1] for c in ch) + (ax, ay, -1.0))
    return {k: np.array(v) for k, v in mats.items()}


def _unit(z, phi):
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=-1)


def off_unit_vector(w, j, prec):
    """The vector of the precision nearest to w whose EXACT |w|^2 - 1 is as close to j ulp of 1 (2^-52 / 2^-23) as stepping its
    components through neighbouring numbers gets it: largest component first (coarse), smallest last (fine)."""
    dt = PRECS[prec].dtype
    ulp1 = Fraction(1, 2 ** (23 if prec == "f32" else 52))
    v = np.asarray(w, dtype=np.float64).astype(dt)
    for _ in range(2):
        for i in np.argsort(-np.abs(v)):
            r = sum(Fraction(float(c)) ** 2 for c in v) - 1
            c = float(v[i])
            gain = 2 * abs(Fraction(c)) * Fraction(float(np.spacing(dt(abs(c)))))  # change of |w|^2 per step away from zero
            steps = int(round((j * ulp1 - r) / gain))
            toward = dt(np.inf if (steps > 0) == (c > 0) else -np.inf)
            for _ in range(min(abs(steps), 64)):
                v[i] = np.nextafter(v[i], toward)
    return v.astype(np.float64)


def off_unit_residual(w, prec):
    """Exact |w|^2 - 1 of the rounded vector, in ulps of 1."""
    dt = PRECS[prec].dtype
    return float((sum(Fraction(float(dt(c))) ** 2 for c in w) - 1) * 2 ** (23 if prec == "f32" else 52))


def direction_strata(prec, seed=41):
    """Local-frame directions (z the shading normal) by stratum, in float64 (the probe and the model round them)."""
    rng = np.random.default_rng(seed)
    f32 = prec == "f32"
    out = {}
    n = 160
    out["random"] = _unit(rng.uniform(0.02, 1.0, n), rng.uniform(0, 2 * np.pi, n))
    k = np.arange(65.0)
    z = 1 - k * 2.0 ** -23 if f32 else np.concatenate([1 - k * 2.0 ** -23, 1 - k * 2.0 ** -52])  # the 1 - z^2 cancellation (2^-52 steps all round to 1 in fp32)
    out["near_normal"] = _unit(z, rng.uniform(0, 2 * np.pi, z.size))
    w = _unit(rng.uniform(0.05, 1.0, 32), rng.uniform(0.1, np.pi / 2 - 0.1, 32) + np.repeat(np.arange(4) * np.pi / 2, 8))
    out["off_unit"] = np.array([off_unit_vector(v, j, prec) for v, j in zip(w, np.tile([-2, -1, 1, 2], 8))])
    e = np.arange(1, (60 if f32 else 500) + 1)
    out["grazing"] = _unit(2.0 ** -e.astype(np.float64), rng.uniform(0, 2 * np.pi, e.size))
    ax = _unit(rng.uniform(0.1, 0.9, 8), np.array([0, np.pi, 0, np.pi, np.pi / 2, -np.pi / 2, np.pi / 2, -np.pi / 2]))
    ax[:4, 1] = 0.0   # w.y == 0 exactly
    ax[4:, 0] = 0.0   # w.x == 0 exactly
    out["axes"] = np.concatenate([ax, [[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0], [0, 1.0, 0]]])
    return out


def _cycle(a, n, start=0):
    return a[(np.arange(n) + start) % len(a)]


def _deal(classes, n, start=0):
    """n material rows dealt round the CLASSES (row i takes class i mod len(classes)), each class cycling through its own
    members: every class is in every stratum of at least len(classes) rows, whatever the sizes of the classes."""
    out = []
    for i in range(n):
        c = classes[i % len(classes)]
        out.append(c[(i // len(classes) + start) % len(c)])
    return np.array(out)


def bsdf_inputs(name, prec, seed=43):
    """(rows, states or None, stratum name per row) for probe `name`; <= 2^16 rows."""
    S = direction_strata(prec)
    rng = np.random.default_rng(seed)
    P = PRECS[prec]
    al = np.array(bsdf_alphas())
    rows, strat, states = [], [], None
    if name in ("tan2theta", "cosphi", "sinphi"):
        for s, w in S.items():
            rows.append(w), strat.extend([s] * len(w))
    elif name in ("ct_D", "ct_lambda", "ct_G1"):
        for s, w in S.items():
            for off in (0, 3):
                rows.append(np.concatenate([_cycle(al, len(w), off), w], 1)), strat.extend([s] * len(w))
    elif name in ("ct_G", "ct_Dv", "ct_fresnel"):
        ek = np.array(eta_k_in_sources())
        pairs = [("random", S["random"], S["random"][::-1]), ("near_normal", S["near_normal"], S["near_normal"][::-1]),
                 ("off_unit", S["off_unit"], S["off_unit"][::-1]), ("grazing_one", S["grazing"], _cycle(S["random"], len(S["grazing"]))),
                 ("grazing_other", _cycle(S["random"], len(S["grazing"])), S["grazing"]),
                 ("grazing_both", S["grazing"], S["grazing"][::-1] * np.array([-1.0, 1.0, 1.0])),
                 ("axes", S["axes"], S["axes"][::-1]), ("below", S["random"] * np.array([1.0, 1.0, -1.0]), S["random"][::-1])]
        for s, a, b in pairs:
            if name == "ct_fresnel":
                m = np.concatenate([_cycle(ek, len(a))[:, :1], _cycle(ek, len(a), 1)[:, :1], _cycle(ek, len(a), 2)[:, :1],
                                    _cycle(ek, len(a))[:, 1:], _cycle(ek, len(a), 1)[:, 1:], _cycle(ek, len(a), 2)[:, 1:]], 1)
            else:
                m = _cycle(al, len(a))
            if name == "ct_fresnel" and s.startswith("grazing"):  # F depends on |wo . wm| alone: every fourth exponent
                m, a, b = m[::4], a[::4], b[::4]
            rows.append(np.concatenate([m, a, b], 1)), strat.extend([s] * len(a))
    elif name in ("mat_eval", "mat_scatter"):
        mats = bsdf_materials()
        allm = [mats["ct"], mats["phong"], mats["lambert"]]  # the classes Eval knows (the mirror's Eval is 0)
        top = (1 << P.bits) - 1
        ends = np.array([0, 1, 1 << (P.bits - 1), top], dtype=np.uint64)
        st = []

        def rand_states(k):
            return rng.integers(1, 1 << 63, size=k).astype(np.uint64)

        def add(s, m, dirs, state):
            rows.append(np.concatenate([m] + dirs, 1)), strat.extend([s] * len(m)), st.append(state)

        if name == "mat_eval":
            R, Rr = S["random"], S["random"][::-1]
            add("random", _deal(allm, 2 * len(R)), [np.concatenate([R, R]), np.concatenate([Rr, np.roll(R, 7, 0)])], rand_states(2 * len(R)))
            # opposite sides and exact zeros: exactly 0 for CookTorrance; Phong returns 0 for wi.z <= 0
            neg = np.array([1.0, 1.0, -1.0])
            zz = np.array([[1.0, 0, 0], [0, 1.0, 0], [0.6, 0.8, 0], [0, 0, 0]])
            a = np.concatenate([R[:24] * neg, R[:24], _cycle(zz, 24), R[:24], _cycle(zz, 24)])
            b = np.concatenate([Rr[:24], Rr[:24] * neg, Rr[:24], _cycle(zz, 24), _cycle(zz, 24, 1)])
            add("opposite_or_zero", _deal([mats["ct"], mats["phong"][2::3]], len(a)), [a, b], rand_states(len(a)))
            # wi near the normal against a random wo, and against itself mirrored in azimuth: wm = normalize(wi + wo) on the axis
            N = S["near_normal"]
            add("near_normal", _deal(allm, 2 * len(N), 1), [np.concatenate([N, N]), np.concatenate([_cycle(Rr, len(N)), N * np.array([-1.0, -1.0, 1.0])])],
                rand_states(2 * len(N)))
            for s in ("off_unit", "axes"):
                add(s, _deal(allm, len(S[s]), 2), [S[s], S[s][::-1]], rand_states(len(S[s])))
            G = S["grazing"]
            odd = (np.arange(len(G)) % 2 == 1)[:, None]  # one direction alone grazes: wi at the even exponents, wo at the odd ones
            add("grazing_one", _cycle(mats["ct"], len(G)), [np.where(odd, _cycle(R, len(G)), G), np.where(odd, G, _cycle(R, len(G)))], rand_states(len(G)))
            turn = np.array([[0.0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])  # another azimuth, the same z: wm grazes as well
            add("grazing_both", _cycle(mats["ct"], len(G), 2), [G, G @ turn.T], rand_states(len(G)))
            ph = mats["phong"]
            k1, k2 = np.meshgrid(ends, ends, indexing="ij")
            cs = craft_state(k1.ravel(), k2.ravel(), shift=P.shift)
            m = np.repeat(ph, len(cs), 0)
            add("rng_ends", m, [_cycle(R, len(m)), _cycle(Rr, len(m), 3)], np.tile(cs, len(ph)))
        else:
            n0, t0 = np.array([0, 0, 1.0]), np.array([1.0, 0, 0])
            n1 = np.array([2.0, -1.0, 2.0]) / 3.0
            t1 = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
            b1 = np.cross(t1, n1)  # bit = cross(t, n): a local (x, y, z) is x t + y bit + z n in the world
            allm = allm + [mats["mirror"]]

            def frame(k, tilted=False):
                n, t = (n1, t1) if tilted else (n0, t0)
                return [np.broadcast_to(n, (k, 3)), np.broadcast_to(t, (k, 3))]

            def world(w, tilted):  # rd = -wo, wo given in the local frame
                if not tilted:
                    return -(w * np.array([1.0, -1.0, 1.0]))  # bit = cross((1,0,0), (0,0,1)) = (0,-1,0)
                return -(w[:, :1] * t1 + w[:, 1:2] * b1 + w[:, 2:] * n1)

            R = S["random"]
            scale = np.where(np.arange(len(R)) % 3 == 0, 2.5, 1.0)[:, None]  # camera rays come in unnormalised
            add("random", _deal(allm, len(R)), [world(R, False) * scale] + frame(len(R)), rand_states(len(R)))
            add("random_tilted_frame", _deal(allm, len(R), 11), [world(R, True) * scale] + frame(len(R), True), rand_states(len(R)))
            # wo.z == 0 exactly: CookTorrance returns false without a draw.  (wo below the surface is outside Scatter's domain:
            # the frame's normal is face-forwarded; the mirror's 1 / wi.z is 1 / 0 at wo.z == 0, as in the reference.)
            zz = np.array([[1.0, 0, 0], [0, 1.0, 0], [0.6, 0.8, 0], [0.6, -0.8, 0]])
            add("zero", _deal(allm[:3], 48), [world(_cycle(zz, 48), False)] + frame(48), rand_states(48))
            for s in ("near_normal", "off_unit", "axes"):
                w = S[s][S[s][:, 2] > 0] if s == "axes" else S[s]  # (wo.z > 0: see above)
                w = np.concatenate([w, w]) if s == "axes" else w
                add(s, _deal(allm, len(w), 2), [world(w, False)] + frame(len(w)), rand_states(len(w)))
            G = S["grazing"]
            add("grazing", _deal([mats["ct"], mats["ct"], mats["phong"], mats["lambert"], mats["mirror"]], len(G)), [world(G, False)] + frame(len(G)), rand_states(len(G)))
            k1, k2 = np.meshgrid(ends, ends, indexing="ij")
            cs = craft_state(k1.ravel(), k2.ravel(), shift=P.shift)
            mm = np.concatenate([mats["lambert"], mats["ct"][:7], mats["phong"]])
            m = np.repeat(mm, len(cs), 0)
            kk1, kk2 = np.tile(k1.ravel(), len(mm)), np.tile(k2.ravel(), len(mm))
            add("rng_ends", m, [world(_cycle(R, len(m)), False)] + frame(len(m)), np.tile(cs, len(mm)))
            # A cosine-hemisphere sample whose draw is 0 lies ON the disk's rim (|2u - 1| = 1; in fp32 the top of the lattice
            # is within the map's rounding of it): z^2 = 1 - x^2 - y^2 is 0 up to rounding, `wi.z > 0` is a knife edge by
            # construction and the loop may draw again (in fp32 one lattice step from either end is still within that rounding:
            # z^2 ~ 2^-22 against an error of a few 2^-24).  Those rows are a stratum of their own, to which the knife-edge cap
            # cannot apply; they are still checked for finiteness, sign and the closed form of att.
            rim_draw = lambda k: (k == 0) | (((k == top) | (k == 1)) if P.f32 else False)
            pkd_eff = np.where(m[:, 16] >= 0, m[:, 16], np.where(m[:, 7] <= 9.0, 1.0, 0.6))
            u_first = kk1.astype(np.float64) / 2.0 ** P.bits
            rim = np.where(m[:, 0] == 0, rim_draw(kk1) | rim_draw(kk2), (m[:, 0] == 1) & (u_first < pkd_eff) & rim_draw(kk2))
            tail = strat[len(strat) - len(m):]
            strat[len(strat) - len(m):] = ["rng_rim" if r else t for r, t in zip(rim, tail)]
        states = np.concatenate(st)
    else:
        raise KeyError(name)
    rows = np.concatenate(rows)
    with np.errstate(all="ignore"):
        rows = rows.astype(P.dtype).astype(np.float64)  # what the probe sees
    assert len(rows) <= 1 << 16 and len(strat) == len(rows)
    return rows, states, np.array(strat)


# ------------------------------------------------------------------ evaluation of one probe on its rows
BSDF_OPS = {"tan2theta": 1, "cosphi": 1, "sinphi": 1, "ct_D": 1, "ct_lambda": 1, "ct_G1": 1, "ct_G": 1, "ct_Dv": 1, "ct_fresnel": 3,
            "mat_eval": 3, "mat_scatter": 7}
BSDF_NONNEG = {"tan2theta", "ct_D", "ct_lambda", "ct_G1", "ct_G", "ct_Dv", "ct_fresnel", "mat_eval"}  # outputs that are >= 0
BSDF_LE1 = {"ct_G1", "ct_G"}


def _bsdf_call(A, name, r, state):
    """Outputs of probe `name` on one row, in backend A; for the two state probes also (rng, closed form, local wi)."""
    x = [A.inp(v) for v in r]
    if name == "tan2theta":
        return [bsdf_tan2theta(A, x)], None
    if name == "cosphi":
        return [bsdf_cosphi(A, x)], None
    if name == "sinphi":
        return [bsdf_sinphi(A, x)], None
    if name in ("ct_D", "ct_lambda", "ct_G1"):
        return [{"ct_D": bsdf_ct_D, "ct_lambda": bsdf_ct_lambda, "ct_G1": bsdf_ct_G1}[name](A, x[0], x[1], x[2:5])], None
    if name in ("ct_G", "ct_Dv"):
        return [{"ct_G": bsdf_ct_G, "ct_Dv": bsdf_ct_Dv}[name](A, x[0], x[1], x[2:5], x[5:8])], None
    if name == "ct_fresnel":
        return bsdf_ct_fresnel(A, x[0:3], x[3:6], x[6:9], x[9:12]), None
    rng = RngModel(state, A.P.f32)
    m = Mat(A, r[:MAT_NI])
    d = x[MAT_NI:]
    if name == "mat_eval":
        return bsdf_mat_eval(A, m, d[0:3], d[3:6], rng), (rng, None, None)
    ok, ww, att, closed, wi = bsdf_mat_scatter(A, m, d[0:3], d[3:6], d[6:9], rng)
    return [A.c(1.0 if ok else 0.0)] + list(ww) + list(att), (rng, closed, wi)


def _to_ld(v):
    if abs(v) == INF:
        return LD(np.inf) if v > 0 else LD(-np.inf)
    return LD(mpmath.nstr(v, 24))


_BSDF_CACHE = {}


def bsdf_reference(name, prec, rows=None, states=None):
    """The model on bsdf_inputs(name, prec) (computed once per process) or on the given rows: a dict with rows, states,
    stratum, ref (longdouble), bound (the running bound), tol = 2 * bound + one subnormal quantum, knife (bool per row) and
    knife_names, undef (bool per row: 0/0 in exact arithmetic, nothing is asserted), and for the state probes state_after,
    draws, closed (the closed form of att)."""
    key = (name, prec)
    if rows is None and key in _BSDF_CACHE:
        return _BSDF_CACHE[key]
    if rows is None:
        rows, states, strat = bsdf_inputs(name, prec)
    else:
        key = None
        with np.errstate(all="ignore"):
            rows = np.asarray(rows, dtype=np.float64).astype(PRECS[prec].dtype).astype(np.float64)
        strat = np.array(["given"] * len(rows))
    n, no = len(rows), BSDF_OPS[name]
    P = PRECS[prec]
    ref = np.zeros((n, no), dtype=LD)
    bound = np.zeros((n, no))
    knife, undef = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    names = [""] * n
    after = np.zeros(n, dtype=np.uint64)
    draws = np.zeros(n, dtype=np.int64)
    closed = np.full((n, 3), np.nan, dtype=LD)
    for i in range(n):
        A = MpArith(prec)
        try:
            out, extra = _bsdf_call(A, name, rows[i], None if states is None else states[i])
        except Undefined as ex:
            undef[i], names[i] = True, str(ex)
            continue
        for j, o in enumerate(out):
            o = A.of(o)
            ref[i, j] = _to_ld(o.v)
            bound[i, j] = np.inf if o.e == INF else float(o.e)
        if A.knife:
            knife[i], names[i] = True, ", ".join(sorted(set(A.knife)))
        if extra:
            after[i], draws[i] = extra[0].s, extra[0].n
            if extra[1] is not None:
                closed[i] = [_to_ld(c.v if isinstance(c, V) else mpf(c)) for c in extra[1]]
    R = dict(name=name, prec=prec, rows=rows, states=states, stratum=strat, ref=ref, bound=bound, tol=2 * bound + float(P.quantum),
             knife=knife, knife_names=names, undef=undef, state_after=after, draws=draws, closed=closed)
    if key:
        _BSDF_CACHE[key] = R
    return R


def bsdf_numpy(name, prec, mut=None, rows=None, states=None):
    """The plain numpy restatement (IEEE operations of the precision only) on the same rows: (outputs, state after)."""
    if rows is None:
        rows, states, _ = bsdf_inputs(name, prec)
    P = PRECS[prec]
    out = np.full((len(rows), BSDF_OPS[name]), np.nan, dtype=P.dtype)
    after = np.zeros(len(rows), dtype=np.uint64)
    with np.errstate(all="ignore"):
        for i in range(len(rows)):
            A = NpArith(prec, mut)
            try:
                o, extra = _bsdf_call(A, name, rows[i], None if states is None else states[i])
            except Undefined:
                continue
            out[i] = [P.dtype(v) for v in o]
            if extra:
                after[i] = extra[0].s
    return out, after


def bsdf_compare(R, got, state_after=None, what="device"):
    """Holds `got` (n, outputs) against the reference R = bsdf_reference(..).  Returns (error / tolerance per row, the failures
    as a list of strings); prints the worst ratio with its input and the worst relative error per stratum."""
    name, prec = R["name"], R["prec"]
    P = PRECS[prec]
    mx = float(P.max)
    g = got.astype(LD)
    ref, tol = R["ref"], R["tol"]
    live = ~R["undef"]
    fails = []
    with np.errstate(all="ignore"):
        exact_finite = np.isfinite(ref) & (np.abs(ref) <= mx)
        bad = live[:, None] & exact_finite & ~np.isfinite(got)
        if bad.any():
            i = int(np.nonzero(bad.any(1))[0][0])
            fails.append(f"{int(bad.any(1).sum())} rows are NaN / inf where the exact value is finite, first: row {i} [{R['stratum'][i]}] "
                         f"{R['rows'][i].tolist()} -> {got[i].tolist()} (exact {ref[i].astype(np.float64).tolist()})")
        # where the exact value is infinite the device must hold that infinity; where it is finite but beyond the largest
        # number of the precision, that infinity or a finite number of its sign — never NaN
        is_inf = live[:, None] & np.isinf(ref)
        wrong = is_inf & (got.astype(np.float64) != ref.astype(np.float64))
        over = live[:, None] & np.isfinite(ref) & (np.abs(ref) > mx) & (np.isnan(got) | (np.sign(got) != np.sign(ref.astype(np.float64))))
        if wrong.any() or over.any():
            i = int(np.nonzero((wrong | over).any(1))[0][0])
            fails.append(f"{int((wrong | over).any(1).sum())} rows are not the infinity the exact value is (or NaN / wrongly signed where it overflows), "
                         f"first: row {i} [{R['stratum'][i]}] {R['rows'][i].tolist()} -> {got[i].tolist()} (exact {ref[i].astype(np.float64).tolist()})")
        nan_ref = live[:, None] & np.isnan(ref)
        if nan_ref.any():
            fails.append(f"{int(nan_ref.any(1).sum())} rows have a NaN reference without being marked undefined")
        cols = slice(4, 7) if name == "mat_scatter" else slice(None)
        if name in BSDF_NONNEG or name == "mat_scatter":
            neg = live[:, None] & (got[:, cols] < 0)
            if neg.any():
                i = int(np.nonzero(neg.any(1))[0][0])
                fails.append(f"negative output at row {i} [{R['stratum'][i]}] {R['rows'][i].tolist()} -> {got[i].tolist()}")
        if name in BSDF_LE1 and (live[:, None] & (got > 1)).any():
            fails.append("an output exceeds 1")
        err = np.abs(g - ref)
        ratio = np.where(np.isfinite(tol), err / tol, 0.0)
        ratio = np.where(np.isnan(ratio), np.where(exact_finite, np.inf, 0.0), ratio).astype(np.float64)
        checked = live & ~R["knife"]
        ratio[~checked] = 0
        rel = np.where(exact_finite & (np.abs(ref) >= float(P.tiny)), err / np.abs(ref), 0.0).astype(np.float64)
        rel[~np.isfinite(rel)] = np.inf
        rel[~checked] = 0
    row_ratio = ratio.max(1)
    i = int(np.argmax(row_ratio))
    print(f"[bsdf] {name} {prec} {what}: worst error / tolerance {row_ratio[i]:.4g} at row {i} [{R['stratum'][i]}] {R['rows'][i].tolist()}"
          f" -> {got[i].tolist()}, tolerance {tol[i].tolist()}; {int(R['knife'].sum())} knife-edge, {int(R['undef'].sum())} undefined of {len(row_ratio)}")
    for s in dict.fromkeys(R["stratum"].tolist()):
        sel = R["stratum"] == s
        fin = np.isfinite(tol[sel]).all(1) & checked[sel]
        print(f"[bsdf] {name} {prec} {what} [{s}]: {int(sel.sum())} rows, worst relative error {rel[sel][fin].max() if fin.any() else 0:.4g} "
              f"(rows with a finite bound: {int(fin.sum())}), worst ratio {row_ratio[sel].max():.4g}")
    if row_ratio[i] > 1:
        fails.append(f"{int((row_ratio > 1).sum())} rows leave the tolerance, worst {row_ratio[i]:.4g} at row {i}")
    if state_after is not None:
        ds = checked & (state_after != R["state_after"])
        if ds.any():
            i = int(np.nonzero(ds)[0][0])
            fails.append(f"{int(ds.sum())} rows leave the RNG in another state than the model's draws, first row {i} [{R['stratum'][i]}]")
    return row_ratio, fails


UNCAPPED_STRATA = {"rng_rim"}  # knife-edge by construction (see bsdf_inputs)


def unbounded_share(R):
    """Share of rows per stratum whose bound is infinite (checked for finiteness and sign only), as a dict."""
    inf = ~np.isfinite(R["tol"]).all(1) & ~R["undef"]
    return {s: float(inf[R["stratum"] == s].mean()) for s in dict.fromkeys(R["stratum"].tolist())}


def knife_edge_share(R):
    """The largest share of knife-edge rows in any stratum but the ones that are knife-edge by construction."""
    return max(float(R["knife"][R["stratum"] == s].mean()) for s in set(R["stratum"].tolist()) - UNCAPPED_STRATA)
