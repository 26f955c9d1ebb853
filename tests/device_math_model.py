"""References for the device primitives of pooraytracer_amd/csrc/prt_device.h (tests/test_gpu_device_math.py compares
the probe library tests/probe/libprt_probe.so with them; tests/test_device_math_cpu.py checks them against each other).

* mpmath at 60 digits: sqrt, reciprocal, division, sin, cos, pow, the complex square root, Fresnel, the Shirley-Chiu
  concentric map and the visible-normal sampler (Material.h:412-435 restated);
* fractions.Fraction for the FMA helpers: float(Fraction(a) * Fraction(b) + Fraction(k)) IS the correctly rounded result;
* numpy longdouble (64-bit mantissa) where 10^6-point grids make mpmath too slow (checked against mpmath on subsets);
* a model of Rng::next and its inverse: any pair of 31-bit draws is one 64-bit state;
* the exact box test and the case generators of tests/test_slab_cpu.py.
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
}
F64_ONLY_OPS = {"fma_sk": (2, 5), "mul_ks": (1, 5)}  # prt_device.h has no fp32 overload of these
OTHER_OPS = ["rng_next", "cosine_hemisphere", "f32_updown", "box4"]
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
