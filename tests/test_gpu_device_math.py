"""The device primitives of pooraytracer_amd/csrc/prt_device.h, run ON THEIR OWN through the test-only probe library
(tests/probe/) and compared with the high-precision references of tests/device_math_model.py.

The rest of the suite sees these functions only through whole kernels, with hashed random streams and the 1e-9 parity
tolerance.  Here the inputs are chosen (lattice ends, branch switches, binade edges, crafted RNG states) and the bounds are
the ones the code's comments state or the arithmetic gives — never what the probe happens to measure.  Every test prints
its measured maximum and where it occurred.
"""
import numpy as np
import pytest

from tests import device_math_model as M

pytestmark = pytest.mark.gpu
LD = np.longdouble
U64 = 2.0 ** -52  # one ulp of a binary64 in [1, 2)
U32 = 2.0 ** -24  # rounding unit (half an ulp in [1, 2)) of a binary32


@pytest.fixture(scope="module")
def probe(gpu):
    import torch  # noqa: F401
    return M.probe_lib()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run(L, name, prec, inp, no, out_dtype=None):
    """Element-wise probe `name` in precision `prec` on the rows of `inp`; returns the (n, no) outputs."""
    import torch
    dt = np.float64 if prec == "f64" else np.float32
    inp = np.ascontiguousarray(inp)
    if inp.dtype.kind == "f":
        inp = inp.astype(dt)
    n = inp.shape[0]
    flat = inp.reshape(-1)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(flat.dtype)
    d_in = torch.from_numpy(flat.view(view) if view else flat).cuda()
    d_out = torch.zeros(n * no, dtype=torch.float32 if (out_dtype or dt) == np.float32 else torch.float64, device="cuda")
    rc = getattr(L, f"prtprobe_{name}_{prec}")(d_in.data_ptr(), d_out.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, prec, rc)
    return d_out.cpu().numpy().reshape(n, no)


def report(what, err, where):
    i = int(np.nanargmax(err))
    print(f"[device-math] {what}: max {float(err[i]):.4g} at {where(i)}")
    return float(err[i])


# ================================================================== fp64 arithmetic
def _arith_inputs():
    rng = np.random.default_rng(21)
    k = np.arange(-4, 5)
    unit = np.concatenate([1.0 + k[k >= 0] * 2.0 ** -52, 1.0 + k[k < 0] * 2.0 ** -53])  # squared lengths of unit vectors
    return np.concatenate([M.binade_inputs(rng), M.lattice_ends(), unit])


def test_fast_arithmetic_fp64_is_within_two_ulp(probe):
    """The documented contract of fast_rsqrt / fast_sqrt / fast_rcp / fast_div (prt_device.h): within 2 ulp of the exact
    result for every positive normal argument — every binade 2^-1022 .. 2^1023, the RNG lattice ends, 1 +- a few ulp."""
    x = _arith_inputs()
    xl = x.astype(LD)
    rng = np.random.default_rng(22)
    a = 1.0 + rng.random(x.size)
    al = a.astype(LD)
    cases = [("fast_rsqrt", x[:, None], 1 / np.sqrt(xl)), ("fast_sqrt", x[:, None], np.sqrt(xl)), ("fast_rcp", x[:, None], 1 / xl),
             ("fast_div", np.stack([a, x], 1), al / xl), ("fast_div", np.stack([x, a], 1), xl / al),
             ("ieee_sqrt", x[:, None], np.sqrt(xl)), ("ieee_div", np.stack([a, x], 1), al / xl)]
    worst = {}
    for name, inp, ref in cases:
        got = run(probe, name, "f64", inp, 1)[:, 0]
        err = M.ulp_err(got, ref)
        err[~np.isfinite(got)] = np.inf
        worst[name] = max(worst.get(name, 0), report(f"{name} fp64 [ulp]", err, lambda i: f"x = {float(inp[i, -1]).hex()}"))
    for name, w in worst.items():
        assert w <= (0.5 if name.startswith("ieee") else 2.0), (name, w)


def test_fast_arithmetic_fp64_edge_points(probe):
    """Promised by the comment: fast_sqrt(0) == 0 and NaN in gives NaN out.  Everything else is pinned as the arithmetic
    gives it (and stated in the comment above fast_rsqrt, with the callers that can or cannot reach it)."""
    nan, inf = np.nan, np.inf
    tiny, big, sub = 2.0 ** -1022, np.finfo(np.float64).max, 5e-324
    x = np.array([0.0, -0.0, tiny, big, sub, 2.0 ** -1030, inf, nan, -1.0, -inf])
    rs = run(probe, "fast_rsqrt", "f64", x[:, None], 1)[:, 0]
    sq = run(probe, "fast_sqrt", "f64", x[:, None], 1)[:, 0]
    rc = run(probe, "fast_rcp", "f64", x[:, None], 1)[:, 0]
    dv = run(probe, "fast_div", "f64", np.stack([np.ones_like(x), x], 1), 1)[:, 0]
    for name, v in (("fast_rsqrt", rs), ("fast_sqrt", sq), ("fast_rcp", rc), ("fast_div(1, x)", dv)):
        print(f"[device-math] {name} at {x.tolist()}: {v.tolist()}")
    # the promises
    assert sq[0] == 0.0 and sq[1] == 0.0 and not np.signbit(sq[0])
    for v in (rs, sq, rc, dv):
        assert np.isnan(v[7])
    # normal extremes are ordinary arguments
    for v, ref in ((rs, 1 / np.sqrt(x[2:4].astype(LD))), (sq, np.sqrt(x[2:4].astype(LD))), (rc[2:3], 1 / x[2:3].astype(LD))):
        assert (M.ulp_err(v[2:4] if v.size > 1 else v, ref) <= 2).all()
    assert M.ulp_err(rc[3:4], 1 / x[3:4].astype(LD))[0] <= 2  # 1 / max: a subnormal result, still within 2 (subnormal) ulp
    # pinned as found — not promised to any caller (arguments are positive normal numbers wherever these are used):
    #   zero: the estimate is +-inf and the Newton step forms 0 * inf, so 1/sqrt(0), 1/0 and 1/(-0) are NaN, not +-inf;
    #   +inf: the estimate is 0 and the step forms inf * 0, so sqrt(inf), 1/sqrt(inf), 1/inf are NaN, not inf / 0 / 0;
    #   negative: sqrt and 1/sqrt are NaN as in IEEE, 1/x is the ordinary reciprocal;
    #   subnormal: sqrt and 1/sqrt are within 2 ulp (v_rsq_f64 takes denormals); 1/x is NaN (estimate inf, then inf * 0)
    assert np.isnan(rs[0]) and np.isnan(rs[1]) and np.isnan(rc[0]) and np.isnan(rc[1]) and np.isnan(dv[0])
    assert np.isnan(sq[6]) and np.isnan(rs[6]) and np.isnan(rc[6]) and np.isnan(rc[9])
    assert np.isnan(sq[8]) and np.isnan(rs[8]) and rc[8] == -1.0 and dv[8] == -1.0
    assert np.isnan(rc[4]) and np.isnan(rc[5]) and np.isnan(dv[4]) and np.isnan(dv[5])  # 1 / subnormal: the estimate overflows to inf
    assert (M.ulp_err(sq[4:6], np.sqrt(x[4:6].astype(LD))) <= 2).all() and (M.ulp_err(rs[4:6], 1 / np.sqrt(x[4:6].astype(LD))) <= 2).all()


def test_normalize_fp64_and_fp32(probe):
    """normalize = v * fast_rsqrt(dot(v, v)); normalize_len adds len = q * rsqrt(q).  Relative to the exact result: dot is
    three positive products and two sums (<= 3 roundings, halved by the square root), rsqrt <= 2 ulp, one product:
    <= (0.75 + 2 + 0.5) ulp < 4 * 2^-52 of the unit vector's length per component (fp32: v_rsq_f32 is 1 ulp; same count)."""
    rng = np.random.default_rng(23)
    v = rng.normal(size=(1 << 16, 3)) * 10.0 ** rng.uniform(-3, 3, size=(1 << 16, 1))
    v[:8] = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 1), (3, 4, 0), (1e-3, 0, 0), (0, 1e3, 0), (-2, 2, -1)]
    for prec, unit in (("f64", U64), ("f32", 2 * U32)):
        vv = v.astype(np.float32 if prec == "f32" else np.float64).astype(LD)
        ln = np.sqrt((vv * vv).sum(1))
        ref = vv / ln[:, None]
        got = run(probe, "normalize", prec, v, 3)
        got4 = run(probe, "normalize_len", prec, v, 4)
        err = np.abs(got.astype(LD) - ref).max(1) / unit
        errl = np.abs(got4[:, 3].astype(LD) - ln) / ln / unit
        w1 = report(f"normalize {prec} [ulp of 1]", err, lambda i: v[i].tolist())
        w2 = report(f"normalize_len {prec} length [ulp]", errl, lambda i: v[i].tolist())
        w3 = float((np.abs(got4[:, :3].astype(LD) - ref).max(1) / unit).max())
        assert w1 <= 4 and w2 <= 4 and w3 <= 4, (prec, w1, w2, w3)


# ================================================================== fp32: exhaustive
NORMAL_POS = (0x00800000, 0x7F7FFFFF)
NORMAL_NEG = (0x80800000, 0xFF7FFFFF)
X_OPS = {0: "v_rcp_f32", 1: "v_rsq_f32", 2: "v_sqrt_f32", 3: "fast_rcp", 4: "fast_rsqrt", 5: "fast_sqrt", 6: "ieee_sqrt"}
X_LOG, X_EXP = 7, 8  # v_log_f32, v_exp_f32 (base 2): the two instructions of the fp32 pow_pos


def _exhaust(L, op, first, last):
    import torch
    res = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = L.prtprobe_exhaust_f32(op, first, last - first + 1, res.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    r = res.cpu().numpy().view(np.uint64)
    return int(r[0] >> np.uint64(32)), int(r[0] & np.uint64(0xFFFFFFFF)), int(r[1]), int(r[2]), int(r[3])


def test_f32_hardware_ops_exhaustive(probe):
    """Every normal float through v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 and the fp32 overloads built on them, against the
    correctly rounded fp64 operation rounded to float, reduced on the device to (max ulp, argmax, count above 1 ulp).
    <= 1 ulp is what prt_device.h claims for them and what the slab test's pad derivation (and tests/test_slab_cpu.py's
    emulation, which uses the correctly rounded reciprocal) rests on.  Where the reference is subnormal (1/x for
    |x| > 2^126) only a correctly signed, NaN-free result is asserted."""
    for op, name in X_OPS.items():
        ranges = [NORMAL_POS] + ([NORMAL_NEG] if op in (0, 3) else [])
        for first, last in ranges:
            mx, arg, over, bad, sub = _exhaust(probe, op, first, last)
            print(f"[device-math] {name} over [{first:#010x}, {last:#010x}]: max {mx} ulp at bits {arg:#010x}, "
                  f"{over} inputs above 1 ulp, {bad} NaN / wrong sign, subnormal references off by at most {sub} * 2^-149")
            assert mx <= 1 and over == 0 and bad == 0, (name, mx, hex(arg), over, bad)


def test_f32_log_and_exp_exhaustive(probe):
    """v_log_f32 over every positive normal float and v_exp_f32 over every normal float of either sign, against the fp64
    library log2 / exp2 rounded to float (reduced on the device), and 2^20 arguments of EACH again against longdouble on the
    CPU (through the raw v_log / v_exp probes).  The ISA manual states 1 ulp for both; the maximum found here is a property
    of the instruction and is what the BSDF model charges the fp32 pow_pos (device_math_model.K_LOG_F32 / K_EXP_F32 = that
    maximum plus the rounded reference's own half ulp).  Where the reference is not a normal float the result must be the
    reference itself for log2(1) = 0 and for the overflow of 2^x to inf; v_exp_f32 flushes a subnormal result to 0
    (x < -126): printed, like v_rcp_f32's."""
    found = {}
    for op, name, ranges in ((X_LOG, "v_log_f32", [NORMAL_POS]), (X_EXP, "v_exp_f32", [NORMAL_POS, NORMAL_NEG])):
        for first, last in ranges:
            mx, arg, over, bad, sub = _exhaust(probe, op, first, last)
            print(f"[device-math] {name} over [{first:#010x}, {last:#010x}]: max {mx} ulp at bits {arg:#010x}, "
                  f"{over} inputs above 1 ulp, {bad} NaN / wrong sign, subnormal references off by at most {sub} * 2^-149")
            found[name] = max(found.get(name, 0), mx)
            assert bad == 0, (name, bad)
            if (first, last) == NORMAL_POS:  # the only references outside the normal range: log2(1) = 0, 2^x = inf from x = 128
                assert sub == 0, (name, sub)
    assert found["v_log_f32"] + 0.5 <= M.K_LOG_F32 and found["v_exp_f32"] + 0.5 <= M.K_EXP_F32, found
    rng = np.random.default_rng(33)
    x = rng.uniform(-126, 127, 1 << 20).astype(np.float32)
    x[: 1 << 18] = rng.uniform(-2.0 ** -8, 2.0 ** -8, 1 << 18).astype(np.float32)  # results around 1
    got = run(probe, "v_exp", "f32", x[:, None], 1)[:, 0]
    w = report("v_exp_f32 vs longdouble [ulp]", M.ulp_err(got, np.exp2(x.astype(LD)), np.float32).astype(np.float64), lambda i: float(x[i]).hex())
    assert w <= M.K_EXP_F32, w
    y = rng.integers(NORMAL_POS[0], NORMAL_POS[1] + 1, size=1 << 20).astype(np.uint32).view(np.float32).copy()
    y[: 1 << 18] = (1 + rng.uniform(-2.0 ** -8, 2.0 ** -8, 1 << 18)).astype(np.float32)  # around 1, where log2 passes through 0
    y[(1 << 18): (1 << 19)] = rng.integers(1, 1 << 24, size=1 << 18) / np.float32(2.0 ** 24)  # the fp32 unit's RNG lattice: pow_pos' arguments
    got = run(probe, "v_log", "f32", y[:, None], 1)[:, 0]
    ref = np.log2(y.astype(LD))
    err = M.ulp_err(got, ref, np.float32).astype(np.float64)
    err[ref == 0] = np.where(got[ref == 0] == 0, 0.0, np.inf)
    w = report("v_log_f32 vs longdouble [ulp]", err, lambda i: float(y[i]).hex())
    assert w <= M.K_LOG_F32, w


def test_f32_hardware_ops_subset_rechecked_on_the_cpu_and_subnormal_inputs(probe):
    rng = np.random.default_rng(24)
    bits = rng.integers(NORMAL_POS[0], NORMAL_POS[1] + 1, size=1 << 20).astype(np.uint32)
    x = bits.view(np.float32)
    x64 = x.astype(np.float64)

    def ulps(got, ref):
        o = lambda f: np.where(f.view(np.int32) < 0, np.int64(-2 ** 31) - f.view(np.int32).astype(np.int64), f.view(np.int32).astype(np.int64))
        return np.abs(o(got) - o(ref))

    with np.errstate(all="ignore"):
        refs = {"fast_rcp": (1.0 / x64).astype(np.float32), "fast_rsqrt": (1.0 / np.sqrt(x64)).astype(np.float32),
                "fast_sqrt": np.sqrt(x64).astype(np.float32), "ieee_sqrt": np.sqrt(x64).astype(np.float32)}
    for name, ref in refs.items():
        got = np.ascontiguousarray(run(probe, name, "f32", x[:, None], 1)[:, 0])
        normal = np.abs(ref) >= np.finfo(np.float32).tiny
        u = ulps(got, ref)
        w = report(f"{name} fp32 on 2^20 floats, CPU reference [ulp]", np.where(normal, u, 0).astype(np.float64), lambda i: float(x[i]).hex())
        assert w <= 1, (name, w)
    # fast_div / ieee_div (fp32) = a * v_rcp_f32(b): the reciprocal's 1 ulp, half an ulp of the product and half an ulp of the
    # rounded reference: at most 2 float steps from the correctly rounded quotient — wherever 1/b is a normal float, i.e.
    # |b| <= 2^126.  Beyond that the reciprocal is subnormal, which v_rcp_f32 flushes to zero (the exhaustive test prints
    # it): the quotient is then 0 although a/b may be a normal number.  Pinned here and stated in prt_device.h; no caller
    # divides by anything near 2^126 (denominators are dot products of unit vectors, pdfs, lengths).
    a = (1.0 + rng.random(x.size)).astype(np.float32)
    for name in ("fast_div", "ieee_div"):
        got = np.ascontiguousarray(run(probe, name, "f32", np.stack([a, x], 1), 1)[:, 0])
        with np.errstate(all="ignore"):
            ref = (a.astype(np.float64) / x64).astype(np.float32)
        dom = (np.abs(ref) >= np.finfo(np.float32).tiny) & (np.abs(x) <= np.float32(2.0 ** 126))
        w = report(f"{name} fp32 [ulp]", np.where(dom, ulps(got, ref), 0).astype(np.float64), lambda i: (float(a[i]).hex(), float(x[i]).hex()))
        assert w <= 2, (name, w)
        flushed = np.abs(x) > np.float32(2.0 ** 126)
        assert flushed.any() and ((got[flushed] == 0) | (ulps(got, ref)[flushed] <= 2)).all() and not np.isnan(got).any(), name
    # subnormal inputs: a correctly signed finite-or-infinite result, never NaN
    sb = np.concatenate([np.arange(1, 1 << 12), rng.integers(1, 1 << 23, size=1 << 12), [(1 << 23) - 1]]).astype(np.uint32)
    for name, signs in (("fast_rcp", (0, 0x80000000)), ("fast_rsqrt", (0,)), ("fast_sqrt", (0,)), ("ieee_sqrt", (0,))):
        for sgn in signs:
            xs = (sb | np.uint32(sgn)).view(np.float32)
            got = run(probe, name, "f32", xs[:, None], 1)[:, 0]
            assert not np.isnan(got).any() and (np.signbit(got) == np.signbit(xs)).all(), (name, sgn)


# ================================================================== FMA helpers
def test_fma_helpers_are_single_fused_operations(probe):
    """fma_ks / fma_sk / mul_ks are inline v_fma_f64 / v_mul_f64 with the literal in a scalar operand: bitwise the correctly
    rounded a * b + k (exact rational arithmetic), on operands most of which an unfused multiply-then-add rounds differently."""
    rng = np.random.default_rng(25)
    n = 100000
    a = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    b_rand = rng.uniform(-2.0, 2.0, n)
    got_any_unfused = 0
    for op in ("fma_ks", "fma_sk"):
        worst = 0
        for j, k in enumerate(M.FMA_K):
            sl = slice(j * (n // 5), (j + 1) * (n // 5))  # each literal gets its own fifth of the operands
            aa = a[sl]
            if op == "fma_ks":  # a * b + k with the product cancelling most of k: the low product bits decide the result
                bb = np.where(rng.random(aa.size) < 0.5, -k / aa * (1 + rng.uniform(-1e-6, 1e-6, aa.size)), b_rand[sl])
                inp, ref = np.stack([aa, bb], 1), M.fma_exact_many(aa, bb, np.float64(k))
                unf = aa * bb + k
            else:                # a * k + c
                cc = np.where(rng.random(aa.size) < 0.5, -k * aa * (1 + rng.uniform(-1e-6, 1e-6, aa.size)), b_rand[sl])
                inp, ref = np.stack([aa, cc], 1), M.fma_exact_many(aa, np.full(aa.size, k), cc)
                unf = aa * k + cc
            got = run(probe, op, "f64", inp, 5)[:, j]
            got_any_unfused += int((unf != ref).sum())
            bad = got.view(np.uint64) != ref.view(np.uint64)
            worst += int(bad.sum())
            assert not bad.any(), (op, k, inp[bad][0].tolist(), got[bad][0], ref[bad][0])
        print(f"[device-math] {op}: {worst} of {n} results differ from the correctly rounded value")
    assert got_any_unfused >= n // 4, got_any_unfused  # the operands do tell a fused from an unfused evaluation
    got = run(probe, "mul_ks", "f64", a[:, None], 5)
    for j, k in enumerate(M.FMA_K):
        assert np.array_equal(got[:, j].view(np.uint64), (a * k).view(np.uint64)), k  # one IEEE product: numpy's
    # the fp32 overload (__builtin_fmaf)
    m = 1000
    a32, k32 = a[:m].astype(np.float32), [np.float32(k) for k in M.FMA_K]
    for j, k in enumerate(k32):
        b32 = (-np.float64(k) / a32.astype(np.float64) * (1 + rng.uniform(-1e-4, 1e-4, m))).astype(np.float32)
        got = run(probe, "fma_ks", "f32", np.stack([a32, b32], 1), 5)[:, j]
        ref = np.array([M.fma_exact32(x, y, k) for x, y in zip(a32, b32)], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), k


# ================================================================== sin / cos
def test_sincos_quarter(probe):
    """|x| <= pi/4.  fp64: the fdlibm kernel polynomials, < 1 ulp of the result (the comment's claim).
    fp32 (Taylor to x^9 / x^8, u = 2^-24 the rounding unit, z = x^2 <= 0.617):
      cos = 1 + z (a1 + z (a2 + ...)): truncation x^10/10! <= 0.41 u; z's rounding moves the result by <= 0.31 u; the
        roundings of a1 + z(..) (<= 0.53 u, scaled by z: 0.33 u), of the product with z (0.29 u), of the last sum (1 u), the
        inner steps (< 0.05 u): < 2.4 u absolute — asserted as 3 u;
      sin = x + (x z) S, |S| <= 1/6: everything but the last sum is scaled by z |S| <= 0.1 (three roundings of x z S plus
        those inside S: < 0.4 u |x|), the last sum rounds by <= u |x|, truncation x^11/11! <= 0.03 u: < 1.5 u |x| — asserted
        as 3 u |x|."""
    pi4 = np.float64(0.78539816339744830961)
    x = np.concatenate([np.linspace(-pi4, pi4, 1 << 20), [pi4, -pi4, 0.0, 5e-324, -5e-324, 1e-300, -1e-300, 2.0 ** -27, 2.0 ** -26,
                                                             np.nextafter(pi4, 0), 1e-8, -1e-8]])
    got = run(probe, "sincos_quarter", "f64", x[:, None], 2)
    xl = x.astype(LD)
    es, ec = M.ulp_err(got[:, 0], np.sin(xl)), M.ulp_err(got[:, 1], np.cos(xl))
    es[x == 0] = 0 if got[x == 0, 0][0] == 0 else np.inf
    ws = report("sincos_quarter fp64 sin [ulp]", es, lambda i: float(x[i]).hex())
    wc = report("sincos_quarter fp64 cos [ulp]", ec, lambda i: float(x[i]).hex())
    assert ws < 1 and wc < 1, (ws, wc)
    tiny = np.abs(x) <= 1e-300
    assert np.array_equal(got[tiny, 0], x[tiny]) and (got[tiny, 1] == 1).all()
    x32 = x[np.abs(x) >= 1e-30].astype(np.float32)  # (the relative sine error needs x != 0; 0 and +-tiny are asserted exactly below)
    x32 = x32[np.abs(x32) <= np.float32(pi4)]
    got = run(probe, "sincos_quarter", "f32", x32[:, None], 2)
    xl = x32.astype(LD)
    es = np.abs(got[:, 0].astype(LD) - np.sin(xl)) / (U32 * np.abs(xl))
    ec = np.abs(got[:, 1].astype(LD) - np.cos(xl)) / U32
    ws = report("sincos_quarter fp32 sin [2^-24 |x|]", es, lambda i: float(x32[i]).hex())
    wc = report("sincos_quarter fp32 cos [2^-24]", ec, lambda i: float(x32[i]).hex())
    assert ws <= 3 and wc <= 3, (ws, wc)
    z = run(probe, "sincos_quarter", "f32", np.array([[0.0], [-0.0], [1e-45], [-1e-45], [1e-38]]), 2)  # 0 and +-tiny, left out above
    assert np.array_equal(z[:, 0], np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38], dtype=np.float32)) and (z[:, 1] == 1).all(), z.tolist()


def _turn_lattice_fp64():
    rng = np.random.default_rng(26)
    near = np.arange(-(1 << 12), (1 << 12) + 1)
    ks = [m * (1 << 28) + near for m in range(9)]  # even multiples: the quarter turns; odd ones: the floor(4u + 1/2) switches
    k = np.concatenate(ks + [rng.integers(0, 1 << 31, size=1 << 20)])
    return np.unique(k[(k >= 0) & (k < (1 << 31))])


def test_sincos_turns_fp64(probe):
    """sin / cos of 2 pi u on the RNG lattice: r = u - k/4 is exact, 2 pi r rounds once (|angle| <= pi/4: <= 2^-53 absolute,
    moved into the result with slope <= 1) and the polynomial is < 1 ulp of a result <= 1: absolute error <= 2^-52."""
    k = _turn_lattice_fp64()
    u = k / 2.0 ** 31
    got = run(probe, "sincos_turns", "f64", u[:, None], 2)
    two_pi = LD(2) * LD("3.14159265358979323846264338327950288")
    th = two_pi * (u.astype(LD) - np.round(u.astype(LD)))  # reduced by whole turns (exact): the reference's own argument error is < 2^-64
    es = np.abs(got[:, 0].astype(LD) - np.sin(th)) / U64
    ec = np.abs(got[:, 1].astype(LD) - np.cos(th)) / U64
    ws = report("sincos_turns fp64 sin [2^-52]", es, lambda i: f"k = {int(k[i])}")
    wc = report("sincos_turns fp64 cos [2^-52]", ec, lambda i: f"k = {int(k[i])}")
    assert ws <= 1 and wc <= 1, (ws, wc)
    q = run(probe, "sincos_turns", "f64", np.array([[0.0], [0.25], [0.5], [0.75]]), 2)
    assert np.array_equal(q, np.array([[0.0, 1.0], [1.0, 0.0], [0.0, -1.0], [-1.0, 0.0]])), q.tolist()
    # sincos_any (fp64): the library sincos of the rounded theta = 2 pi u, documented to 2 ulp
    theta = (2 * np.float64(3.14159265358979323846)) * u
    got = run(probe, "sincos_any", "f64", u[:, None], 2)
    es, ec = M.ulp_err(got[:, 0], np.sin(theta.astype(LD))), M.ulp_err(got[:, 1], np.cos(theta.astype(LD)))
    es[theta == 0] = 0
    ws = report("sincos_any fp64 sin [ulp]", es, lambda i: f"k = {int(k[i])}")
    wc = report("sincos_any fp64 cos [ulp]", ec, lambda i: f"k = {int(k[i])}")
    assert ws <= 2 and wc <= 2, (ws, wc)


def test_sincos_turns_and_any_fp32_exhaustive_over_the_lattice(probe):
    """Every u = k / 2^24 of the fp32 unit's RNG against float64.
    sincos_turns: 2 pi r in fp32 — pi rounded (2^-25 relative) and one product (2^-24), |angle| <= pi/4: <= 1.2 u absolute —
      plus sincos_quarter's 3 u (above): <= 5 u absolute, u = 2^-24.
    sincos_any: v_sin_f32 / v_cos_f32 take u itself (exact).  16 u = 2^-20 absolute is a BUDGET, not an accuracy claim: no
      accuracy of the two instructions is documented that the code could cite, so prt_device.h states what the fp32 mode
      needs of them (the size of the 16-ulp perturbation it is validated against) and this test holds them to
      it."""
    k = np.arange(1 << 24)
    u = (k / 2.0 ** 24)
    ref_s, ref_c = np.sin(2 * np.pi * (u - np.round(u))), np.cos(2 * np.pi * (u - np.round(u)))
    for name, bound in (("sincos_turns", 5.0), ("sincos_any", 16.0)):
        got = run(probe, name, "f32", u[:, None], 2)
        es = np.abs(got[:, 0].astype(np.float64) - ref_s) / U32
        ec = np.abs(got[:, 1].astype(np.float64) - ref_c) / U32
        ws = report(f"{name} fp32 sin [2^-24]", es, lambda i: f"k = {int(k[i])}")
        wc = report(f"{name} fp32 cos [2^-24]", ec, lambda i: f"k = {int(k[i])}")
        assert ws <= bound and wc <= bound, (name, ws, wc)
        if name == "sincos_turns":
            q = got[[0, 1 << 22, 1 << 23, 3 << 22]]
            assert np.array_equal(q, np.array([[0, 1], [1, 0], [0, -1], [-1, 0]], dtype=np.float32)), q.tolist()


# ================================================================== pow_pos
NS_VALUES = M.ns_values_in_sources()  # every Ns written in scenes.py and tests/, read from the sources (tests/test_device_math_cpu.py checks the reader)
POW_Y = sorted(set(NS_VALUES + [1.0 / (ns + 1.0) for ns in NS_VALUES] + [0.0, 1.0, 5.0, 50.0, 1000.0]))


def _pow_x():
    rng = np.random.default_rng(27)
    lat = M.lattice_ends()  # both ends of the lattice; the upper one is dense near 1
    r2 = np.float64(0.70710678118654752440)
    sw = [np.ldexp(v, e) for e in range(-30, 1) for v in (np.nextafter(r2, 0), r2, np.nextafter(r2, 1), np.nextafter(np.nextafter(r2, 0), 0))]
    cosines = np.cos(rng.uniform(0, np.pi / 2, 1 << 14))
    cosines = cosines[cosines > 0]
    return np.concatenate([lat, sw, cosines, [np.nextafter(1.0, 0.0), 0.5, 0.25, 2.0 ** -31, 1.0 - 2.0 ** -31],
                           rng.integers(1, 1 << 31, size=1 << 14) / 2.0 ** 31])


def test_pow_pos_fp64(probe):
    """x^y = exp(y log x) for the Phong lobe: within 1e-14 relative wherever |y ln x| <= 50 (the comment's domain and figure)."""
    x = _pow_x()
    xx, yy = np.meshgrid(x, np.array(POW_Y), indexing="ij")
    xx, yy = xx.ravel(), yy.ravel()
    got = run(probe, "pow_pos", "f64", np.stack([xx, yy], 1), 1)[:, 0]
    t = yy.astype(LD) * np.log(xx.astype(LD))
    ref = np.exp(t)
    dom = np.abs(t) <= 50
    with np.errstate(all="ignore"):
        rel = np.where(dom, np.abs(got.astype(LD) - ref) / ref, 0).astype(np.float64)
    w = report("pow_pos fp64 relative error, |y ln x| <= 50", rel, lambda i: f"x = {float(xx[i]).hex()}, y = {yy[i]}, y ln x = {float(t[i]):.3f}")
    for lim in (1, 10, 25, 50):
        s = np.abs(t) <= lim
        print(f"[device-math] pow_pos fp64: max relative error {rel[s].max():.4g} over |y ln x| <= {lim}")
    assert np.isfinite(got).all() and (got >= 0).all()
    assert w <= 1e-14, w


def test_pow_pos_special_values(probe):
    """pow_pos(1, y) == 1 exactly (ca = fmin(pow, 1) follows it), pow_pos(0, y) == 0, a deep underflow is 0 or tiny and never
    NaN / Inf.  Out of domain the two precisions DIFFER and the comment says so: fp64 returns 0 for x < 0 and for NaN
    (`x > 0 ? e : 0`), fp32 returns NaN (v_log_f32 of a negative number).  No caller can see the difference: mat_eval's
    `ca = fmax(0, dot)` with `if (ca <= 0) return` keeps negatives and NaN out, mat_scatter's x is a lattice draw in [0, 1)
    and its result is used only under `u1 > 0`."""
    y = np.array(POW_Y)
    for prec in ("f64", "f32"):
        one = run(probe, "pow_pos", prec, np.stack([np.ones_like(y), y], 1), 1)[:, 0]
        zero = run(probe, "pow_pos", prec, np.stack([np.zeros_like(y), y], 1), 1)[:, 0]
        assert (one == 1).all(), (prec, one.tolist())
        pos = y > 0
        assert (zero[pos] == 0).all(), (prec, zero.tolist())
        xs = np.array([2.0 ** -31, 1e-3, 0.5, 2.0 ** -31, 0.01])
        ys = np.array([1000.0, 2000.0, 2000.0, 2000.0, 900.0])  # y ln x < -1000 for all but the last two
        deep = run(probe, "pow_pos", prec, np.stack([xs, ys], 1), 1)[:, 0]
        print(f"[device-math] pow_pos {prec} deep underflow: {deep.tolist()}; pow_pos(0, 0) = {zero[~pos].tolist()}")
        assert np.isfinite(deep).all() and (deep >= 0).all() and (deep[:2] <= 1e-300).all() and deep[3] <= 1e-300, (prec, deep.tolist())
        # y = 0 at x = 0, as the header's comment states it: 0 in fp64 (`x > 0 ? e : 0`), NaN in fp32 (0 * -inf)
        assert (~pos).sum() == 1
        assert (zero[~pos] == 0).all() if prec == "f64" else np.isnan(zero[~pos]).all(), (prec, zero[~pos].tolist())
    bad = np.array([[-0.5, 2.0], [-1.0, 0.5], [np.nan, 2.0], [-np.inf, 2.0]])
    g64 = run(probe, "pow_pos", "f64", bad, 1)[:, 0]
    g32 = run(probe, "pow_pos", "f32", bad, 1)[:, 0]
    assert (g64 == 0).all() and not np.signbit(g64).any(), g64.tolist()
    assert np.isnan(g32).all(), g32.tolist()
    # fp32 accuracy: a figure only here.  (test_f32_log_and_exp_exhaustive measures v_log_f32 / v_exp_f32 on their own, and
    # the BSDF model charges pow_pos with those maxima where the Phong lobe uses it.)
    x = _pow_x().astype(np.float32)
    xx, yy = np.meshgrid(x[x > 0], np.array(POW_Y, dtype=np.float32), indexing="ij")
    xx, yy = xx.ravel(), yy.ravel()
    got = run(probe, "pow_pos", "f32", np.stack([xx, yy], 1), 1)[:, 0]
    t = yy.astype(LD) * np.log(xx.astype(LD))
    with np.errstate(all="ignore"):
        rel = np.where(np.abs(t) <= 50, np.abs(got.astype(LD) - np.exp(t)) / np.exp(t), 0).astype(np.float64)
    report("pow_pos fp32 relative error, |y ln x| <= 50 (not asserted)", rel, lambda i: f"x = {float(xx[i]).hex()}, y = {yy[i]}")
    assert not np.isnan(got).any() and (got >= 0).all()


# ================================================================== Fresnel
# every (eta, k) channel of a CookTorrance material written in scenes.py and tests/ (read from the sources), then dielectrics
# with eta < 1 (total internal reflection), eta = 1 with and without k, a strong conductor and a k = 0 "metal"
ETA_K = M.eta_k_in_sources() + [(1 / 1.5, 0.0), (0.5, 0.0), (0.9, 0.0), (1.0, 0.0), (1.0, 0.5), (2.5, 4.0), (0.1, 0.0)]
COS_I = [0.0, 2.0 ** -31, 1e-8, 0.5, float(np.nextafter(1.0, 0.0)), 1.0]


def test_csqrt_and_fr_complex_against_mpmath(probe):
    import mpmath
    rows = [(c, e, k) for c in COS_I for e, k in ETA_K]
    for prec, tol in (("f64", 1e-13),):
        got = run(probe, "fr_complex", prec, np.array(rows), 1)[:, 0]
        worst, where = 0.0, None
        for (c, e, k), g in zip(rows, got):
            ref = M.fr_complex_mp(c, e, k)
            if ref is None:
                continue
            assert np.isfinite(g) and -tol <= g <= 1 + tol, (c, e, k, g)
            if ref >= 1e-12:
                rel = float(abs(mpmath.mpf(float(g)) - ref) / ref)
                if rel > worst:
                    worst, where = rel, (c, e, k)
        print(f"[device-math] fr_complex {prec}: max relative error {worst:.4g} at (cos, eta, k) = {where}")
        assert worst <= tol, (worst, where)
    # the complex square root on the arguments fr_complex forms, and on negative reals (total internal reflection)
    zs = []
    for c, e, k in rows:
        z = 1 - (1 - mpmath.mpf(c) ** 2) / mpmath.mpc(e, k) ** 2
        zs.append((float(z.real), float(z.imag)))
    zs += [(-1.0, 0.0), (-0.25, 0.0), (4.0, 0.0), (0.0, 2.0), (0.0, -2.0), (-3.0, 4.0), (-3.0, -4.0), (1e-300, 0.0), (0.0, 0.0)]
    got = run(probe, "csqrt", "f64", np.array(zs), 2)
    worst, where = 0.0, None
    for (re, im), g in zip(zs, got):
        ref = M.csqrt_mp(re, im)
        if im == 0 and re < 0 and np.signbit(im):
            continue
        for gv, rv in ((g[0], ref.real), (g[1], ref.imag)):
            if abs(rv) >= 1e-12:
                rel = float(abs(mpmath.mpf(float(gv)) - rv) / abs(rv))
                if rel > worst:
                    worst, where = rel, (re, im)
            else:
                assert abs(gv) <= 1e-12, (re, im, g.tolist())
    print(f"[device-math] csqrt_ fp64: max relative error {worst:.4g} at z = {where}")
    assert worst <= 1e-13, (worst, where)


def test_fr_complex_zero_over_zero_agrees_with_the_oracle(probe):
    """eta = 1, k = 0, cos = 0: both amplitude ratios are 0/0.  The device and the oracle's fp64 twin (the same formula in
    std::complex-free C++) must agree on NaN or not-NaN — a difference would be a parity break no frame test can provoke."""
    import oracle
    from pooraytracer_amd import _abi, scenes
    from pooraytracer_amd.scenes import Material
    data = scenes.tiny_scene()
    mats = list(data.materials)
    mats.append(Material("VacuumCT", _abi.MAT_COOKTORRANCE, kd=(0.5, 0.5, 0.5), eta=(1.0, 1.0, 1.5), k=(0.0, 0.0, 0.0), alpha_x=0.5, alpha_y=0.5))
    data.materials = mats
    orc = oracle.Oracle(data)
    w = np.array([[1.0, 0.0, 0.0]])   # cos_i = |w . wm| = 0
    wm = np.array([[0.0, 0.0, 1.0]])
    terms = orc.cooktorrance_terms(len(mats) - 1, w, wm)
    fres = np.asarray(terms["F"]).reshape(-1, 3)[0]
    got = run(probe, "fr_complex", "f64", np.array([[0.0, 1.0, 0.0], [0.0, 1.5, 0.0]]), 1)[:, 0]
    print(f"[device-math] fr_complex(0, 1 + 0i): device {got[0]}, oracle {fres[0]}; (0, 1.5): device {got[1]}, oracle {fres[2]}")
    assert np.isnan(got[0]) == np.isnan(fres[0])
    assert abs(got[1] - fres[2]) <= 1e-13


# ================================================================== visible-normal sampler
WM_ALPHAS = [(0.5, 0.5), (0.2, 0.6), (0.3, 0.3), (1e-3, 1e-3), (1.0, 1.0)]  # tests/test_materials.py's, plus 1e-3 and 1


def _wm_bound(info):
    """First-order error bound against the exact result of the sampler AS THE REFERENCE WRITES IT (h = sqrt(1 - p.x^2),
    pz = sqrt(1 - |p|^2)), from the condition number of each step.  The device forms h and pz without those cancellations
    (prt_device.h), so for it the d_h and d_pz lines are far too generous: measured error / bound <= 0.015.  This bound only
    fences gross errors; what holds the cancellation-free forms in place is the absolute 1e-11 assertion of
    test_ct_sample_wm_is_within_a_hundredth_of_the_parity_tolerance.  Step by step
    (e = 2^-52; every constant is an upper bound, and each later step carries the earlier ones):
      wh = normalize(..)                 d_wh <= 4 e          (test_normalize_fp64_and_fp32)
      T1 = normalize(z x wh)             d_T1 <= sqrt2 d_wh / sin(theta_h) + 4 e   — 1/sin = 224 at the wh.z = 0.99999 switch;
                                         0 for the fixed basis
      T2 = wh x T1                       d_T2 <= d_wh + d_T1 + 2 e
      p = sqrt(u.x) (cos, sin)(2 pi u.y) d_p <= 6 e           (theta rounds once, <= 4 e; library sincos 2 ulp; sqrt exact)
      h = sqrt(1 - p.x^2)                d_h <= (2 d_p + e) / (2 h) + e
      p.y' = (1 - lx) h + lx p.y         d_py <= d_h + d_p + d_wh + 3 e
      pz = sqrt(q), q = 1 - |p|^2        d_q <= 2 (d_p + d_py) + 3 e;  d_pz <= min(d_q / (2 pz), sqrt(d_q)) + e
      nh = p.x T1 + p.y' T2 + pz wh      d_nh <= |p.x| d_T1 + |p.y'| d_T2 + d_p + d_py + d_pz + pz d_wh + 5 e
      wm = normalize(ax nh.x, ay nh.y, max(1e-6, nh.z))   d_wm <= sqrt3 max(ax, ay, 1) d_nh / |v| + 4 e — the stretch
                                         back divides by |v|, which is as small as alpha for a grazing nh."""
    e = U64
    d_wh = 4 * e
    d_t1 = (np.sqrt(2) * d_wh / max(info["sin_h"], 1e-300) + 4 * e) if info["basis"] else 0.0
    d_t2 = d_wh + d_t1 + 2 * e
    d_p = 6 * e
    d_h = (2 * d_p + e) / (2 * max(info["h"], 1e-300)) + e
    d_py = d_h + d_p + d_wh + 3 * e
    d_q = 2 * (d_p + d_py) + 3 * e
    d_pz = min(d_q / (2 * info["pz"]) if info["pz"] > 0 else np.inf, np.sqrt(d_q)) + e
    d_nh = abs(info["px"]) * d_t1 + abs(info["py"]) * d_t2 + d_p + d_py + d_pz + info["pz"] * d_wh + 5 * e
    return np.sqrt(3) * info["amax"] * d_nh / info["vlen"] + 4 * e


def _wm_inputs():
    rng = np.random.default_rng(31)
    top = (1 << 31) - 1
    us = [(a / 2.0 ** 31, b / 2.0 ** 31) for a in (0, top, 1 << 30, 1) for b in (0, top, 1 << 29, 1 << 30)]  # rims, centre
    us += [tuple(v) for v in (rng.integers(0, 1 << 31, size=(12, 2)) / 2.0 ** 31).tolist()]
    rows, straddle = [], []
    for ax, ay in WM_ALPHAS:
        ws = [(0.0, 0.0, 1.0)]
        for z in (1e-6, 1e-3, 0.5, -0.5):
            s = np.sqrt(1 - z * z)
            ws.append((s * np.cos(0.7), s * np.sin(0.7), z))
        for target in (0.99999 - 1e-6, 0.99999 + 1e-6):  # stretched wh.z on either side of the switch
            t = np.sqrt(1 / target ** 2 - 1)
            ws.append((t * np.cos(2.1) / ax, t * np.sin(2.1) / ay, 1.0))
        # one pair of ADJACENT doubles t whose exact wh.z straddles 0.99999 (wh.z falls as t grows)
        whz = lambda t: M.ct_sample_wm_mp(ax, ay, (t / ax, 0.0, 1.0), (0.5, 0.5))[1]["whz_mp"]
        lo, hi = 0.004, 0.005
        while np.nextafter(lo, hi) < hi:
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if whz(mid) >= M.WM_SWITCH else (lo, mid)
        for t in (np.nextafter(lo, 0), lo, hi, np.nextafter(hi, 1)):
            ws.append((t / ax, 0.0, 1.0))
            straddle.append(len(rows) + (len(ws) - 1) * len(us))
        for w in ws:
            rows += [(ax, ay) + tuple(w) + u for u in us]
    marks = np.zeros(len(rows), dtype=bool)
    for s0 in straddle:
        marks[s0:s0 + len(us)] = True
    return np.array(rows), marks


@pytest.fixture(scope="module")
def wm_results(probe):
    """(rows, device results, error, derived bound) per input; an input within an ulp of the wh.z < 0.99999 switch may take
    either basis and is compared with the nearer of the two branch references."""
    rows, near_switch = _wm_inputs()
    got = run(probe, "ct_sample_wm", "f64", rows, 3)
    errs, bounds = np.zeros(len(rows)), np.zeros(len(rows))
    for i, r in enumerate(rows):
        best = np.inf
        for force in ([True, False] if near_switch[i] else [None]):
            ref, info = M.ct_sample_wm_mp(r[0], r[1], r[2:5], r[5:7], force_basis=force)
            err = max(abs(float(M.mpf(float(g)) - c)) for g, c in zip(got[i], ref))
            b = _wm_bound(info)
            if err / b < best:
                best, errs[i], bounds[i] = err / b, err, b
    return rows, got, errs, bounds


def test_ct_sample_wm_is_a_unit_vector_within_its_derived_bound(wm_results):
    """The visible-normal sampler (Material.h:412-435) on chosen materials, directions and draws against its restatement in
    mpmath: unit length to 4 ulp, finite, z > 0, and within _wm_bound — the first-order bound derived above, step by step,
    from each step's condition number.  No input is excluded."""
    rows, got, errs, bounds = wm_results
    assert np.isfinite(got).all() and (got[:, 2] > 0).all()
    nrm = np.abs(np.sqrt((got.astype(LD) ** 2).sum(1)) - 1).astype(np.float64) / U64
    wn = report("ct_sample_wm |wm| - 1 [ulp]", nrm, lambda i: rows[i].tolist())
    assert wn <= 4, wn
    w = report("ct_sample_wm error / derived bound", errs / bounds, lambda j: f"{rows[j].tolist()} error {errs[j]:.4g} bound {bounds[j]:.4g}")
    assert w <= 1, w


def test_ct_sample_wm_is_within_a_hundredth_of_the_parity_tolerance(wm_results):
    """... and the error itself may not exceed 1e-11, one hundredth of the parity tolerance, for ANY input.

    The reference's expressions miss this: evaluated as written (h = sqrt(1 - p.x^2), pz = sqrt(1 - p.x^2 - p.y'^2)) they
    were off by 9.0e-10 at alpha = (1e-3, 1e-3), w = (0.765, 0.644, 1e-3), u = (1 - 2^-31, 1/2) and by 1.25e-11 at
    alpha = (0.2, 0.6) — on the disk's rim 1 - p.x^2 ~ 2^-31 squares sqrt(u.x) back and keeps only 2^-22 relative, and the
    stretch back to the ellipsoid divides the result by |v| ~ alpha.  ct_sample_wm now forms both from 1 - u.x and sums of
    non-negative terms (see its comment); this test is what holds that in place."""
    rows, got, errs, bounds = wm_results
    over = errs > 1e-11
    print(f"[device-math] ct_sample_wm: {int(over.sum())} of {len(rows)} inputs are off by more than 1e-11; alphas involved: "
          f"{sorted(set(map(tuple, rows[over][:, :2].tolist())))}; {int((bounds > 1e-11).sum())} derived bounds exceed 1e-11")
    for ax, ay in WM_ALPHAS:
        sel = (rows[:, 0] == ax) & (rows[:, 1] == ay)
        print(f"[device-math] ct_sample_wm alpha = ({ax}, {ay}): max error {errs[sel].max():.4g}, max derived bound {bounds[sel].max():.4g}")
    w = report("ct_sample_wm error [abs]", errs, lambda j: rows[j].tolist())
    assert w <= 1e-11, w


def test_ct_sample_wm_fp32_is_a_finite_unit_vector_above_the_surface(probe):
    """The fp32 twin on the same materials and directions, its draws moved onto the fp32 unit's lattice (k / 2^24): finite,
    z > 0, unit length to normalize's fp32 bound (4 * 2^-23, test_normalize_fp64_and_fp32).  No accuracy is asserted against
    the restatement: v_sin_f32 / v_cos_f32 enter with a budget only (sincos_any), so no bound could be derived."""
    rows, near_switch = _wm_inputs()
    rows = rows.copy()
    rows[:, 5:7] = np.floor(rows[:, 5:7] * 2.0 ** 24) / 2.0 ** 24
    got = run(probe, "ct_sample_wm", "f32", rows, 3)
    assert np.isfinite(got).all() and (got[:, 2] > 0).all()
    nrm = np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(1)) - 1) / (2 * U32)
    wn = report("ct_sample_wm fp32 |wm| - 1 [2^-23]", nrm, lambda i: rows[i].tolist())
    assert wn <= 4, wn
    sub = np.nonzero(~near_switch)[0][::7]  # (within an fp64 ulp of the switch fp32 may rightly take the other basis)
    ref = np.array([[float(c) for c in M.ct_sample_wm_mp(*np.float32(r[:2]), np.float32(r[2:5]), r[5:7])[0]] for r in rows[sub]])
    report("ct_sample_wm fp32 error vs the restatement (not asserted)", np.abs(got[sub] - ref).max(1), lambda i: rows[sub][i].tolist())


# ================================================================== concentric map, cosine hemisphere
def _disk_pairs(bits):
    """Draw pairs (k1, k2) of a `bits`-bit lattice: centre, rims, axes, diagonals, their neighbours within 2^8 steps, random."""
    rng = np.random.default_rng(28)
    top, half = (1 << bits) - 1, 1 << (bits - 1)
    n = 1 << 9
    t = rng.integers(0, top + 1, size=n)
    base = [np.stack([np.full(n, 0), t], 1), np.stack([np.full(n, top), t], 1), np.stack([t, np.full(n, 0)], 1),
            np.stack([t, np.full(n, top)], 1), np.stack([np.full(n, half), t], 1), np.stack([t, np.full(n, half)], 1),
            np.stack([t, t], 1), np.stack([t, (1 << bits) - t], 1), np.array([[half, half], [0, 0], [top, top], [0, top], [top, 0]])]
    base = np.concatenate(base)
    near = []
    for dx, dy in rng.integers(-(1 << 8), (1 << 8) + 1, size=(16, 2)).tolist() + [[1, 0], [0, 1], [-1, 0], [0, -1], [1, 1], [-1, 1]]:
        near.append(base + np.array([dx, dy]))
    k = np.concatenate([base] + near + [rng.integers(0, top + 1, size=(1 << 20, 2))])
    return np.clip(k, 0, top).astype(np.uint64)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_disk_concentric_and_cosine_hemisphere(probe, prec):
    """Shirley-Chiu on chosen draws.  At most five roundings of quantities <= 1 (the quotient, its product with pi/4, the
    polynomial's result, the product with the radius; 2u - 1 is exact), doubled: 2^-50 in fp64; in fp32 the same count
    times 2^-24, doubled.  cosine_hemisphere takes its two draws from a CRAFTED state (first draw = u.y) and
    must leave the stream exactly two draws further."""
    bits, shift, f32 = (31, 1, False) if prec == "f64" else (24, 8, True)
    bound = 2.0 ** -50 if prec == "f64" else 10 * U32
    k = _disk_pairs(bits)
    u = k.astype(np.float64) / 2.0 ** bits
    rx, ry = M.disk_concentric_ld(u[:, 0], u[:, 1])
    got = run(probe, "disk_concentric", prec, u, 2)
    err = np.maximum(np.abs(got[:, 0].astype(LD) - rx), np.abs(got[:, 1].astype(LD) - ry)).astype(np.float64)
    w = report(f"disk_concentric {prec} [abs]", err, lambda i: f"k = {k[i].tolist()}")
    assert w <= bound, (w, bound)
    centre = (k[:, 0] == 1 << (bits - 1)) & (k[:, 1] == 1 << (bits - 1))
    assert centre.any() and (got[centre] == 0).all()
    r2 = got[:, 0].astype(LD) ** 2 + got[:, 1].astype(LD) ** 2
    print(f"[device-math] disk_concentric {prec}: max x^2 + y^2 - 1 = {float((r2 - 1).max()):.4g}")
    assert (r2 <= 1 + (2.0 ** -51 if prec == "f64" else 4 * U32)).all()
    # cosine_hemisphere: first draw = u.y, second = u.x
    state = M.craft_state(k[:, 1], k[:, 0], shift=shift)
    draws, after = M.rng_draws(state, 3, f32=f32)
    assert np.array_equal(draws[:, 0], u[:, 1]) and np.array_equal(draws[:, 1], u[:, 0])
    h = run(probe, "cosine_hemisphere", prec, state, 4)
    assert np.array_equal(h[:, :2], got), "cosine_hemisphere does not feed disk_concentric (second draw, first draw)"
    assert np.array_equal(h[:, 3].astype(np.float64), draws[:, 2]), "cosine_hemisphere consumed other than two draws"
    _, _, rz = M.cosine_hemisphere_ld(u[:, 1], u[:, 0])
    assert np.isfinite(h[:, 2]).all() and (h[:, 2] >= 0).all()
    assert np.array_equal(h[centre][:, :3], np.broadcast_to(np.array([0.0, 0.0, 1.0]), h[centre][:, :3].shape))
    # z = sqrt(1 - x^2 - y^2): compare z^2, which is as well conditioned as x and y are (z itself is not, at the rim)
    ez = np.abs(h[:, 2].astype(LD) ** 2 - rz ** 2).astype(np.float64)
    wz = report(f"cosine_hemisphere {prec} z^2 [abs]", ez, lambda i: f"k = {k[i].tolist()}")
    assert wz <= 4 * bound, (wz, bound)  # x^2 + y^2 moves by <= 2 (|x| + |y|) bound / 2 ... <= 2 bound; two more roundings
    # the raw stream: the first draws of the crafted states, and of arbitrary states, are the model's
    st = np.concatenate([state[: 1 << 12], np.random.default_rng(29).integers(1, 1 << 63, size=1 << 12).astype(np.uint64)])
    want, _ = M.rng_draws(st, M.RNG_DRAWS, f32=f32)
    assert np.array_equal(run(probe, "rng_next", prec, st, M.RNG_DRAWS).astype(np.float64), want)


# ================================================================== conservative conversions, the box test
def test_f32_up_and_f32_down_bracket_their_argument(probe):
    """f32_up(x) >= x >= f32_down(x), exactly (a float and a double compare exactly as doubles; a subset again as Fractions),
    and strictly wherever x is not itself a float (the widening by 2^-22 is there)."""
    from fractions import Fraction
    rng = np.random.default_rng(30)
    x = np.concatenate([M.binade_inputs(rng, -120, 120, 16), -M.binade_inputs(rng, -120, 120, 4), [0.0, 1e-4, 1e-3, 1e30, 1.0, -1.0],
                        rng.random(1 << 14), (rng.integers(0, 1 << 24, size=1 << 12) + 0.5) * 2.0 ** -24])  # the last: float ties
    got = run(probe, "f32_updown", "f64", x[:, None], 2, out_dtype=np.float32).astype(np.float64)
    assert (got[:, 1] >= x).all() and (x >= got[:, 0]).all()
    nz = x != 0
    assert (got[nz, 1] > x[nz]).all() and (x[nz] > got[nz, 0]).all()
    for i in range(0, x.size, 997):
        assert Fraction(got[i, 1]) >= Fraction(x[i]) >= Fraction(got[i, 0])
    print(f"[device-math] f32_up / f32_down: max widening {float(np.max((got[nz, 1] - got[nz, 0]) / np.abs(x[nz]))):.4g} relative")
    assert ((got[nz, 1] - got[nz, 0]) <= 8e-7 * np.abs(x[nz])).all()  # 2 * (2^-24 + 2.4e-7 + their roundings): still a tight bracket
    # what the kernels pass: tmax through f32_up, tmin through f32_down
    tmax = np.array([1e30, 1e300, np.inf])
    up = run(probe, "f32_updown", "f64", tmax[:, None], 2, out_dtype=np.float32)[:, 1].astype(np.float64)
    assert (up >= tmax).all() and up[1] == np.inf and up[2] == np.inf, up.tolist()
    tmin = np.array([0.0, 1e-4, 1e-3])
    dn = run(probe, "f32_updown", "f64", tmin[:, None], 2, out_dtype=np.float32)[:, 0].astype(np.float64)
    assert (dn <= tmin).all() and dn[0] == 0 and (dn[1:] > 0.999999 * tmin[1:]).all(), dn.tolist()
    # fp32 origins: the argument is a float already, the bracket still holds
    x32 = x[np.abs(x) < 1e30].astype(np.float32)
    got = run(probe, "f32_updown", "f32", x32[:, None], 2)
    assert (got[:, 1] >= x32).all() and (x32 >= got[:, 0]).all()


def _run_box(L, prec, c):
    import torch
    dt = np.float64 if prec == "f64" else np.float32
    n = c["o"].shape[0]
    ray = np.concatenate([c["o"], c["d"], c["tmin"][:, None], c["tmax"][:, None]], axis=1)
    with np.errstate(over="ignore"):
        d_ray = torch.from_numpy(np.ascontiguousarray(ray.astype(dt))).cuda()
    d_grid = torch.from_numpy(np.ascontiguousarray(c["grid"], dtype=np.float32)).cuda()
    d_box = torch.from_numpy(np.ascontiguousarray(c["packed"]).view(np.int32)).cuda()
    d_out = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    rc = getattr(L, f"prtprobe_box4_{prec}")(d_ray.data_ptr(), d_grid.data_ptr(), d_box.data_ptr(), d_out.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return d_out.cpu().numpy().reshape(n, 4)


@pytest.fixture(scope="module")
def box_cases():
    return M.box_cases()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_box_test_is_conservative_and_not_vacuous(probe, box_cases, prec):
    """The DEVICE's slab_axis + Trav::box4 (plain and packed-FMA) against the exact box test on ~2^20 (ray, box) pairs.
    Conservative: wherever the exact test accepts, the device has n <= f — no exception allowed.  Not vacuous: wherever the
    exact entry exceeds the exact exit by more than four pads, the device rejects."""
    c = dict(box_cases)
    if prec == "f32":  # the ray the fp32 kernels trace IS the rounded one: the exact test sees the same ray
        c["o"] = c["o"].astype(np.float32).astype(np.float64)
        with np.errstate(over="ignore", under="ignore"):
            c["d"] = c["d"].astype(np.float32).astype(np.float64)
        c["r"] = c["grid"][:, 1:4].astype(np.float64) - c["o"]
    acc, rej = M.box_expectations(c)
    out = _run_box(probe, prec, c)
    with np.errstate(invalid="ignore"):
        dev_acc = out[:, 0] <= out[:, 1]
    lost, kept = acc & ~dev_acc, rej & dev_acc
    print(f"[device-math] box4 {prec}: {out.shape[0]} pairs, exact accepts {int(acc.sum())}, device accepts {int(dev_acc.sum())}, "
          f"clearly rejected {int(rej.sum())}; violations: conservative {int(lost.sum())}, vacuous {int(kept.sum())}")
    assert acc.sum() >= 10 ** 4 and rej.sum() >= 10 ** 4
    assert not lost.any(), (int(lost.sum()), int(np.nonzero(lost)[0][0]))
    assert not kept.any(), (int(kept.sum()), int(np.nonzero(kept)[0][0]))
    assert np.array_equal(out[:, :2].view(np.uint32), out[:, 2:].view(np.uint32)), "plain and packed box4 differ"


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_empty_slot_is_rejected_by_its_range_near_the_scene(probe, prec):
    c = M.empty_slot_cases()
    out = _run_box(probe, prec, c)
    with np.errstate(invalid="ignore"):
        dev_acc = out[:, 0] <= out[:, 1]
    print(f"[device-math] box4 {prec}: empty slot accepted for {int(dev_acc.sum())} of {dev_acc.size} rays within 2^17 extents")
    assert not dev_acc.any()
    assert np.array_equal(out[:, :2].view(np.uint32), out[:, 2:].view(np.uint32))


# ================================================================== the BSDF layer
def run_state(L, name, prec, rows, states):
    """mat_eval / mat_scatter on (rows, 64-bit RNG states): returns (outputs, states after)."""
    import torch
    ni, no = M.STATE_OPS[name]
    dt = np.float64 if prec == "f64" else np.float32
    rows = np.ascontiguousarray(rows.astype(dt))
    n = rows.shape[0]
    assert rows.shape[1] == ni and states.shape == (n,) and n <= 1 << 16
    d_in = torch.from_numpy(rows.reshape(-1)).cuda()
    d_st = torch.from_numpy(np.ascontiguousarray(states).view(np.int64)).cuda()
    d_out = torch.zeros(n * no, dtype=torch.float32 if prec == "f32" else torch.float64, device="cuda")
    d_after = torch.zeros(n, dtype=torch.int64, device="cuda")
    rc = getattr(L, f"prtprobe_{name}_{prec}")(d_in.data_ptr(), d_st.data_ptr(), d_out.data_ptr(), d_after.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, prec, rc)
    return d_out.cpu().numpy().reshape(n, no), d_after.cpu().numpy().view(np.uint64)


BSDF_HELPERS = ["tan2theta", "cosphi", "sinphi", "ct_D", "ct_lambda", "ct_G1", "ct_G", "ct_Dv", "ct_fresnel"]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", BSDF_HELPERS)
def test_bsdf_helpers_against_the_mpmath_model(probe, name, prec):
    """The CookTorrance terms on their own, every stratum of device_math_model.bsdf_inputs: within twice the model's running
    bound plus one subnormal quantum; finite wherever the exact value is finite — the grazing strata cross the window in
    which ct_D's cos4 underflows while sqr(1 + e) overflows; D, G, G1, F, Lambda, Dv >= 0; G1, G <= 1."""
    R = M.bsdf_reference(name, prec)
    assert len(R["rows"]) <= 1 << 16 and not R["knife"].any()
    got = run(probe, name, prec, R["rows"], M.BSDF_OPS[name])
    ratio, fails = M.bsdf_compare(R, got)
    assert not fails, fails


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_mat_eval_against_the_mpmath_model(probe, prec):
    """Material::Eval of the Lambertian, Phong (every Ns of the sources; the real lobe probabilities and both forced lobes;
    crafted first draws at the lattice's ends) and CookTorrance (every alpha and (eta, k) of the sources, alpha 1e-3, 1 and
    (0.01, 1)) materials.  Opposite sides and exact zeros give exactly 0; the stream is left one draw further for Phong and
    untouched otherwise; a light and an eye that both graze the surface give a finite value down to z = 2^-60 / 2^-500."""
    R = M.bsdf_reference("mat_eval", prec)
    got, after = run_state(probe, "mat_eval", prec, R["rows"], R["states"])
    ratio, fails = M.bsdf_compare(R, got, after)
    assert not fails, fails
    z = (R["stratum"] == "opposite_or_zero") & ((R["rows"][:, 0] == 3) | (R["rows"][:, 19] <= 0))  # CookTorrance; Phong with wi.z <= 0
    assert z.sum() >= 64 and (R["ref"][z] == 0).all() and (got[z] == 0).all()
    assert np.array_equal(R["draws"][~R["undef"]], (R["rows"][~R["undef"], 0] == 1).astype(np.int64))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_mat_scatter_against_the_mpmath_model(probe, prec):
    """Material::Scatter: `ok`, the scattered direction, att and the RNG state afterwards against the model (which counts the
    draws), on the upright and a tilted frame, unnormalised incoming rays, crafted draws at 0, one step, 1/2 and the top of
    the lattice.  att is held against the CLOSED FORMS — kd (Lambertian, Phong diffuse), Ks (Ns+2)/(Ns+1) wi.z and 0 below
    the horizon (Phong specular), 1 (mirror), F G(wo, wi) / G1(wo) (CookTorrance, on the model's exact directions) — within
    the tolerance the model derives for the header's expression fr * wi.z / pdf, in which D is computed twice and divided
    out: an over- or underflow of D would show as 0/0 here."""
    R = M.bsdf_reference("mat_scatter", prec)
    got, after = run_state(probe, "mat_scatter", prec, R["rows"], R["states"])
    ratio, fails = M.bsdf_compare(R, got, after)
    assert not fails, fails
    P = M.PRECS[prec]
    live = ~R["undef"]
    ok = live & (got[:, 0] == 1)
    assert set(np.unique(got[:, 0]).tolist()) <= {0.0, 1.0}
    assert (got[live & (got[:, 0] == 0), 1:] == 0).all()
    assert np.isfinite(got[live]).all()
    # a unit vector within normalize's bound (test_normalize_fp64_and_fp32: 4 ulp of 1)
    nrm = np.abs(np.sqrt((got[ok, 1:4].astype(LD) ** 2).sum(1)) - 1).astype(np.float64) / (2 * float(P.u))
    wn = report(f"mat_scatter {prec} |wi_world| - 1 [ulp]", nrm, lambda i: R["rows"][ok][i].tolist())
    assert wn <= 4, wn
    # att against the closed form, with the tolerance of the header's expression
    checked = ok & ~R["knife"] & ~np.isnan(R["closed"].astype(np.float64)).any(1)
    err = np.abs(got[checked, 4:7].astype(LD) - R["closed"][checked]).astype(np.float64)
    rc = np.where(np.isfinite(R["tol"][checked, 4:7]), err / R["tol"][checked, 4:7], 0).max(1)
    wc = report(f"mat_scatter {prec} att vs closed form / tolerance", rc, lambda i: R["rows"][checked][i].tolist())
    assert checked.sum() >= 0.6 * len(R["rows"]) and wc <= 1, wc
    with np.errstate(all="ignore"):
        rel = (err / np.abs(R["closed"][checked]).astype(np.float64))[R["closed"][checked].astype(np.float64) > 0]
    print(f"[bsdf] mat_scatter {prec}: att vs closed form, worst relative error {rel.max():.4g} over {int(checked.sum())} samples; "
          f"bounds that are infinite: {int((~np.isfinite(R['tol'][checked, 4:7])).any(1).sum())}")
    # the rim rows (knife-edge by construction: the cosine sample may be drawn again): att is kd whichever sample was taken.
    # (fr wi.z) rcp(pdf) / fr wi.z / pdf: five roundings and one reciprocal, twice, as everywhere
    # (rows of the stratum that ended in the specular lobe after all — the all-zero crafted state is replaced — are left to the checks above)
    rim = live & (R["stratum"] == "rng_rim") & (np.abs(R["closed"].astype(np.float64) - R["rows"][:, 1:4]) <= 1e-7 * R["rows"][:, 1:4]).all(1)
    tol = 2 * (2.5 + P.k_fast) * float(P.u) * np.abs(R["rows"][rim, 1:4])
    assert rim.sum() >= 64 and (np.abs(got[rim, 4:7].astype(np.float64) - R["rows"][rim, 1:4]) <= tol).all()
    assert (got[rim, 3] > 0).all()  # and the direction it left with is above the surface (upright frame)
