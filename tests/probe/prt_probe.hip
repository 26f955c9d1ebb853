// prt_probe.hip — TEST-ONLY probe of the device primitives of pooraytracer_amd/csrc/prt_device.h.
//
// Every primitive is wrapped in a trivial element-wise kernel behind an extern "C" launcher that takes device pointers,
// the element count and a stream (tests/test_gpu_device_math.py drives them; tests/device_math_model.py holds the
// references).  Built into tests/probe/libprt_probe.so by pooraytracer_amd/build.py:build_probe(); never linked into
// libprt_hip.so / libprt_hip_dev.so (tests/test_device_math_cpu.py checks their exports).
//
// Like prt_kernels.hip this file is compiled twice: as it stands (real = double, launchers prtprobe_<op>_f64) and through
// prt_probe_f32.hip with PRT_REAL = float (launchers prtprobe_<op>_f32).  The two definitions of real / d3 / Rng / Trav
// never meet: each translation unit keeps its kernels in an unnamed namespace and exports only the suffixed launchers.
//
// RULE: no op forms an address from an input VALUE.  Element i reads in[i * NI ..] and writes out[i * NO ..], nothing
// else; NaN, Inf and out-of-domain inputs are therefore arithmetic only and cannot fault.  (tex_value is not probed for
// that reason: its index comes from (int)x.)
#include <hip/hip_runtime.h>

#include "../../pooraytracer_amd/csrc/prt_device.h" // unmodified

#ifndef PRT_PROBE_F32
#define PRT_PROBE_F32 0
#endif
#if PRT_PROBE_F32
#define PROBE_SYM(name) prtprobe_##name##_f32
#else
#define PROBE_SYM(name) prtprobe_##name##_f64
#endif

namespace {
template <typename F>
__global__ void __launch_bounds__(256) k_each(size_t n, F f) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) f(i);
}
template <typename F>
int launch_each(size_t n, hipStream_t stream, F f) {
    if (n == 0) return 0;
    if (n > (size_t(1) << 24)) return -1; // the tests never need more; keeps the grid far below every limit
    hipLaunchKernelGGL(k_each<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, f);
    return (int)hipGetLastError();
}
} // namespace

// An op over `real` records: element i reads NI reals at a = in + i * NI and writes NO reals at o = out + i * NO.
#define PROBE_REAL(name, NI, NO, ...)                                                                    \
    extern "C" int PROBE_SYM(name)(const void* in_, void* out_, size_t n, hipStream_t stream) {          \
        const real* in = static_cast<const real*>(in_);                                                  \
        real* out = static_cast<real*>(out_);                                                            \
        return launch_each(n, stream, [=] __device__(size_t i) {                                         \
            const real* a = in + i * (NI);                                                               \
            real* o = out + i * (NO);                                                                    \
            __VA_ARGS__                                                                                  \
        });                                                                                              \
    }

// ------------------------------------------------------------------ arithmetic
PROBE_REAL(fast_rsqrt, 1, 1, o[0] = fast_rsqrt(a[0]);)
PROBE_REAL(fast_sqrt, 1, 1, o[0] = fast_sqrt(a[0]);)
PROBE_REAL(fast_rcp, 1, 1, o[0] = fast_rcp(a[0]);)
PROBE_REAL(fast_div, 2, 1, o[0] = fast_div(a[0], a[1]);)
PROBE_REAL(ieee_sqrt, 1, 1, o[0] = ieee_sqrt(a[0]);)
PROBE_REAL(ieee_div, 2, 1, o[0] = ieee_div(a[0], a[1]);)
PROBE_REAL(normalize, 3, 3, const d3 v = normalize(mk3(a[0], a[1], a[2])); o[0] = v.x; o[1] = v.y; o[2] = v.z;)
PROBE_REAL(normalize_len, 3, 4, real len; const d3 v = normalize_len(mk3(a[0], a[1], a[2]), len); o[0] = v.x; o[1] = v.y;
           o[2] = v.z; o[3] = len;)

// ------------------------------------------------------------------ FMA helpers with a literal operand
// The literal must be a compile-time value (an "s" operand of the inline v_fma_f64): five fixed constants, among them
// real coefficients of sincos_quarter (K0, K2) and pow_pos (K1, K3 = ln2_lo, K4 = 1/ln2).  tests/device_math_model.py
// lists the same five.
#define PROBE_K0 8.33333333332248946124e-03
#define PROBE_K1 6.666666666666735130e-01
#define PROBE_K2 -1.66666666666666324348e-01
#define PROBE_K3 1.90821492927058770002e-10
#define PROBE_K4 1.44269504088896338700e+00
PROBE_REAL(fma_ks, 2, 5, o[0] = fma_ks(a[0], a[1], RL(PROBE_K0)); o[1] = fma_ks(a[0], a[1], RL(PROBE_K1));
           o[2] = fma_ks(a[0], a[1], RL(PROBE_K2)); o[3] = fma_ks(a[0], a[1], RL(PROBE_K3));
           o[4] = fma_ks(a[0], a[1], RL(PROBE_K4));)
#if !PRT_PROBE_F32 // fma_sk / mul_ks exist in fp64 only (pow_pos's fp64 body is their one user)
PROBE_REAL(fma_sk, 2, 5, o[0] = fma_sk(a[0], PROBE_K0, a[1]); o[1] = fma_sk(a[0], PROBE_K1, a[1]);
           o[2] = fma_sk(a[0], PROBE_K2, a[1]); o[3] = fma_sk(a[0], PROBE_K3, a[1]); o[4] = fma_sk(a[0], PROBE_K4, a[1]);)
PROBE_REAL(mul_ks, 1, 5, o[0] = mul_ks(a[0], PROBE_K0); o[1] = mul_ks(a[0], PROBE_K1); o[2] = mul_ks(a[0], PROBE_K2);
           o[3] = mul_ks(a[0], PROBE_K3); o[4] = mul_ks(a[0], PROBE_K4);)
#endif

// ------------------------------------------------------------------ transcendentals
PROBE_REAL(sincos_quarter, 1, 2, real s, c; sincos_quarter(a[0], s, c); o[0] = s; o[1] = c;)
PROBE_REAL(sincos_turns, 1, 2, real s, c; sincos_turns(a[0], s, c); o[0] = s; o[1] = c;)
// input u (turns); theta = 2 pi u is formed as ct_sample_wm forms it
PROBE_REAL(sincos_any, 1, 2, real s, c; sincos_any(2 * PRT_PI * a[0], a[0], s, c); o[0] = s; o[1] = c;)
PROBE_REAL(pow_pos, 2, 1, o[0] = pow_pos(a[0], a[1]);)

// ------------------------------------------------------------------ Fresnel
PROBE_REAL(csqrt, 2, 2, const Cx z = csqrt_(cx(a[0], a[1])); o[0] = z.re; o[1] = z.im;)
PROBE_REAL(fr_complex, 3, 1, o[0] = fr_complex(a[0], cx(a[1], a[2]));) // cos, eta, k

// ------------------------------------------------------------------ samplers
PROBE_REAL(disk_concentric, 2, 2, const d2 p = disk_concentric(d2{a[0], a[1]}); o[0] = p.x; o[1] = p.y;)
// alpha_x, alpha_y, w.xyz, u.xy -> wm.xyz
PROBE_REAL(ct_sample_wm, 7, 3, DMaterial m = {}; m.alpha_x = a[0]; m.alpha_y = a[1];
           const d3 wm = ct_sample_wm(m, mk3(a[2], a[3], a[4]), d2{a[5], a[6]}); o[0] = wm.x; o[1] = wm.y; o[2] = wm.z;)

// ------------------------------------------------------------------ the BSDF layer: CookTorrance terms
PROBE_REAL(tan2theta, 3, 1, o[0] = tan2theta(mk3(a[0], a[1], a[2]));)
PROBE_REAL(cosphi, 3, 1, o[0] = cosphi(mk3(a[0], a[1], a[2]));)
PROBE_REAL(sinphi, 3, 1, o[0] = sinphi(mk3(a[0], a[1], a[2]));)
// alpha_x, alpha_y, then the directions
#define PROBE_ALPHA DMaterial m = {}; m.alpha_x = a[0]; m.alpha_y = a[1];
PROBE_REAL(ct_D, 5, 1, PROBE_ALPHA o[0] = ct_D(m, mk3(a[2], a[3], a[4]));)
PROBE_REAL(ct_lambda, 5, 1, PROBE_ALPHA o[0] = ct_lambda(m, mk3(a[2], a[3], a[4]));)
PROBE_REAL(ct_G1, 5, 1, PROBE_ALPHA o[0] = ct_G1(m, mk3(a[2], a[3], a[4]));)
PROBE_REAL(ct_G, 8, 1, PROBE_ALPHA o[0] = ct_G(m, mk3(a[2], a[3], a[4]), mk3(a[5], a[6], a[7]));)  // wo, wi
PROBE_REAL(ct_Dv, 8, 1, PROBE_ALPHA o[0] = ct_Dv(m, mk3(a[2], a[3], a[4]), mk3(a[5], a[6], a[7]));) // w, wm
// eta[3], k[3], wo, wm -> F per channel
PROBE_REAL(ct_fresnel, 12, 3, DMaterial m = {}; for (int c = 0; c < 3; ++c) m.eta[c] = a[c], m.k[c] = a[3 + c];
           const d3 F = ct_fresnel(m, mk3(a[6], a[7], a[8]), mk3(a[9], a[10], a[11])); o[0] = F.x; o[1] = F.y; o[2] = F.z;)

// ------------------------------------------------------------------ the BSDF layer: Material::Eval and Material::Scatter
// An untextured material from its RAW fields, 17 reals: type, kd[3], ks[3], ns, eta[3], k[3], alpha_x, alpha_y, pkd.  The
// derived fields are filled as scene_setup.cpp:setup_materials fills them — in double, from the double ns — and then rounded
// to `real` as prt_api.cpp makes the fp32 material table.  pkd >= 0 overrides the lobe probabilities (pkd, 1 - pkd): 0 and 1
// force a lobe; a negative value keeps SetProbabilitiesByNs' 1 / 0 or 0.6 / 0.4.
#define PROBE_MAT_NI 17
namespace {
__device__ __forceinline__ DMaterial probe_material(const real* a) {
    DMaterial m = {};
    m.type = (int32_t)a[0];
    m.texture = -1;
    for (int c = 0; c < 3; ++c) m.kd[c] = a[1 + c], m.ks[c] = a[4 + c], m.eta[c] = a[8 + c], m.k[c] = a[11 + c];
    const double ns = (double)a[7];
    m.ns = a[7];
    m.inv_ns1 = (real)(1.0 / (ns + 1.0));
    m.spec_scale = (real)((ns + 2.0) / (ns + 1.0));
    m.pkd = (real)(ns <= 9. ? 1.0 : 0.6);
    m.pks = (real)(ns <= 9. ? 0.0 : 0.4);
    if (a[16] >= 0) m.pkd = a[16], m.pks = RL(1.) - a[16];
    m.alpha_x = a[14];
    m.alpha_y = a[15];
    return m;
}
// The all-zero state is xoroshiro's fixed point (every draw 0, and the sampling loops `while (wi.z <= 0)` would never end);
// Rng::seed_keyed never produces it, and this replaces it the same way.
__device__ __forceinline__ uint64_t probe_state(uint64_t s) { return s ? s : 0x9E3779B97F4A7C15ULL; }
} // namespace
// in[i] = material (17), wi.xyz, wo.xyz (local frame, z the shading normal); state[i]; out[i] = f.xyz; state_out[i]
extern "C" int PROBE_SYM(mat_eval)(const void* in_, const void* state_, void* out_, void* state_out_, size_t n, hipStream_t stream) {
    const real* in = static_cast<const real*>(in_);
    const uint64_t* state = static_cast<const uint64_t*>(state_);
    real* out = static_cast<real*>(out_);
    uint64_t* state_out = static_cast<uint64_t*>(state_out_);
    return launch_each(n, stream, [=] __device__(size_t i) {
        const real* a = in + i * (PROBE_MAT_NI + 6);
        const DMaterial m = probe_material(a);
        DScene S = {};
        Rng g;
        g.s = probe_state(state[i]);
        const d3 f = mat_eval<PRT_FEAT_PHONG | PRT_FEAT_CT>(S, m, mk3(a[17], a[18], a[19]), mk3(a[20], a[21], a[22]), d2{RL(0.), RL(0.)}, g);
        out[i * 3] = f.x, out[i * 3 + 1] = f.y, out[i * 3 + 2] = f.z;
        state_out[i] = g.s;
    });
}
// in[i] = material (17), rd.xyz, frame normal.xyz, frame tangent.xyz; out[i] = ok, wi_world.xyz, att.xyz (zeros where the
// function leaves them unassigned)
extern "C" int PROBE_SYM(mat_scatter)(const void* in_, const void* state_, void* out_, void* state_out_, size_t n, hipStream_t stream) {
    const real* in = static_cast<const real*>(in_);
    const uint64_t* state = static_cast<const uint64_t*>(state_);
    real* out = static_cast<real*>(out_);
    uint64_t* state_out = static_cast<uint64_t*>(state_out_);
    return launch_each(n, stream, [=] __device__(size_t i) {
        const real* a = in + i * (PROBE_MAT_NI + 9);
        const DMaterial m = probe_material(a);
        DScene S = {};
        Rng g;
        g.s = probe_state(state[i]);
        Frame f;
        f.n = mk3(a[20], a[21], a[22]);
        f.t = mk3(a[23], a[24], a[25]);
        d3 att = mk3(0, 0, 0), wi = mk3(0, 0, 0);
        const bool ok = mat_scatter<PRT_FEAT_PHONG | PRT_FEAT_CT>(S, m, mk3(a[17], a[18], a[19]), f, d2{RL(0.), RL(0.)}, g, att, wi);
        real* o = out + i * 7;
        o[0] = ok ? RL(1.) : RL(0.);
        o[1] = wi.x, o[2] = wi.y, o[3] = wi.z;
        o[4] = att.x, o[5] = att.y, o[6] = att.z;
        state_out[i] = g.s;
    });
}

// ------------------------------------------------------------------ RNG (raw 64-bit states in, reals out)
#define PROBE_RNG_DRAWS 4
extern "C" int PROBE_SYM(rng_next)(const void* in_, void* out_, size_t n, hipStream_t stream) {
    const uint64_t* in = static_cast<const uint64_t*>(in_);
    real* out = static_cast<real*>(out_);
    return launch_each(n, stream, [=] __device__(size_t i) {
        Rng g;
        g.s = in[i];
        for (int k = 0; k < PROBE_RNG_DRAWS; ++k) out[i * PROBE_RNG_DRAWS + k] = g.next();
    });
}
// state -> cosine_hemisphere(rng).xyz and the draw that FOLLOWS it (the third of the stream if exactly two were consumed)
extern "C" int PROBE_SYM(cosine_hemisphere)(const void* in_, void* out_, size_t n, hipStream_t stream) {
    const uint64_t* in = static_cast<const uint64_t*>(in_);
    real* out = static_cast<real*>(out_);
    return launch_each(n, stream, [=] __device__(size_t i) {
        Rng g;
        g.s = in[i];
        const d3 w = cosine_hemisphere(g);
        out[i * 4] = w.x;
        out[i * 4 + 1] = w.y;
        out[i * 4 + 2] = w.z;
        out[i * 4 + 3] = g.next();
    });
}

// ------------------------------------------------------------------ box test
// x -> f32_down(x), f32_up(x)
extern "C" int PROBE_SYM(f32_updown)(const void* in_, void* out_, size_t n, hipStream_t stream) {
    const real* in = static_cast<const real*>(in_);
    float* out = static_cast<float*>(out_);
    return launch_each(n, stream, [=] __device__(size_t i) {
        out[i * 2] = f32_down(in[i]);
        out[i * 2 + 1] = f32_up(in[i]);
    });
}
// ray[i] = o.xyz, d.xyz, tmin, tmax (8 reals); grid[i] = slab_scale, grid_origin[3], grid_step[3] (7 floats) of a stub
// DScene; box[i] = the three packed (lo | hi << 16) ranges.  out[i] = (n, f) of Trav<false,false>::box4, then (n, f) of
// the packed-FMA variant Trav<false,true>::box4.  The stub scene's pointers stay null: start() and box4() read none.
extern "C" int PROBE_SYM(box4)(const void* ray_, const void* grid_, const void* box_, void* out_, size_t n, hipStream_t stream) {
    const real* ray = static_cast<const real*>(ray_);
    const float* grid = static_cast<const float*>(grid_);
    const uint32_t* box = static_cast<const uint32_t*>(box_);
    float* out = static_cast<float*>(out_);
    return launch_each(n, stream, [=] __device__(size_t i) {
        const real* r = ray + i * 8;
        const float* g = grid + i * 7;
        DScene S = {};
        S.n_tris = 1;
        S.slab_scale = g[0];
        for (int a = 0; a < 3; ++a) S.grid_origin[a] = g[1 + a], S.grid_step[a] = g[4 + a];
        const uint32_t x = box[i * 3], y = box[i * 3 + 1], z = box[i * 3 + 2];
        Trav<false, false> t0;
        t0.init(S, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), r[6], r[7]);
        Trav<false, true> t1;
        t1.init(S, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), r[6], r[7]);
        float nn, ff;
        t0.box4(x, y, z, nn, ff);
        out[i * 4] = nn, out[i * 4 + 1] = ff;
        t1.box4(x, y, z, nn, ff);
        out[i * 4 + 2] = nn, out[i * 4 + 3] = ff;
    });
}

#if PRT_PROBE_F32
// the two instructions of the fp32 pow_pos on their own (base 2), for the CPU-side recheck against longdouble
PROBE_REAL(v_log, 1, 1, o[0] = __builtin_amdgcn_logf(a[0]);)
PROBE_REAL(v_exp, 1, 1, o[0] = __builtin_amdgcn_exp2f(a[0]);)
// ------------------------------------------------------------------ exhaustive fp32 checks (reduced on the device)
// Float bit patterns first .. first + count - 1 go through op OP; each result is compared with the correctly rounded
// fp64 operation rounded to float (1 / sqrt: an fp64 sqrt and an fp64 division, so two fp64 roundings before the one to
// float — a near-tie can move that reference by one float step, which the <= 1 ulp assertion then counts against the op).  res[0] = max over the inputs whose reference is a NORMAL float of
// (ulp distance << 32 | input bits), res[1] = how many of those are more than 1 ulp off, res[2] = results that are NaN
// or carry the wrong sign (for any reference), res[3] = max |result - reference| in units of 2^-149 over the inputs whose
// reference is subnormal or zero (float bits of the difference's magnitude, as an integer).
namespace {
template <int OP>
__device__ __forceinline__ float x_op(float x) {
    switch (OP) {
    case 0: return __builtin_amdgcn_rcpf(x);
    case 1: return __builtin_amdgcn_rsqf(x);
    case 2: return __builtin_amdgcn_sqrtf(x);
    case 3: return fast_rcp(x);
    case 4: return fast_rsqrt(x);
    case 5: return fast_sqrt(x);
    case 6: return ieee_sqrt(x);
    case 7: return __builtin_amdgcn_logf(x);  // v_log_f32: log2
    default: return __builtin_amdgcn_exp2f(x); // v_exp_f32: 2^x
    }
}
template <int OP>
__device__ __forceinline__ float x_ref(float x) {
    const double d = (double)x;
    switch (OP) {
    case 0: case 3: return (float)(1.0 / d);
    case 1: case 4: return (float)(1.0 / sqrt(d));
    case 7: return (float)log2(d);
    case 8: return (float)exp2(d);
    default: return (float)sqrt(d);
    }
}
__device__ __forceinline__ int32_t ordered(float f) { // monotone map of floats to integers
    const int32_t b = (int32_t)__float_as_uint(f);
    return b < 0 ? (int32_t)0x80000000 - b : b;
}
#define PROBE_X_PER_THREAD 256
template <int OP>
__global__ void __launch_bounds__(256) k_exhaust(uint32_t first, unsigned long long count, unsigned long long* res) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long worst = 0, over = 0, bad = 0, sub = 0;
    for (int j = 0; j < PROBE_X_PER_THREAD; ++j) {
        // consecutive lanes take consecutive patterns
        const unsigned long long idx = ((t >> 6) * PROBE_X_PER_THREAD + j) * 64 + (t & 63);
        if (idx >= count) break;
        const uint32_t bits = first + (uint32_t)idx;
        const float x = __uint_as_float(bits);
        const float got = x_op<OP>(x), ref = x_ref<OP>(x);
        if (got != got || (signbit(got) != signbit(ref))) bad++;
        if (fabsf(ref) >= 1.17549435e-38f && fabsf(ref) <= 3.40282347e+38f) {
            const long long d = (long long)ordered(got) - (long long)ordered(ref);
            const unsigned long long u = (got != got) ? 0xffffffffull : (unsigned long long)(d < 0 ? -d : d);
            if (u > 1) over++;
            const unsigned long long key = (u << 32) | bits;
            worst = key > worst ? key : worst;
        } else if (got == got) {
            const long long d = (long long)ordered(got) - (long long)ordered(ref);
            const unsigned long long u = (unsigned long long)(d < 0 ? -d : d);
            sub = u > sub ? u : sub;
        }
    }
    if (worst) atomicMax(&res[0], worst);
    if (over) atomicAdd(&res[1], over);
    if (bad) atomicAdd(&res[2], bad);
    if (sub) atomicMax(&res[3], sub);
}
template <int OP>
int launch_exhaust(uint32_t first, unsigned long long count, unsigned long long* res, hipStream_t stream) {
    const unsigned long long per_block = 256ull * PROBE_X_PER_THREAD;
    const unsigned long long blocks = (count + per_block - 1) / per_block;
    if (count == 0 || (unsigned long long)first + count > (1ull << 32) || blocks > (1ull << 20)) return -1;
    hipLaunchKernelGGL(k_exhaust<OP>, dim3((unsigned)blocks), dim3(256), 0, stream, first, count, res);
    return (int)hipGetLastError();
}
} // namespace
// op: 0 v_rcp_f32, 1 v_rsq_f32, 2 v_sqrt_f32 (the raw instructions), 3 fast_rcp, 4 fast_rsqrt, 5 fast_sqrt, 6 ieee_sqrt
// (the fp32 overloads of prt_device.h), 7 v_log_f32, 8 v_exp_f32 (base 2: the two instructions of the fp32 pow_pos, against
// the fp64 library log2 / exp2 rounded to float).  `res`: four zeroed 64-bit words on the device.
extern "C" int prtprobe_exhaust_f32(int op, uint32_t first, unsigned long long count, void* res_, hipStream_t stream) {
    unsigned long long* res = static_cast<unsigned long long*>(res_);
    switch (op) {
    case 0: return launch_exhaust<0>(first, count, res, stream);
    case 1: return launch_exhaust<1>(first, count, res, stream);
    case 2: return launch_exhaust<2>(first, count, res, stream);
    case 3: return launch_exhaust<3>(first, count, res, stream);
    case 4: return launch_exhaust<4>(first, count, res, stream);
    case 5: return launch_exhaust<5>(first, count, res, stream);
    case 6: return launch_exhaust<6>(first, count, res, stream);
    case 7: return launch_exhaust<7>(first, count, res, stream);
    case 8: return launch_exhaust<8>(first, count, res, stream);
    default: return -1;
    }
}
#endif
