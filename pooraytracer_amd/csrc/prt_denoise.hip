// prt_denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010), spatial only, fp32,
// deterministic (no atomics).  prt_denoise / prt_accum_resolve_denoised (include/prt.h) launch it; the rule it implements
// is stated there and restated in numpy by tests/denoise_model.py.
//
//   k_dn_pack   colour [H][W][3] (divided by max(albedo, eps) with demodulation) and the features -> three float4 planes:
//               colour (r, g, b, 0), albedo + depth (a.rgb, z), normal (n.xyz, 0): one 16-byte load each per tap
//   k_dn_level  one level: 5x5 gather with step 2^i, B3 spline weights times the edge-stopping terms; the last level writes
//               the [H][W][3] output (multiplied back by max(albedo, eps) with demodulation) instead of a float4 plane
//
// The variance-guided form (prt_denoise_guided, SVGF-style colour weights; the rule is in include/prt.h and in numpy in
// tests/denoise_guided_model.py) is the GUIDED = true instantiation of the same two kernels: the colour plane's fourth lane
// carries the variance of the pixel's mean luminance, so a tap still costs three 16-byte loads and the scratch stays at 64
// bytes per pixel.  A guided level blurs the variance 3x3 at the centre (nine more loads from the plane it gathers from),
// uses sigma_color sqrt(blur) as the colour tolerance and propagates the variance as sum w^2 v / (sum w)^2.
//
// Memory-bound and cache-resident: a level reads 25 taps x 48 bytes per pixel, almost all of it from L2 (16x16 blocks: the
// taps of a block at step <= 16 cover at most a 80x80 window); only the three planes themselves come from HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "prt_launch.h"

namespace {

#define PRT_DN_TILE 16
#define PRT_DN_EPS 1e-3f // demodulation: c / max(a, eps)

struct DnLevel {
    int w, h, step;
    float ic, in, iz, ia; // 1 / sigma^2 of the colour (this level's sigma_c * 2^-i), normal, depth, albedo terms; 0 = off
    float sc;             // guided: sigma_color, the multiplier of the standard deviation (0 = off); ic is unused there
};

__device__ __forceinline__ bool finite3(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }
__device__ __forceinline__ float luma(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
// A variance that is negative, NaN or infinite counts as 0.
__device__ __forceinline__ float sane_variance(float v) { return (v >= 0.f && isfinite(v)) ? v : 0.f; }
// Y(max(a, eps))^2: what demodulation divides a variance by
__device__ __forceinline__ float luma_mod2(float ar, float ag, float ab) {
    const float y = luma(fmaxf(ar, PRT_DN_EPS), fmaxf(ag, PRT_DN_EPS), fmaxf(ab, PRT_DN_EPS));
    return y * y;
}

template <bool GUIDED>
__global__ void k_dn_pack(const float* __restrict__ rgb, const float* __restrict__ var, const float* __restrict__ albedo,
                          const float* __restrict__ normal, const float* __restrict__ depth, size_t n, int demod,
                          float4* __restrict__ col, float4* __restrict__ af, float4* __restrict__ nf) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float ar = albedo[i * 3], ag = albedo[i * 3 + 1], ab = albedo[i * 3 + 2];
    float r = rgb[i * 3], g = rgb[i * 3 + 1], b = rgb[i * 3 + 2];
    if (demod) {
        r = r / fmaxf(ar, PRT_DN_EPS);
        g = g / fmaxf(ag, PRT_DN_EPS);
        b = b / fmaxf(ab, PRT_DN_EPS);
    }
    float v = 0.f;
    if constexpr (GUIDED) {
        v = sane_variance(var[i]);
        if (demod) v = v / luma_mod2(ar, ag, ab);
    }
    col[i] = make_float4(r, g, b, v);
    af[i] = make_float4(ar, ag, ab, depth[i]);
    nf[i] = make_float4(normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2], 0.f);
}

// out_p = sum_q w c_q / sum_q w over the taps inside the image with a finite colour; a non-finite centre gives 0.
// w = h(dx) h(dy) exp(-(|c_p - c_q|^2 ic + |n_p - n_q|^2 in + (z_p - z_q)^2 iz / z_p^2 + |a_p - a_q|^2 ia)), the depth
// term only between two hits (z finite); a hit next to a miss gets weight 0 while the depth term is on.
// GUIDED: the colour term is |Y(c_p) - Y(c_q)| / (sc sqrt(g_p) + 1e-4) instead, g_p the 3x3 binomial blur (step 1, taps
// outside the image skipped and the rest renormalised) of the variance lane around p, and the variance lane of the output
// is sum_q w^2 v_q / (sum_q w)^2 (0 for a non-finite centre); the last level writes it to out_var if that is given.
template <bool GUIDED>
__global__ __launch_bounds__(PRT_DN_TILE * PRT_DN_TILE) void k_dn_level(DnLevel L, const float4* __restrict__ in,
                                                                       const float4* __restrict__ af, const float4* __restrict__ nf,
                                                                       float4* __restrict__ out, float* __restrict__ out_rgb,
                                                                       float* __restrict__ out_var, int demod) {
    const int x = blockIdx.x * PRT_DN_TILE + threadIdx.x, y = blockIdx.y * PRT_DN_TILE + threadIdx.y;
    if (x >= L.w || y >= L.h) return;
    const size_t p = (size_t)y * L.w + x;
    const float4 cp = in[p];
    const float4 ap = af[p];
    float rr = 0.f, rg = 0.f, rb = 0.f, rv = 0.f;
    if (finite3(cp)) {
        const float4 np = nf[p];
        const bool hit_p = isfinite(ap.w);
        const float iz = L.iz / (ap.w * ap.w);
        const float hk[5] = {1.f / 16.f, 4.f / 16.f, 6.f / 16.f, 4.f / 16.f, 1.f / 16.f};
        float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f, sv = 0.f;
        float ic = L.ic;
        if constexpr (GUIDED) {
            ic = 0.f;
            if (L.sc > 0.f) {
                const float bk[3] = {1.f, 2.f, 1.f};
                float gs = 0.f, gw = 0.f;
                for (int j = 0; j < 3; ++j) {
                    const int yy = y + j - 1;
                    if (yy < 0 || yy >= L.h) continue;
                    for (int i = 0; i < 3; ++i) {
                        const int xx = x + i - 1;
                        if (xx < 0 || xx >= L.w) continue;
                        gs += bk[i] * bk[j] * in[(size_t)yy * L.w + xx].w;
                        gw += bk[i] * bk[j];
                    }
                }
                ic = 1.f / (L.sc * sqrtf(gs / gw) + 1e-4f);
            }
        }
        for (int j = 0; j < 5; ++j) {
            const int yy = y + (j - 2) * L.step;
            if (yy < 0 || yy >= L.h) continue;
            for (int i = 0; i < 5; ++i) {
                const int xx = x + (i - 2) * L.step;
                if (xx < 0 || xx >= L.w) continue;
                const size_t q = (size_t)yy * L.w + xx;
                const float4 cq = in[q];
                if (!finite3(cq)) continue;
                const float4 aq = af[q];
                const float4 nq = nf[q];
                float e = 0.f;
                if constexpr (GUIDED) { // Y of the difference: Y is linear, and close colours subtract exactly
                    if (ic > 0.f) e += fabsf(luma(cp.x - cq.x, cp.y - cq.y, cp.z - cq.z)) * ic;
                } else {
                    if (ic > 0.f) e += ((cp.x - cq.x) * (cp.x - cq.x) + (cp.y - cq.y) * (cp.y - cq.y) + (cp.z - cq.z) * (cp.z - cq.z)) * ic;
                }
                if (L.in > 0.f) e += ((np.x - nq.x) * (np.x - nq.x) + (np.y - nq.y) * (np.y - nq.y) + (np.z - nq.z) * (np.z - nq.z)) * L.in;
                if (L.ia > 0.f) e += ((ap.x - aq.x) * (ap.x - aq.x) + (ap.y - aq.y) * (ap.y - aq.y) + (ap.z - aq.z) * (ap.z - aq.z)) * L.ia;
                if (L.iz > 0.f) {
                    const bool hit_q = isfinite(aq.w);
                    if (hit_p != hit_q) continue;
                    if (hit_p && ap.w != aq.w) e += (ap.w - aq.w) * (ap.w - aq.w) * iz;
                }
                const float wgt = hk[i] * hk[j] * expf(-e);
                sr += wgt * cq.x;
                sg += wgt * cq.y;
                sb += wgt * cq.z;
                sw += wgt;
                if constexpr (GUIDED) sv += wgt * wgt * cq.w;
            }
        }
        // sw >= the centre's own weight h(0)^2 = 0.140625 > 0: every term of the centre's exponent is 0
        rr = sr / sw;
        rg = sg / sw;
        rb = sb / sw;
        if constexpr (GUIDED) rv = sv / (sw * sw);
    }
    if (out_rgb) {
        if (demod) {
            rr *= fmaxf(ap.x, PRT_DN_EPS);
            rg *= fmaxf(ap.y, PRT_DN_EPS);
            rb *= fmaxf(ap.z, PRT_DN_EPS);
            if constexpr (GUIDED) rv *= luma_mod2(ap.x, ap.y, ap.z);
        }
        if constexpr (GUIDED) {
            if (out_var) out_var[p] = rv;
        }
        out_rgb[p * 3] = rr;
        out_rgb[p * 3 + 1] = rg;
        out_rgb[p * 3 + 2] = rb;
    } else {
        out[p] = make_float4(rr, rg, rb, rv);
    }
}

// iterations = 0 of the guided filter: the variance plane, sanitised.
__global__ void k_dn_sane_variance(const float* __restrict__ var, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sane_variance(var[i]);
}

} // namespace

namespace prt {

// Scratch the filter needs: three float4 planes of the features and colour plus a second colour plane (ping-pong).
size_t denoise_scratch_bytes(int w, int h) { return (size_t)w * h * 4 * sizeof(float4); }

// `sigma` = {colour, normal, depth, albedo}; a sigma <= 0 or infinite switches its term off.  iterations >= 1.
// GUIDED: `var` [h][w] comes in with the colour, sigma[0] multiplies the standard deviation and is not halved per level,
// and out_var (may be null) receives the filtered variance.
template <bool GUIDED>
static void launch_levels(int w, int h, const float* rgb, const float* var, const float* albedo, const float* normal,
                          const float* depth, int iterations, int demod, const float sigma[4], void* scratch, float* out,
                          float* out_var, hipStream_t st) {
    const size_t n = (size_t)w * h;
    float4* col0 = static_cast<float4*>(scratch);
    float4* col1 = col0 + n;
    float4* af = col1 + n;
    float4* nf = af + n;
    hipLaunchKernelGGL(k_dn_pack<GUIDED>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rgb, var, albedo, normal, depth, n, demod, col0, af, nf);
    auto inv2 = [](double s) { return (s > 0.0 && s < __builtin_huge_val()) ? (float)std::fmin(1.0 / (s * s), 3.4e38) : 0.f; }; // (finite: 0 * ic = 0)
    DnLevel L;
    L.w = w;
    L.h = h;
    L.in = inv2(sigma[1]);
    L.iz = inv2(sigma[2]);
    L.ia = inv2(sigma[3]);
    L.ic = 0.f;
    L.sc = (GUIDED && sigma[0] > 0.f && sigma[0] < __builtin_huge_valf()) ? sigma[0] : 0.f;
    const dim3 grid((unsigned)((w + PRT_DN_TILE - 1) / PRT_DN_TILE), (unsigned)((h + PRT_DN_TILE - 1) / PRT_DN_TILE));
    for (int i = 0; i < iterations; ++i) {
        L.step = 1 << i;
        if (!GUIDED) L.ic = inv2((double)sigma[0] * std::ldexp(1.0, -i)); // sigma_c 2^-i
        const bool last = i == iterations - 1;
        hipLaunchKernelGGL(k_dn_level<GUIDED>, grid, dim3(PRT_DN_TILE, PRT_DN_TILE), 0, st, L, (i & 1) ? col1 : col0, af, nf,
                           last ? nullptr : ((i & 1) ? col0 : col1), last ? out : nullptr, last ? out_var : nullptr, demod);
    }
}

void launch_denoise(int w, int h, const float* rgb, const float* albedo, const float* normal, const float* depth,
                    int iterations, int demod, const float sigma[4], void* scratch, float* out, hipStream_t st) {
    launch_levels<false>(w, h, rgb, nullptr, albedo, normal, depth, iterations, demod, sigma, scratch, out, nullptr, st);
}

// The guided filter; iterations = 0 only sanitises the variance into out_var (the caller copies the colour).
void launch_denoise_guided(int w, int h, const float* rgb, const float* var, const float* albedo, const float* normal,
                           const float* depth, int iterations, int demod, const float sigma[4], void* scratch, float* out,
                           float* out_var, hipStream_t st) {
    if (iterations == 0) {
        const size_t n = (size_t)w * h;
        if (out_var) hipLaunchKernelGGL(k_dn_sane_variance, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, var, n, out_var);
        return;
    }
    launch_levels<true>(w, h, rgb, var, albedo, normal, depth, iterations, demod, sigma, scratch, out, out_var, st);
}

} // namespace prt
