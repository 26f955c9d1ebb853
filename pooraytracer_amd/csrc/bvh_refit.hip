// bvh_refit.hip — in-place geometry update of a resident scene (prt_scene_refit, include/prt.h): new vertex positions in,
// the intersection records, the tangents and the boxes of the 4-wide tree follow on the GPU; the topology stays.
//
//   k_refit_check    read-only first phase: vertex range test, scene bounds (wave + block reduction, one partial per
//                    block, k_refit_check_final folds them in a fixed order), light triangles compared bit for bit
//   k_refit_tris     one thread per leaf position: the Triangle constructor precompute (scene_setup.cpp,
//                    setup_triangle_geometry) and the DTri / DTriShade derivation of prt_scene_upload on the new vertices,
//                    written straight into the resident records, plus the triangle's fp32 box by the rule of prim_boxes
//   k_prim_boxes     prt_scene_rebuild: the same box rule for every triangle in description order, the device builder's input
//   k_permute_shade  prt_scene_rebuild: the shading records from the old leaf order into the new one (k_invert_order first)
//   k_refit_parents  once per topology: the parent of every node
//   k_refit_boxes    bottom-up over the 64-byte nodes: every thread fills the leaf slots of its own node, then arrives at
//                    the node's counter; the last arriver of a node (its own thread and one per inner child) fills the
//                    node's inner slots from its children and climbs to the parent
//   k_refit_sah      SAH cost of the wide tree (tests/bvh_model.py, sah_cost), reduced like the bounds
//
// fp64 with contraction OFF in this file: the records are meant to be the ones the host computes (x86-64 without fused
// multiply-adds), operation for operation; fp64 division and sqrt are correctly rounded on either side.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "prt_types.h"

#pragma clang fp contract(off)

#include "prt_launch.h"
#include "prt_vec64.h"

namespace prt {

// RefitCheck::flags (the struct, the result of the first phase, is in prt_launch.h)
#define PRT_REFIT_BAD_VERTEX 1u // a coordinate is not finite or beyond 1e18
#define PRT_REFIT_LIGHT_MOVED 2u // a light triangle's vertex differs bitwise from the resident one

namespace {

constexpr unsigned kBlock = 256;
constexpr unsigned kMaxBlocks = 1024; // partials of the two reductions (prt_api.cpp sizes the scratch for it)
constexpr int32_t kUnused = (int32_t)0x80000000;
constexpr uint32_t kNoParent = 0xffffffffu;

__device__ inline V unit(V a) { return scale(a, 1.0 / sqrt(dot(a, a))); }
__device__ inline bool has_nan(V a) { return a.x != a.x || a.y != a.y || a.z != a.z; }
__device__ inline V load3(const double* p) { return {p[0], p[1], p[2]}; }

// scene_setup.cpp, edge_interval
__device__ inline void edge_interval(double a, double b, double& lo, double& hi) {
    lo = (a <= b) ? a : b;
    hi = (a <= b) ? b : a;
    if (hi - lo < 0.0001) {
        lo -= 0.0001 / 2.;
        hi += 0.0001 / 2.;
    }
}
// HostTri::lo / hi of one axis: the union of the two padded edge boxes (Triangle.cpp:94-99)
__device__ inline void tri_interval(double v0, double v1, double v2, double& lo, double& hi) {
    double l0, h0, l1, h1;
    edge_interval(v0, v1, l0, h0);
    edge_interval(v0, v2, l1, h1);
    lo = l0 <= l1 ? l0 : l1;
    hi = h0 >= h1 ? h0 : h1;
}

// bvh_build.cpp, round_down / round_up
__device__ inline float round_down(double v) {
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, -INFINITY);
    return f;
}
__device__ inline float round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

__device__ inline double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// (a butterfly like the two above, the sum in every lane: prt_wave.h's wave_sum, valid in lane 0 only, gives k_refit_sah the
// same bits through other vector instructions, so this one stays)
__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// r[0..2] min, r[3..6] max over the block; valid in thread 0 afterwards
__device__ inline void block_bounds(double r[7]) {
    __shared__ double sh[kBlock / 64][7];
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (int k = 0; k < 7; ++k) {
        r[k] = k < 3 ? wave_min(r[k]) : wave_max(r[k]);
        if (lane == 0) sh[w][k] = r[k];
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (unsigned j = 1; j < kBlock / 64; ++j)
            for (int k = 0; k < 7; ++k) r[k] = k < 3 ? fmin(r[k], sh[j][k]) : fmax(r[k], sh[j][k]);
}

__global__ void __launch_bounds__(kBlock) k_refit_check(const double* __restrict__ verts, uint32_t n,
                                                        const DLightTriT<double>* __restrict__ ltris, uint32_t n_lights,
                                                        RefitCheck* __restrict__ partial, const double* __restrict__ normals,
                                                        double* __restrict__ gather_v, double* __restrict__ gather_n) {
    const double inf = INFINITY;
    double r[7] = {inf, inf, inf, -inf, -inf, -inf, 1.0};
    uint32_t flags = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const double* p = verts + (size_t)t * 9;
        double v[9];
        for (int k = 0; k < 9; ++k) {
            v[k] = p[k];
            if (!(fabs(v[k]) <= 1e18)) flags |= PRT_REFIT_BAD_VERTEX;
        }
        for (int a = 0; a < 3; ++a) {
            double lo, hi;
            tri_interval(v[a], v[3 + a], v[6 + a], lo, hi);
            r[a] = fmin(r[a], lo);
            r[3 + a] = fmax(r[3 + a], hi);
            r[6] = fmax(r[6], fmax(fabs(lo), fabs(hi)));
        }
    }
    // emitters in place: does every light triangle still have the vertices it was uploaded with, bit for bit?  (Without
    // prt_scene_set_dynamic_lights a moved one refuses the call; with it, the new vertices - and vertex normals - of every
    // light triangle are gathered here, in resident CDF order, for the host's light tree: k_light_gather, folded into this
    // loop, which reads these 72 bytes anyway.)
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n_lights; l += stride) {
        const DLightTriT<double>& L = ltris[l];
        const uint32_t prim = (uint32_t)L.prim;
        if (prim >= n) {
            flags |= PRT_REFIT_LIGHT_MOVED;
            continue;
        }
        const unsigned long long* nv = reinterpret_cast<const unsigned long long*>(verts + (size_t)prim * 9);
        if (gather_v)
            for (int k = 0; k < 9; ++k) gather_v[(size_t)l * 9 + k] = verts[(size_t)prim * 9 + k];
        if (gather_n)
            for (int k = 0; k < 9; ++k) gather_n[(size_t)l * 9 + k] = normals[(size_t)prim * 9 + k];
        for (int k = 0; k < 3; ++k)
            if (nv[k] != (unsigned long long)__double_as_longlong(L.v0[k]) || nv[3 + k] != (unsigned long long)__double_as_longlong(L.v1[k]) ||
                nv[6 + k] != (unsigned long long)__double_as_longlong(L.v2[k]))
                flags |= PRT_REFIT_LIGHT_MOVED;
    }
    __shared__ uint32_t sh_flags;
    if (threadIdx.x == 0) sh_flags = 0;
    __syncthreads();
    if (flags) atomicOr(&sh_flags, flags);
    block_bounds(r); // (its barrier also orders the flags)
    if (threadIdx.x == 0) {
        RefitCheck o;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = r[a];
            o.hi[a] = r[3 + a];
        }
        o.scale = r[6];
        o.flags = sh_flags;
        o.pad_ = 0;
        partial[blockIdx.x] = o;
    }
}

__global__ void __launch_bounds__(kBlock) k_refit_check_final(const RefitCheck* __restrict__ partial, uint32_t nb,
                                                              RefitCheck* __restrict__ out) {
    const double inf = INFINITY;
    double r[7] = {inf, inf, inf, -inf, -inf, -inf, 1.0};
    uint32_t flags = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += kBlock) {
        const RefitCheck p = partial[b];
        for (int a = 0; a < 3; ++a) {
            r[a] = fmin(r[a], p.lo[a]);
            r[3 + a] = fmax(r[3 + a], p.hi[a]);
        }
        r[6] = fmax(r[6], p.scale);
        flags |= p.flags;
    }
    __shared__ uint32_t sh_flags;
    if (threadIdx.x == 0) sh_flags = 0;
    __syncthreads();
    if (flags) atomicOr(&sh_flags, flags);
    block_bounds(r);
    if (threadIdx.x == 0) {
        RefitCheck o;
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = r[a];
            o.hi[a] = r[3 + a];
        }
        o.scale = r[6];
        o.flags = sh_flags;
        o.pad_ = 0;
        *out = o;
    }
}

struct RefitFrame { // prim_boxes' numbers for this refit, computed on the host from the first phase's bounds
    double origin[3]; // the fp32 grid origin, widened
    double delta;     // 1e-9 extent + 256 eps scale
};

// the triangle's fp32 box relative to the grid origin (bvh_build.cpp, prim_boxes): b[0..2] lo, b[3..5] hi
__device__ inline void tri_box(V p0, V p1, V p2, const RefitFrame& F, float* __restrict__ b) {
    const double c[3][3] = {{p0.x, p1.x, p2.x}, {p0.y, p1.y, p2.y}, {p0.z, p1.z, p2.z}};
    for (int a = 0; a < 3; ++a) {
        double lo, hi;
        tri_interval(c[a][0], c[a][1], c[a][2], lo, hi);
        b[a] = round_down((lo - F.delta) - F.origin[a]);
        b[3 + a] = round_up((hi + F.delta) - F.origin[a]);
    }
}

__global__ void __launch_bounds__(kBlock) k_refit_tris(const double* __restrict__ verts, const double* __restrict__ normals,
                                                       const uint32_t* __restrict__ order, uint32_t n, char* __restrict__ tris,
                                                       uint32_t tri_stride, DTriShadeT<double>* __restrict__ shade,
                                                       float* __restrict__ tbox, RefitFrame F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = order[i];
    if (t >= n) return; // (a permutation by construction; never index out of the caller's buffer)
    const double* pv = verts + (size_t)t * 9;
    const V p0 = load3(pv), p1 = load3(pv + 3), p2 = load3(pv + 6);
    // Triangle::Triangle (Triangle.cpp:11-53), as scene_setup.cpp setup_triangle_geometry evaluates it
    const V e0 = sub(p1, p0), e1 = sub(p2, p0);
    const V nrm = cross(e0, e1);
    V nn = unit(nrm);
    if (has_nan(nn)) { // degenerate face: vertex-normal fallback, then +z
        V s{0.0, 0.0, 0.0};
        if (normals) {
            const double* pn = normals + (size_t)t * 9;
            s = add(add(load3(pn), load3(pn + 3)), load3(pn + 6));
        }
        nn = unit(s);
        if (has_nan(nn)) nn = V{0.0, 0.0, 1.0};
    }
    DTriShadeT<double>& S = shade[i];
    const double du0 = S.uv1[0] - S.uv0[0], dv0 = S.uv1[1] - S.uv0[1];
    const double du1 = S.uv2[0] - S.uv0[0], dv1 = S.uv2[1] - S.uv0[1];
    const double f = 1.0 / (du0 * dv1 - du1 * dv0);
    V tg{f * (dv1 * e0.x - dv0 * e1.x), f * (dv1 * e0.y - dv0 * e1.y), f * (dv1 * e0.z - dv0 * e1.z)};
    tg = unit(tg);
    if (has_nan(tg)) {
        const V helper = (fabs(nn.x) < (double)0.9f) ? V{1, 0, 0} : V{0, 1, 0};
        tg = unit(cross(nn, helper));
    }
    const double nn2 = dot(nrm, nrm);
    const V w{nrm.x / nn2, nrm.y / nn2, nrm.z / nn2};
    // the intersection record (prt_scene_upload): A = e1 x w, B = w x e0
    double rec[12];
    rec[0] = nn.x;
    rec[1] = nn.y;
    rec[2] = nn.z;
    rec[3] = dot(nn, p0);
    rec[4] = e1.y * w.z - w.y * e1.z;
    rec[5] = e1.z * w.x - w.z * e1.x;
    rec[6] = e1.x * w.y - w.x * e1.y;
    rec[8] = w.y * e0.z - e0.y * w.z;
    rec[9] = w.z * e0.x - e0.z * w.x;
    rec[10] = w.x * e0.y - e0.x * w.y;
    rec[7] = p0.x * rec[4] + p0.y * rec[5] + p0.z * rec[6];
    rec[11] = p0.x * rec[8] + p0.y * rec[9] + p0.z * rec[10];
    double2* out = reinterpret_cast<double2*>(tris + (size_t)i * tri_stride);
    for (int k = 0; k < 6; ++k) out[k] = make_double2(rec[2 * k], rec[2 * k + 1]);
    S.tangent[0] = tg.x;
    S.tangent[1] = tg.y;
    S.tangent[2] = tg.z;
    tri_box(p0, p1, p2, F, tbox + (size_t)i * 6);
}

// The builder's input: the PrimBox of every triangle in DESCRIPTION order (prt_scene_rebuild).
__global__ void __launch_bounds__(kBlock) k_prim_boxes(const double* __restrict__ verts, uint32_t n, float* __restrict__ boxes,
                                                       RefitFrame F) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double* pv = verts + (size_t)t * 9;
    tri_box(load3(pv), load3(pv + 3), load3(pv + 6), F, boxes + (size_t)t * 6);
}

// inv[order[i]] = i: where the triangle of description index t sits in a leaf order
__global__ void __launch_bounds__(kBlock) k_invert_order(const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = order[i];
    if (t < n) inv[t] = i;
}

// shade_new[j] = shade_old[inv_old[new_order[j]]], out of place, 16 bytes per lane (bvh_build_gpu.hip, k_gather_tris)
__global__ void __launch_bounds__(kBlock) k_permute_shade(const uint4* __restrict__ shade_old, const uint32_t* __restrict__ inv_old,
                                                          const uint32_t* __restrict__ new_order, uint32_t n,
                                                          uint4* __restrict__ shade_new) {
    constexpr uint32_t SP = sizeof(DTriShadeT<double>) / 16;
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = (uint32_t)(x / SP), c = (uint32_t)(x % SP);
    if (j >= n) return;
    const uint32_t t = new_order[j];
    if (t >= n) return; // (permutations by construction; never index out of a buffer)
    const uint32_t src = inv_old[t];
    if (src >= n) return;
    shade_new[(uint64_t)j * SP + c] = shade_old[(uint64_t)src * SP + c];
}

__global__ void __launch_bounds__(kBlock) k_refit_parents(const DNode* __restrict__ nodes, uint32_t n_nodes,
                                                          uint32_t* __restrict__ parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    if (i == 0) parent[0] = kNoParent;
    for (int s = 0; s < 4; ++s) {
        const int32_t r = nodes[i].ref[s];
        if (r > 0 && (uint32_t)r < n_nodes) parent[r] = i; // (the root is nobody's child)
    }
}

struct RefitGrid {
    float step[3]; // the boxes are relative to the grid origin: the grid starts at 0 in their coordinates
};
// the builders' outward quantisation (bvh_build.cpp qlo / qhi) with g0 = 0
__device__ inline uint32_t quant_lo(double gs, float v) {
    double q = floor((double)v / gs);
    q = fmin(65535.0, fmax(0.0, q));
    while (q > 0 && q * gs > (double)v) q -= 1;
    return (uint32_t)q;
}
__device__ inline uint32_t quant_hi(double gs, float v) {
    double q = ceil((double)v / gs);
    q = fmin(65535.0, fmax(0.0, q));
    while (q < 65535 && q * gs < (double)v) q += 1;
    return (uint32_t)q;
}

__device__ inline int inner_children(const int32_t ref[4]) {
    int k = 0;
    for (int s = 0; s < 4; ++s) k += ref[s] >= 0; // (an unused slot's ref is negative)
    return k;
}

// `nodes` is read and written across workgroups inside the launch: no const, no __restrict__ (vector loads behind the
// acquire, never the scalar cache).  cnt[] is zero at the launch.
__global__ void __launch_bounds__(kBlock) k_refit_boxes(DNode* nodes, uint32_t n_nodes, const uint32_t* __restrict__ parent,
                                                        uint32_t* cnt, const float* __restrict__ tbox, uint32_t n_tris,
                                                        RefitGrid G) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    int32_t ref[4];
    {
        const int4 r = *reinterpret_cast<const int4*>(nodes[i].ref);
        ref[0] = r.x; ref[1] = r.y; ref[2] = r.z; ref[3] = r.w;
    }
    // leaf slots: the union of the leaf's 1-4 triangle boxes, quantised outward onto the new grid
    for (int s = 0; s < 4; ++s) {
        const int32_t r = ref[s];
        if (r >= 0 || r == kUnused) continue;
        const uint32_t enc = ~(uint32_t)r, first = enc >> 3, count = (enc & 7u) + 1u;
        if ((uint64_t)first + count > n_tris) continue;
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = INFINITY;
            hi[a] = -INFINITY;
        }
        for (uint32_t k = first; k < first + count; ++k) {
            const float* b = tbox + (size_t)k * 6;
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], b[a]);
                hi[a] = fmaxf(hi[a], b[3 + a]);
            }
        }
        nodes[i].bx[s] = quant_lo((double)G.step[0], lo[0]) | (quant_hi((double)G.step[0], hi[0]) << 16);
        nodes[i].by[s] = quant_lo((double)G.step[1], lo[1]) | (quant_hi((double)G.step[1], hi[1]) << 16);
        nodes[i].bz[s] = quant_lo((double)G.step[2], lo[2]) | (quant_hi((double)G.step[2], hi[2]) << 16);
    }
    // Climb.  A node is complete when its own thread (leaf slots) and the last arriver of each inner child have arrived:
    // 1 + inner children arrivals.  Every arrival releases what the thread wrote (agent scope: the XCDs' L2s are not
    // coherent with each other), the last one acquires before it reads the children.
    uint32_t cur = i;
    int kin = inner_children(ref);
    for (;;) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        // (the fence's own wait for the stores above must not depend on the compiler keeping it in front of a returning atomic)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(&cnt[cur], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != (uint32_t)kin) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // inner slots: the integer min / max of the child's used slots (quantising is idempotent on one grid)
        for (int s = 0; s < 4; ++s) {
            const int32_t r = ref[s];
            if (r < 0 || (uint32_t)r >= n_nodes) continue;
            const DNode* c = &nodes[r];
            const uint4 cx = *reinterpret_cast<const uint4*>(c->bx), cy = *reinterpret_cast<const uint4*>(c->by),
                        cz = *reinterpret_cast<const uint4*>(c->bz);
            const int4 cr = *reinterpret_cast<const int4*>(c->ref);
            const uint32_t bx[4] = {cx.x, cx.y, cx.z, cx.w}, by[4] = {cy.x, cy.y, cy.z, cy.w}, bz[4] = {cz.x, cz.y, cz.z, cz.w};
            const int32_t rr[4] = {cr.x, cr.y, cr.z, cr.w};
            uint32_t lo[3] = {0xffffu, 0xffffu, 0xffffu}, hi[3] = {0u, 0u, 0u};
            for (int k = 0; k < 4; ++k) {
                if (rr[k] == kUnused) continue;
                lo[0] = min(lo[0], bx[k] & 0xffffu); hi[0] = max(hi[0], bx[k] >> 16);
                lo[1] = min(lo[1], by[k] & 0xffffu); hi[1] = max(hi[1], by[k] >> 16);
                lo[2] = min(lo[2], bz[k] & 0xffffu); hi[2] = max(hi[2], bz[k] >> 16);
            }
            nodes[cur].bx[s] = lo[0] | (hi[0] << 16);
            nodes[cur].by[s] = lo[1] | (hi[1] << 16);
            nodes[cur].bz[s] = lo[2] | (hi[2] << 16);
        }
        const uint32_t p = parent[cur];
        if (p == kNoParent || p >= n_nodes) break;
        cur = p;
        const int4 r = *reinterpret_cast<const int4*>(nodes[cur].ref);
        ref[0] = r.x; ref[1] = r.y; ref[2] = r.z; ref[3] = r.w;
        kin = inner_children(ref);
    }
}

struct SahGrid {
    float origin[3], step[3];
};
// tests/bvh_model.py sah_cost: per used slot the half area of its dequantised box, times 1.0 (inner child: a node visit)
// or 1.5 x triangles (leaf); partial[b] = block b's sum
__global__ void __launch_bounds__(kBlock) k_refit_sah(const DNode* __restrict__ nodes, uint32_t n_nodes, SahGrid G,
                                                      double* __restrict__ partial) {
    double sum = 0.0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x) {
        const DNode nd = nodes[i];
        for (int s = 0; s < 4; ++s) {
            if (nd.ref[s] == kUnused) continue;
            const uint32_t q[3] = {nd.bx[s], nd.by[s], nd.bz[s]};
            double e[3];
            for (int a = 0; a < 3; ++a) {
                const double lo = (double)G.origin[a] + (double)(q[a] & 0xffffu) * (double)G.step[a];
                const double hi = (double)G.origin[a] + (double)(q[a] >> 16) * (double)G.step[a];
                e[a] = fmax(hi - lo, 0.0);
            }
            const double area = e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
            sum += nd.ref[s] >= 0 ? 1.0 * area : 1.5 * (double)((~(uint32_t)nd.ref[s] & 7u) + 1u) * area;
        }
    }
    __shared__ double sh[kBlock / 64];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned j = 1; j < kBlock / 64; ++j) sum += sh[j];
        partial[blockIdx.x] = sum;
    }
}
__global__ void k_refit_sah_final(const DNode* __restrict__ nodes, SahGrid G, const double* __restrict__ partial, uint32_t nb,
                                  double* __restrict__ out) {
    double sum = 0.0;
    for (uint32_t b = 0; b < nb; ++b) sum += partial[b];
    const DNode nd = nodes[0];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int s = 0; s < 4; ++s) {
        if (nd.ref[s] == kUnused) continue;
        const uint32_t q[3] = {nd.bx[s], nd.by[s], nd.bz[s]};
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], (double)G.origin[a] + (double)(q[a] & 0xffffu) * (double)G.step[a]);
            hi[a] = fmax(hi[a], (double)G.origin[a] + (double)(q[a] >> 16) * (double)G.step[a]);
        }
    }
    const double e[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double root = fmax(e[0] * e[1] + e[1] * e[2] + e[2] * e[0], 1e-300);
    *out = 1.0 + sum / root;
}

inline unsigned blocks_for(uint64_t items) { return (unsigned)std::max<uint64_t>(1, (items + kBlock - 1) / kBlock); }

} // namespace

// bytes of the reductions' partials (one buffer serves both)
size_t refit_scratch_bytes() { return (size_t)kMaxBlocks * sizeof(RefitCheck); }

// d_gather_v / d_gather_n: null, or room for 9 doubles per light triangle (the new vertices; the new vertex normals, only
// with d_normals): filled in the order of d_ltris
void launch_refit_check(const double* d_verts, uint32_t n, const DLightTriT<double>* d_ltris, uint32_t n_lights, void* d_scratch,
                        RefitCheck* d_out, hipStream_t st, const double* d_normals, double* d_gather_v, double* d_gather_n) {
    const unsigned nb = std::min(kMaxBlocks, blocks_for(std::max(n, n_lights)));
    k_refit_check<<<nb, kBlock, 0, st>>>(d_verts, n, d_ltris, n_lights, static_cast<RefitCheck*>(d_scratch), d_normals, d_gather_v,
                                         d_normals ? d_gather_n : nullptr);
    k_refit_check_final<<<1, kBlock, 0, st>>>(static_cast<const RefitCheck*>(d_scratch), nb, d_out);
}

void launch_refit_tris(const double* d_verts, const double* d_normals, const uint32_t* d_order, uint32_t n, void* d_tris,
                       uint32_t tri_stride, DTriShadeT<double>* d_shade, float* d_tbox, const double origin[3], double delta,
                       hipStream_t st) {
    if (!n) return;
    RefitFrame F;
    for (int a = 0; a < 3; ++a) F.origin[a] = origin[a];
    F.delta = delta;
    k_refit_tris<<<blocks_for(n), kBlock, 0, st>>>(d_verts, d_normals, d_order, n, static_cast<char*>(d_tris), tri_stride, d_shade,
                                                   d_tbox, F);
}

// d_boxes: n PrimBox (prt_host.h: float lo[3], hi[3]) in description order
void launch_prim_boxes(const double* d_verts, uint32_t n, float* d_boxes, const double origin[3], double delta, hipStream_t st) {
    if (!n) return;
    RefitFrame F;
    for (int a = 0; a < 3; ++a) F.origin[a] = origin[a];
    F.delta = delta;
    k_prim_boxes<<<blocks_for(n), kBlock, 0, st>>>(d_verts, n, d_boxes, F);
}

// The shading records from the leaf order `d_old_order` into the leaf order `d_new_order`; d_inv: n entries of scratch.
void launch_permute_shade(const DTriShadeT<double>* d_shade_old, const uint32_t* d_old_order, const uint32_t* d_new_order,
                          uint32_t n, uint32_t* d_inv, DTriShadeT<double>* d_shade_new, hipStream_t st) {
    static_assert(sizeof(DTriShadeT<double>) % 16 == 0, "records are moved in 16-byte pieces");
    if (!n) return;
    k_invert_order<<<blocks_for(n), kBlock, 0, st>>>(d_old_order, n, d_inv);
    k_permute_shade<<<blocks_for((uint64_t)n * (sizeof(DTriShadeT<double>) / 16)), kBlock, 0, st>>>(
        reinterpret_cast<const uint4*>(d_shade_old), d_inv, d_new_order, n, reinterpret_cast<uint4*>(d_shade_new));
}

void launch_refit_parents(const DNode* d_nodes, uint32_t n_nodes, uint32_t* d_parent, hipStream_t st) {
    k_refit_parents<<<blocks_for(n_nodes), kBlock, 0, st>>>(d_nodes, n_nodes, d_parent);
}

// d_cnt: n_nodes counters, zeroed here (rounded up to 16 bytes: the caller allocates that much)
hipError_t launch_refit_boxes(DNode* d_nodes, uint32_t n_nodes, const uint32_t* d_parent, uint32_t* d_cnt, const float* d_tbox,
                              uint32_t n_tris, const float step[3], hipStream_t st) {
    const hipError_t e = hipMemsetAsync(d_cnt, 0, (((size_t)n_nodes * sizeof(uint32_t)) + 15) & ~(size_t)15, st);
    if (e != hipSuccess) return e;
    RefitGrid G;
    for (int a = 0; a < 3; ++a) G.step[a] = step[a];
    k_refit_boxes<<<blocks_for(n_nodes), kBlock, 0, st>>>(d_nodes, n_nodes, d_parent, d_cnt, d_tbox, n_tris, G);
    return hipSuccess;
}

void launch_refit_sah(const DNode* d_nodes, uint32_t n_nodes, const float origin[3], const float step[3], void* d_scratch,
                      double* d_out, hipStream_t st) {
    SahGrid G;
    for (int a = 0; a < 3; ++a) {
        G.origin[a] = origin[a];
        G.step[a] = step[a];
    }
    const unsigned nb = std::min(kMaxBlocks, blocks_for(n_nodes));
    k_refit_sah<<<nb, kBlock, 0, st>>>(d_nodes, n_nodes, G, static_cast<double*>(d_scratch));
    k_refit_sah_final<<<1, 1, 0, st>>>(d_nodes, G, static_cast<const double*>(d_scratch), nb, d_out);
}

} // namespace prt
