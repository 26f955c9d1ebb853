// closest_point.hip — K6: batched closest-point queries against the resident 4-wide BVH (prt_closest_point, include/prt.h).
//
//   k_gather_corners   one thread per leaf position: the three fp64 corners of the triangle that sits there, and its index
//                      in description order, into the scene's DTriCorners table (prt_types.h) — from positions in
//                      description order through the leaf order, for every path that moves the resident geometry
//   k_closest_point    one lane per query: a best-first descent.  A node visit is the ray traversal's (four 16-byte loads,
//                      four fp32 box tests, a 5-exchange sort, nearest child next, the others pushed far to near on the
//                      lane's LDS stack) with the slab test replaced by a lower bound of the squared point-box distance; a
//                      leaf runs Ericson's point-triangle routine in fp64 on its 1-4 triangles and keeps the smaller
//                      (d2, prim).  A subtree is skipped only when its bound is STRICTLY greater than the best d2: the
//                      answer is the minimum of (d2, prim) over ALL triangles, whatever the tree (include/prt.h, contract 3).
//
// Stack.  An entry is 8 bytes: the ref and the bound it was pushed with, in two lane-strided word arrays (entry e of lane l
// at word e*64+l of each: conflict-free, as in prt_device.h).  The bound lets a pop drop an entry the best distance has
// overtaken since the push without fetching its node — or, for a leaf, without its fp64 triangle tests; with 4-byte
// entries every pushed entry costs a node fetch (a leaf: up to four tests) to find that out.  A visit pushes at most three
// entries, so the builders' bound on the ray traversal's stack (tree_stack_need <= PRT_STACK_DEPTH) holds here unchanged;
// the launch sizes its dynamic LDS from what the resident tree needs (2 KB per entry per block).  The counting
// instantiation reports the dropped entries (DESIGN.md §7 has the figures that decided this).
// Schedule.  Persistent waves that refill finished lanes, as K1 does: queries differ in work by two orders of magnitude
// where the mesh has centres of curvature (a point inside a tessellated ball is about as far from thousands of triangles
// as from the nearest), and in the plain one-lane-per-query form every wave lasted as long as its slowest lane.
//
// fp64 and fp32 with contraction OFF in this file: d2, alpha and beta are the contract's values operation for operation
// (tests/closest_point_model.py evaluates the same expressions in numpy), and the bound below is derived for individually
// rounded operations.  fp64 division and sqrt are correctly rounded.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/prt.h"
#include "prt_types.h"

#pragma clang fp contract(off)

#include "prt_launch.h"
#include "prt_vec64.h"
#include "prt_wave.h"

namespace prt {
namespace {

constexpr uint32_t kUnusedRef = 0x80000000u;
constexpr uint32_t kNoKey = 0xffffffffu;

// v0 + alpha (v1 - v0) + beta (v2 - v0), per component ((v0 + alpha ab) + beta ac): contract 2's `point`
__device__ __forceinline__ V bary_point(V a, V ab, V ac, double al, double be) {
    return {a.x + al * ab.x + be * ac.x, a.y + al * ab.y + be * ac.y, a.z + al * ab.z + be * ac.z};
}

// Ericson, Real-Time Collision Detection 5.1.5 (ClosestPtPointTriangle): the Voronoi region of p decides the feature, the
// barycentrics follow from the region's own projection.  feature: 0 face, 1/2/3 edge v0v1 / v1v2 / v2v0, 4/5/6 vertex.
// A degenerate triangle divides 0 by 0 somewhere: its NaN d2 fails every comparison and it is never a candidate.
__device__ __forceinline__ void point_triangle(V p, V a, V b, V c, double& al, double& be, int32_t& feature) {
    const V ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) {
        al = 0.0, be = 0.0, feature = 4;
        return;
    }
    const V bp = sub(p, b);
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) {
        al = 1.0, be = 0.0, feature = 5;
        return;
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        al = d1 / (d1 - d3), be = 0.0, feature = 1;
        return;
    }
    const V cp = sub(p, c);
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) {
        al = 0.0, be = 1.0, feature = 6;
        return;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        al = 0.0, be = d2 / (d2 - d6), feature = 3;
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        be = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        al = 1.0 - be;
        feature = 2;
        return;
    }
    const double denom = 1.0 / (va + vb + vc);
    al = vb * denom;
    be = vc * denom;
    feature = 0;
}

// Per-query constants of the box bound, one set per axis.
struct BoundAxis {
    float r;   // the query coordinate RELATIVE TO THE GRID ORIGIN: subtracted in fp64, rounded to fp32 once
    float gs;  // the grid step
    float pad; // (|r| + E) * 2^-21
};
// Lower bound of the squared distance from the query to a child box, from its three packed (lo | hi << 16) grid ranges.
//
// The box is [g0 + qlo gs, g0 + qhi gs] per axis in real arithmetic (what the builders round OUTWARD to, prt_types.h), the
// point is r* = p - g0 relative to the grid origin, and the exact per-axis distance is d* = max(qlo gs - r*, r* - qhi gs, 0).
// Taking the point relative to the grid origin makes every rounding scale with |r| + E (E = the grid's largest extent,
// DScene::slab_scale, >= every q gs), not with where the scene sits in the world — slab_axis's argument (prt_device.h).
// Roundings of the computed d, each at most 2^-24 relative:  r = (float)(p - g0): 2^-24 |r| (the fp64 subtraction adds
// 2^-53);  b = (float)q * gs, q exact: 2^-24 E;  the subtraction b - r or r - b: 2^-24 (|r| + E).  Together
// |d - d*| <= 2^-23 (|r| + E) (1 + 2^-23).  The pad 2^-21 (|r| + E) is four times that: d' = max(d - pad, 0) <= d* (1 + 2^-24),
// the last factor being the rounding of d - pad itself.  d' is clamped to 1e18 so that no square overflows (a smaller
// bound is still a bound).  lb = (d'x^2 + d'y^2 + d'z^2) has five more roundings: lb <= |d*|^2 (1 + 2^-24)^7; the final
// factor 1 - 2^-20, with its own rounding, leaves lb <= |d*|^2 (1 - 2^-21).  (Nothing here underflows for a grid of
// extent >= 2^-40: a nonzero d' is at least ~2^-22 E.)
// That margin also covers the fp64 side: d2 = |p - point|^2 carries a relative rounding of ~2^-50, and `point` — a
// combination of the corners with weights in [0, 1] up to rounding — lies within a few fp64 ulps of the coordinates of the
// triangle, which both builders and the refit keep inside the leaf's box by a margin of 1e-9 extents + 256 ulp
// (prim_boxes): the distance from p to the box is a lower bound of |p - point|, and lb <= computed d2 of every
// triangle below the box.  A NaN coordinate gives d = 0 (fmaxf drops it): nothing is culled, the descent is a finite scan.
__device__ __forceinline__ float axis_gap(uint32_t range, const BoundAxis& a) {
    const float lo = (float)(range & 0xffffu) * a.gs, hi = (float)(range >> 16) * a.gs;
    const float d = fmaxf(fmaxf(lo - a.r, a.r - hi), 0.f);
    return fminf(fmaxf(d - a.pad, 0.f), 1e18f);
}
__device__ __forceinline__ float box_bound(uint32_t x, uint32_t y, uint32_t z, const BoundAxis& ax, const BoundAxis& ay,
                                           const BoundAxis& az) {
    const float dx = axis_gap(x, ax), dy = axis_gap(y, ay), dz = axis_gap(z, az);
    return (dx * dx + dy * dy + dz * dz) * 0.99999905f; // 1 - 2^-20
}
// fp64 -> fp32, never below: the best d2 as the bounds are compared with it (lb > up(best) implies lb > best)
__device__ __forceinline__ float f32_above(double x) {
    const float f = (float)x;
    return f + fabsf(f) * 2.4e-7f;
}

struct ClosestArgs {
    const DNode* nodes;
    const DTriCorners* corners;
    const PrtPointQuery* q;
    PrtClosestPoint* out;
    DCounters* ctr;
    size_t n;
    uint32_t n_tris;
    int32_t stack_depth;
    float g0[3], gs[3], E;
};
struct SignedArgs : ClosestArgs { // the SIGNED instantiations' (the others keep their kernel arguments)
    const uint32_t* slot; // DSignedTables::slot / normal (prt_launch.h)
    const double* normal;
    uint32_t n_normals; // edges + vertices
};

// REFILL: persistent waves; a lane takes its next query the moment its descent ends (a wave-local pool refilled by one
// atomic per PRT_K6_CHUNK queries), so that no lane waits for the slowest query of its wave.  !REFILL: the plain form, one
// lane per query and one block per 256 consecutive queries - kept as the yardstick the schedule was chosen against
// (developer hook PRT_TUNE_CLOSEST_PLAIN).  Either way a record is a pure function of its query.
// LDS decides the occupancy: two blocks per CU at the builders' stack bound (40 entries: 80 KB of stacks), up to four for
// the shallow trees of small scenes, which is what the 106 registers per lane (no scratch) leave room for.
// SIGNED (prt_signed_distance): the write-out also takes the sign of dot(N, p - point), N the pseudonormal of the nearest
// feature - the descent is the same code, and at the write-out the lane already holds p, point, the feature and the prim:
// one id load and one 24-byte load per query, and only where the feature is an edge or a vertex.
template <bool COUNT, bool REFILL, bool SIGNED = false>
__global__ __launch_bounds__(PRT_BLOCK, 2) void k_closest_point(std::conditional_t<SIGNED, SignedArgs, ClosestArgs> A) {
    extern __shared__ uint32_t s_stack[]; // [2][PRT_BLOCK / 64][stack_depth][64]: refs, then bounds
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* stk_ref = s_stack + (size_t)(wave * A.stack_depth) * 64 + lane;
    float* stk_lb = reinterpret_cast<float*>(s_stack + (size_t)(PRT_BLOCK / 64) * A.stack_depth * 64) + (size_t)(wave * A.stack_depth) * 64 + lane;
    V p{0, 0, 0};
    BoundAxis ax{0.f, A.gs[0], 0.f}, ay{0.f, A.gs[1], 0.f}, az{0.f, A.gs[2], 0.f};
    // the best candidate so far: (d2, prim) with its leaf position; prim = INT32_MAX: none yet, and best_d2 is the radius
    double best_d2 = 0.0, best_al = 0.0, best_be = 0.0;
    int32_t best_prim = INT32_MAX, best_feature = -1;
    uint32_t best_at = 0;
    float bestf = 0.f;
    uint32_t n_nodes = 0, n_tests = 0, n_drop_inner = 0, n_drop_leaf = 0;
    int32_t sp = 0;
    uint32_t cur = kUnusedRef; // an inner node, a leaf ref, or kUnusedRef: nothing left
    size_t qi = 0;             // the query this lane is answering
    bool have = false, active = false;
    WavePool<PRT_K6_CHUNK> pool; // the wave's queries (prt_wave.h); !REFILL uses only its `exhausted`
    for (;;) {
        if (!active && have) { // the lane's descent has ended: its record
            double4 o0 = make_double4(__builtin_huge_val(), 0.0, 0.0, 0.0), o1 = make_double4(0.0, 0.0, 0.0, 0.0);
            int32_t prim = -1, feature = -1, side = 0, sign = 0; // sign: PrtClosestPoint.reserved = 0 unless SIGNED
            if (best_prim != INT32_MAX) {
                const Corners t = load_corners(A.corners + best_at);
                const V a = t.v0, ab = sub(t.v1, a), ac = sub(t.v2, a);
                const V pt = bary_point(a, ab, ac, best_al, best_be); // the same expression on the same values as in the test
                const double s = dot(cross(ab, ac), sub(p, pt));
                o0 = make_double4(sqrt(best_d2), pt.x, pt.y, pt.z);
                o1.x = best_al, o1.y = best_be;
                prim = best_prim, feature = best_feature;
                side = s > 0.0 ? 1 : (s < 0.0 ? -1 : 0);
                if constexpr (SIGNED) {
                    sign = side; // a face: N = cross(v1 - v0, v2 - v0), s is side's expression
                    if (feature != 0) {
                        sign = 0;
                        // (prim < n_tris and id < n_normals by construction; never read out of the tables)
                        const uint32_t id = (uint32_t)prim < A.n_tris ? A.slot[(size_t)(uint32_t)prim * 6 + (uint32_t)(feature - 1)] : kNoKey;
                        if (id < A.n_normals) { // kNoKey: a slot without an id
                            const double* nrm = A.normal + (size_t)id * 3;
                            const double sn = dot(V{nrm[0], nrm[1], nrm[2]}, sub(p, pt));
                            sign = sn > 0.0 ? 1 : (sn < 0.0 ? -1 : 0);
                        }
                    }
                    if (sign < 0) o0.x = -o0.x;
                }
            }
            o1.z = __longlong_as_double((long long)(((unsigned long long)(uint32_t)feature << 32) | (uint32_t)prim));
            o1.w = SIGNED ? __longlong_as_double((long long)(((unsigned long long)(uint32_t)sign << 32) | (uint32_t)side))
                          : __longlong_as_double((long long)(unsigned long long)(uint32_t)side); // reserved = 0
            double4* o = reinterpret_cast<double4*>(A.out + qi);
            o[0] = o0;
            o[1] = o1;
            have = false;
        }
        bool take = false;
        size_t next = 0;
        if (REFILL) {
            const unsigned long long need = __ballot(!active);
            if (pool.wants(need)) {
                pool.refill(need, lane, A.n, &A.ctr->next_item);
                if (!pool.exhausted && !active) {
                    const unsigned long long idx = pool.index(need, lane);
                    take = idx < pool.end;
                    next = (size_t)idx;
                }
                pool.advance(need);
            }
        } else if (!pool.exhausted) {
            next = (size_t)blockIdx.x * PRT_BLOCK + threadIdx.x;
            take = next < A.n;
            pool.exhausted = true;
        }
        if (take) { // the lane starts query `next`
            const PrtPointQuery* q = A.q + next;
            p = V{q->p[0], q->p[1], q->p[2]};
            const double lim = q->max_dist * q->max_dist;
            ax.r = (float)(p.x - (double)A.g0[0]), ay.r = (float)(p.y - (double)A.g0[1]), az.r = (float)(p.z - (double)A.g0[2]);
            ax.pad = (fabsf(ax.r) + A.E) * 4.7683716e-7f, ay.pad = (fabsf(ay.r) + A.E) * 4.7683716e-7f, az.pad = (fabsf(az.r) + A.E) * 4.7683716e-7f;
            best_d2 = lim, best_al = 0.0, best_be = 0.0;
            best_prim = INT32_MAX, best_feature = -1;
            bestf = f32_above(best_d2);
            sp = 0;
            cur = 0; // the root
            qi = next;
            have = true;
            active = A.n_tris != 0 && lim == lim; // (no triangles, or a NaN radius: the miss record)
        }
        if (__ballot(active || have) == 0ULL && pool.exhausted) break;
        do {
            if (active) {
                if ((int32_t)cur >= 0) {
                    const uint4* np = reinterpret_cast<const uint4*>(A.nodes + cur);
                    const uint4 bx = np[0], by = np[1], bz = np[2], rf = np[3];
                    if (COUNT) n_nodes++;
                    const float l0 = box_bound(bx.x, by.x, bz.x, ax, ay, az), l1 = box_bound(bx.y, by.y, bz.y, ax, ay, az);
                    const float l2 = box_bound(bx.z, by.z, bz.z, ax, ay, az), l3 = box_bound(bx.w, by.w, bz.w, ax, ay, az);
                    // bounds are >= +0: as unsigned integers they order like the floats.  A child is kept unless its bound is
                    // strictly above the best (a NaN bound fails the comparison: dropped).  An unused slot is recognised by its ref,
                    // as in the ray traversal — its inverted range is no box and its "bound" means nothing; only slots 2 and 3 can
                    // be unused in a builder's tree, the other two checks cost nothing and keep a one-triangle root safe.
                    uint32_t k0 = (l0 <= bestf && rf.x != kUnusedRef) ? __float_as_uint(l0) : kNoKey;
                    uint32_t k1 = (l1 <= bestf && rf.y != kUnusedRef) ? __float_as_uint(l1) : kNoKey;
                    uint32_t k2 = (l2 <= bestf && rf.z != kUnusedRef) ? __float_as_uint(l2) : kNoKey;
                    uint32_t k3 = (l3 <= bestf && rf.w != kUnusedRef) ? __float_as_uint(l3) : kNoKey;
                    uint32_t r0 = rf.x, r1 = rf.y, r2 = rf.z, r3 = rf.w;
#define PRT_CE(ka, ra, kb, rb)              \
            {                                       \
                const bool sw_ = kb < ka;           \
                const uint32_t tk_ = sw_ ? kb : ka; \
                kb = sw_ ? ka : kb;                 \
                ka = tk_;                           \
                const uint32_t tr_ = sw_ ? rb : ra; \
                rb = sw_ ? ra : rb;                 \
                ra = tr_;                           \
            }
                    PRT_CE(k0, r0, k1, r1)
                    PRT_CE(k2, r2, k3, r3)
                    PRT_CE(k0, r0, k2, r2)
                    PRT_CE(k1, r1, k3, r3)
                    PRT_CE(k1, r1, k2, r2)
#undef PRT_CE
                    if (k3 != kNoKey) {
                        stk_ref[sp * 64] = r3;
                        stk_lb[sp * 64] = __uint_as_float(k3);
                        sp++;
                    }
                    if (k2 != kNoKey) {
                        stk_ref[sp * 64] = r2;
                        stk_lb[sp * 64] = __uint_as_float(k2);
                        sp++;
                    }
                    if (k1 != kNoKey) {
                        stk_ref[sp * 64] = r1;
                        stk_lb[sp * 64] = __uint_as_float(k1);
                        sp++;
                    }
                    cur = k0 != kNoKey ? r0 : kUnusedRef;
                } else if (cur != kUnusedRef) {
                    const uint32_t enc = ~cur;
                    const uint32_t first = enc >> 3, cnt = (enc & 7u) + 1u;
                    for (uint32_t i = 0; i < cnt; ++i) {
                        int32_t prim;
                        const Corners t = load_corners(A.corners + first + i, &prim);
                        if (COUNT) n_tests++;
                        const V a = t.v0, b = t.v1, c = t.v2;
                        double al, be;
                        int32_t feature;
                        point_triangle(p, a, b, c, al, be, feature);
                        const V d = sub(p, bary_point(a, sub(b, a), sub(c, a), al, be));
                        const double d2 = dot(d, d);
                        if (d2 < best_d2 || (d2 == best_d2 && prim < best_prim)) {
                            best_d2 = d2, best_al = al, best_be = be;
                            best_prim = prim, best_feature = feature;
                            best_at = first + i;
                            bestf = f32_above(d2);
                        }
                    }
                    cur = kUnusedRef;
                }
                // nothing to descend into: the nearest pushed entry whose bound the best has not overtaken
                while (cur == kUnusedRef && sp > 0) {
                    sp--;
                    const float lb = stk_lb[sp * 64];
                    const uint32_t r = stk_ref[sp * 64];
                    if (lb <= bestf) cur = r;
                    else if (COUNT) ((int32_t)r >= 0 ? n_drop_inner : n_drop_leaf)++;
                }
                if (cur == kUnusedRef) active = false;
            }
        } while (__popcll(__ballot(active)) > (REFILL ? PRT_K6_KEEP : 0));
    }
    flush_query_counts<COUNT>(A.ctr, lane, n_nodes, n_tests, n_drop_inner, n_drop_leaf);
}

__global__ void __launch_bounds__(256) k_gather_corners(const double* __restrict__ verts, const uint32_t* __restrict__ order, uint32_t n,
                                                        DTriCorners* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = order[i];
    if (t >= n) return; // (a permutation by construction; never index out of the caller's buffer)
    const double* v = verts + (size_t)t * 9;
    double4* o = reinterpret_cast<double4*>(out + i);
    o[0] = make_double4(v[0], v[1], v[2], v[3]);
    o[1] = make_double4(v[4], v[5], v[6], v[7]);
    o[2] = make_double4(v[8], __longlong_as_double((long long)(unsigned long long)t), 0.0, 0.0);
}

} // namespace

// The corners of every triangle from positions in description order ([n][3][xyz]) into leaf order.
void launch_gather_corners(const double* d_verts, const uint32_t* d_order, uint32_t n, DTriCorners* d_out, hipStream_t st) {
    if (n) k_gather_corners<<<(n + 255) / 256, 256, 0, st>>>(d_verts, d_order, n, d_out);
}

namespace {
void fill_args(ClosestArgs& A, const DScene& S, const DTriCorners* d_corners, const PrtPointQuery* d_q, size_t n, void* d_out, DCounters* d_ctr,
               int stack_depth) {
    A.nodes = S.nodes;
    A.corners = d_corners;
    A.q = d_q;
    A.out = static_cast<PrtClosestPoint*>(d_out);
    A.ctr = d_ctr;
    A.n = n;
    A.n_tris = S.n_tris;
    A.stack_depth = std::min(std::max(stack_depth, 1), PRT_STACK_DEPTH);
    for (int a = 0; a < 3; ++a) {
        A.g0[a] = S.grid_origin[a];
        A.gs[a] = S.grid_step[a];
    }
    A.E = S.slab_scale;
}
template <typename Kernel, typename Args>
hipError_t launch_k6(Kernel k, const Args& A, int n_cu, bool plain, hipStream_t st) {
    const size_t lds = (size_t)2 * PRT_BLOCK * A.stack_depth * sizeof(uint32_t); // refs and bounds: at most 80 KB
    unsigned grid = 0;
    const hipError_t e = point_query_grid(reinterpret_cast<const void*>(k), A.n, lds, n_cu, plain, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(PRT_BLOCK), lds, st, A);
    return hipGetLastError();
}
} // namespace

// One batch of queries through K6.  stack_depth: entries per lane (what the resident tree can need); d_out 32-byte aligned;
// d_ctr->next_item is zero (the call slot's start clears the counters); plain: the one-block-per-256-queries form.
hipError_t launch_closest_point(const DScene& S, const DTriCorners* d_corners, const PrtPointQuery* d_q, size_t n, PrtClosestPoint* d_out,
                                DCounters* d_ctr, bool count, int stack_depth, int n_cu, bool plain, hipStream_t st) {
    static_assert(sizeof(PrtPointQuery) == 32 && sizeof(PrtClosestPoint) == 64, "query and answer records");
    if (n == 0) return hipSuccess;
    ClosestArgs A;
    fill_args(A, S, d_corners, d_q, n, d_out, d_ctr, stack_depth);
    auto k = plain ? (count ? k_closest_point<true, false> : k_closest_point<false, false>)
                   : (count ? k_closest_point<true, true> : k_closest_point<false, true>);
    return launch_k6(k, A, n_cu, plain, st);
}

// ... with the sign of the nearest feature's pseudonormal: PrtSignedDistance records (the layout of PrtClosestPoint).
hipError_t launch_signed_distance(const DScene& S, const DTriCorners* d_corners, const DSignedTables& T, const PrtPointQuery* d_q, size_t n,
                                  PrtSignedDistance* d_out, DCounters* d_ctr, bool count, int stack_depth, int n_cu, hipStream_t st) {
    static_assert(sizeof(PrtSignedDistance) == sizeof(PrtClosestPoint) && offsetof(PrtSignedDistance, sign) == offsetof(PrtClosestPoint, reserved),
                  "PrtSignedDistance has the layout of PrtClosestPoint");
    if (n == 0) return hipSuccess;
    SignedArgs A;
    fill_args(A, S, d_corners, d_q, n, d_out, d_ctr, stack_depth);
    A.slot = T.slot;
    A.normal = T.normal;
    A.n_normals = T.n_edges + T.n_vertices;
    return launch_k6(count ? k_closest_point<true, true, true> : k_closest_point<false, true, true>, A, n_cu, false, st);
}

} // namespace prt
