// winding_number.hip — K8: batched generalized winding numbers against the resident 4-wide BVH (prt_winding_number,
// include/prt.h; Jacobson et al. 2013, the dipole form of Barill et al. 2018), and the moments table it reads.
//
//   k_winding_moments  bottom-up over the nodes, in the shape of k_refit_boxes (bvh_refit.hip): every thread fills the
//                      records of the leaf slots of its own node from the corner table, then arrives at the node's
//                      counter; the last arriver of a node fills the records of its inner slots from the children's
//                      records and climbs.  One 64-byte record {N[3], c[3], r, A} per child slot: the area vector, the
//                      area-weighted centroid, a radius around it that holds every corner below, the area.  Every sum is
//                      taken by one thread in leaf / slot order from 0.0: no floating-point atomics, one tree always gives
//                      the same bits.
//   k_winding_number   one lane per query: a walk from the root.  A slot whose cluster is far (|c - p|^2 > (beta r)^2) adds
//                      its dipole dot(N, d) / |d|^3; a near leaf adds the exact solid angle of each of its triangles (Van
//                      Oosterom and Strackee 1983); a near inner slot is walked.
//
// Leaves are popped as rounds of their own, not evaluated inside the node visit.  A node visit is four 64-byte record
// loads and at most four short far terms; a leaf is up to four fp64 atan2, each a few hundred instructions.  Inline, one
// lane with four near leaves holds its wave for sixteen of them inside one visit while the lanes that took far terms
// idle; as entries of the stack, the leaves of different lanes meet in the same step (a lane near the surface pops
// several in a row, and lanes of one wave are near the surface together or not at all for coherent batches), the visit
// stays short, and the registers of the solid angle are not live across the record loads.
//
// Stack.  Entries are refs only, 4 bytes, lane-strided (entry e of lane l at word e*64+l): there is no bound to carry, a
// near slot is always walked.  A visit keeps one near slot as the next step and pushes at most three, so the builders'
// bound on the ray traversal's stack holds here unchanged.  Schedule: K6's persistent waves with the chunked refill -
// queries differ in work by the same two orders of magnitude (far from the mesh: a handful of far terms at the root).
// The order of a query's terms is fixed by the tree alone, so its value does not depend on the batch or the schedule.
//
// fp64 with contraction OFF in this file: tests/winding_model.py evaluates the same expressions in numpy.  Division and
// sqrt are correctly rounded; atan2 is the device library's (a few ulp).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/prt.h"
#include "prt_types.h"

#pragma clang fp contract(off)

#include "prt_launch.h"
#include "prt_vec64.h"
#include "prt_wave.h"

namespace prt {
namespace {

constexpr uint32_t kUnusedRef = 0x80000000u;
constexpr uint32_t kNoParent = 0xffffffffu;
constexpr unsigned kBlock = 256;

struct Moment {
    V N, c;
    double r, A;
};
__device__ __forceinline__ Moment load_moment(const DWindingMoment* m) {
    const double4* rec = reinterpret_cast<const double4*>(m);
    const double4 a = rec[0], b = rec[1];
    return {V{a.x, a.y, a.z}, V{a.w, b.x, b.y}, b.z, b.w};
}
__device__ __forceinline__ void store_moment(DWindingMoment* m, const Moment& q) {
    double4* rec = reinterpret_cast<double4*>(m);
    rec[0] = make_double4(q.N.x, q.N.y, q.N.z, q.c.x);
    rec[1] = make_double4(q.c.y, q.c.z, q.r, q.A);
}
__device__ __forceinline__ double dist(V a, V b) {
    const V d = sub(a, b);
    return sqrt(dot(d, d));
}

// The record of a leaf slot: its triangles in leaf order, sums from 0.0 in that order (include/prt.h).
__device__ inline Moment leaf_moment(const DTriCorners* corners, uint32_t first, uint32_t count) {
    double A = 0.0;
    V N{0.0, 0.0, 0.0}, G{0.0, 0.0, 0.0};
    const V v0_first = load_corners(corners + first).v0;
    for (uint32_t k = first; k < first + count; ++k) {
        const Corners t = load_corners(corners + k);
        const V av = scale(cross(sub(t.v1, t.v0), sub(t.v2, t.v0)), 0.5);
        const double a = sqrt(dot(av, av));
        const V s = add(add(t.v0, t.v1), t.v2);
        const V g{s.x / 3.0, s.y / 3.0, s.z / 3.0};
        if (a > 0.0 && a < __builtin_huge_val()) { // (a NaN fails the first comparison)
            A = A + a;
            N = add(N, av);
            G = add(G, scale(g, a));
        }
    }
    Moment m;
    m.A = A, m.N = N;
    m.c = A > 0.0 ? V{G.x / A, G.y / A, G.z / A} : v0_first;
    double r = 0.0;
    for (uint32_t k = first; k < first + count; ++k) {
        const Corners t = load_corners(corners + k);
        const double d0 = dist(t.v0, m.c), d1 = dist(t.v1, m.c), d2 = dist(t.v2, m.c);
        r = d0 > r ? d0 : r;
        r = d1 > r ? d1 : r;
        r = d2 > r ? d2 : r;
    }
    m.r = r;
    return m;
}

__device__ inline int inner_children(const int32_t ref[4]) {
    int k = 0;
    for (int s = 0; s < 4; ++s) k += ref[s] >= 0; // (an unused slot's ref is negative)
    return k;
}

// `mom` is read and written across workgroups inside the launch: no const, no __restrict__ (vector loads behind the
// acquire, never the scalar cache).  The nodes are only read here, and only their refs.  cnt[] is zero at the launch.
__global__ void __launch_bounds__(kBlock) k_winding_moments(const DNode* __restrict__ nodes, uint32_t n_nodes, const uint32_t* __restrict__ parent,
                                                            uint32_t* cnt, const DTriCorners* __restrict__ corners, uint32_t n_tris,
                                                            DWindingMoment* mom) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    int32_t ref[4];
    {
        const int4 r = *reinterpret_cast<const int4*>(nodes[i].ref);
        ref[0] = r.x; ref[1] = r.y; ref[2] = r.z; ref[3] = r.w;
    }
    const Moment zero{V{0.0, 0.0, 0.0}, V{0.0, 0.0, 0.0}, 0.0, 0.0};
    for (int s = 0; s < 4; ++s) { // leaf slots, and zeros for the unused ones (an inner slot is written by the climb)
        const int32_t r = ref[s];
        if (r >= 0) continue;
        Moment m = zero;
        if ((uint32_t)r != kUnusedRef) {
            const uint32_t enc = ~(uint32_t)r, first = enc >> 3, count = (enc & 7u) + 1u;
            if ((uint64_t)first + count <= n_tris) m = leaf_moment(corners, first, count);
        }
        store_moment(mom + (size_t)i * 4 + s, m);
    }
    // The climb of k_refit_boxes: 1 + inner children arrivals complete a node; every arrival releases what the thread wrote
    // (agent scope), the last one acquires before it reads the children's records.
    uint32_t cur = i;
    int kin = inner_children(ref);
    for (;;) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(&cnt[cur], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != (uint32_t)kin) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        for (int s = 0; s < 4; ++s) { // inner slots: the child's used slots in slot order, sums from 0.0
            const int32_t r = ref[s];
            if (r < 0) continue;
            Moment m = zero;
            if ((uint32_t)r < n_nodes) {
                const int4 cr4 = *reinterpret_cast<const int4*>(nodes[r].ref);
                const int32_t cr[4] = {cr4.x, cr4.y, cr4.z, cr4.w};
                Moment ch[4];
                for (int k = 0; k < 4; ++k) ch[k] = load_moment(mom + (size_t)r * 4 + k);
                double A = 0.0;
                V N{0.0, 0.0, 0.0}, G{0.0, 0.0, 0.0}, c0{0.0, 0.0, 0.0};
                bool any = false;
                for (int k = 0; k < 4; ++k) {
                    if ((uint32_t)cr[k] == kUnusedRef) continue;
                    if (!any) c0 = ch[k].c;
                    any = true;
                    A = A + ch[k].A;
                    N = add(N, ch[k].N);
                    G = add(G, scale(ch[k].c, ch[k].A));
                }
                m.A = A, m.N = N;
                m.c = A > 0.0 ? V{G.x / A, G.y / A, G.z / A} : c0;
                double rad = 0.0;
                for (int k = 0; k < 4; ++k) {
                    if ((uint32_t)cr[k] == kUnusedRef) continue;
                    const double d = dist(ch[k].c, m.c) + ch[k].r;
                    rad = d > rad ? d : rad;
                }
                m.r = rad;
            }
            store_moment(mom + (size_t)cur * 4 + s, m);
        }
        const uint32_t p = parent[cur];
        if (p == kNoParent || p >= n_nodes) break;
        cur = p;
        const int4 r = *reinterpret_cast<const int4*>(nodes[cur].ref);
        ref[0] = r.x; ref[1] = r.y; ref[2] = r.z; ref[3] = r.w;
        kin = inner_children(ref);
    }
}

struct WindingArgs {
    const DNode* nodes;
    const DTriCorners* corners;
    const DWindingMoment* mom;
    const PrtPointQuery* q;
    double* out;
    DCounters* ctr;
    size_t n;
    double beta;
    uint32_t n_tris, n_nodes;
    int32_t stack_depth;
};

// The signed solid angle of triangle (v0, v1, v2) seen from p (Van Oosterom and Strackee): positive where p sees the
// triangle clockwise, i.e. from inside a mesh whose faces are counter-clockwise seen from outside.
__device__ __forceinline__ double solid_angle(V p, const Corners& t) {
    const V a = sub(t.v0, p), b = sub(t.v1, p), c = sub(t.v2, p);
    const double la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), lc = sqrt(dot(c, c));
    const double num = dot(a, cross(b, c));
    const double den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb;
    return 2.0 * atan2(num, den);
}

template <bool COUNT>
__global__ __launch_bounds__(PRT_BLOCK, 2) void k_winding_number(WindingArgs A) {
    extern __shared__ uint32_t s_stack[]; // [PRT_BLOCK / 64][stack_depth][64] refs
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* stk = s_stack + (size_t)(wave * A.stack_depth) * 64 + lane;
    V p{0, 0, 0};
    double S = 0.0;
    uint32_t n_nodes = 0, n_tests = 0, n_far_inner = 0, n_far_leaf = 0;
    int32_t sp = 0;
    uint32_t cur = kUnusedRef; // an inner node, a leaf ref, or kUnusedRef: nothing left
    size_t qi = 0;
    bool have = false, active = false;
    WavePool<PRT_K8_CHUNK> pool; // the wave's queries (prt_wave.h)
    for (;;) {
        if (!active && have) { // the lane's walk has ended: its value
            A.out[qi] = S / (4.0 * 3.14159265358979323846);
            have = false;
        }
        bool take = false;
        size_t next = 0;
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
        if (take) { // the lane starts query `next` (max_dist is not read)
            const PrtPointQuery* q = A.q + next;
            p = V{q->p[0], q->p[1], q->p[2]};
            S = 0.0;
            sp = 0;
            cur = 0; // the root
            qi = next;
            have = true;
            active = A.n_tris != 0 && A.n_nodes != 0; // (no triangles: the value is 0)
        }
        if (__ballot(active || have) == 0ULL && pool.exhausted) break;
        do {
            if (active) {
                if ((int32_t)cur >= 0) {
                    uint32_t near0 = kUnusedRef, near1 = kUnusedRef, near2 = kUnusedRef, near3 = kUnusedRef;
                    if (cur < A.n_nodes) { // (a ref of a builder's tree; never read out of the arrays)
                        const uint4 rf = *reinterpret_cast<const uint4*>(A.nodes[cur].ref);
                        const uint32_t ref[4] = {rf.x, rf.y, rf.z, rf.w};
                        if (COUNT) n_nodes++;
                        const DWindingMoment* mm = A.mom + (size_t)cur * 4;
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            if (ref[s] == kUnusedRef) continue;
                            if (s > 0 && (int32_t)ref[s] < 0 && ref[s] == ref[s - 1]) continue; // (the one-triangle root lists its leaf twice)
                            const Moment m = load_moment(mm + s);
                            const V d = sub(m.c, p);
                            const double dd = dot(d, d), br = A.beta * m.r;
                            if (dd > br * br) { // far: the cluster's dipole (beta = inf: br is inf or NaN, never far)
                                S = S + dot(m.N, d) / (dd * sqrt(dd));
                                if (COUNT) ((int32_t)ref[s] >= 0 ? n_far_inner : n_far_leaf)++;
                            } else { // near: walked, in slot order
                                if (near0 == kUnusedRef) near0 = ref[s];
                                else if (near1 == kUnusedRef) near1 = ref[s];
                                else if (near2 == kUnusedRef) near2 = ref[s];
                                else near3 = ref[s];
                            }
                        }
                    }
                    if (near3 != kUnusedRef) stk[(sp++) * 64] = near3;
                    if (near2 != kUnusedRef) stk[(sp++) * 64] = near2;
                    if (near1 != kUnusedRef) stk[(sp++) * 64] = near1;
                    cur = near0;
                } else if (cur != kUnusedRef) {
                    const uint32_t enc = ~cur;
                    const uint32_t first = enc >> 3, cnt = (enc & 7u) + 1u;
                    if ((uint64_t)first + cnt <= A.n_tris)
                        for (uint32_t i = 0; i < cnt; ++i) {
                            const Corners t = load_corners(A.corners + first + i);
                            if (COUNT) n_tests++;
                            S = S + solid_angle(p, t);
                        }
                    cur = kUnusedRef;
                }
                if (cur == kUnusedRef && sp > 0) cur = stk[(--sp) * 64];
                if (cur == kUnusedRef) active = false;
            }
        } while (__popcll(__ballot(active)) > PRT_K8_KEEP);
    }
    flush_query_counts<COUNT>(A.ctr, lane, n_nodes, n_tests, n_far_inner, n_far_leaf);
}

} // namespace

// The moments of every child slot of `d_nodes` from the corner table, on `st` behind whatever wrote the corners and
// d_parent.  d_cnt: n_nodes counters, zeroed here (rounded up to 16 bytes: the caller allocates that much); d_mom: 4 records
// per node, every one of them written.
hipError_t launch_winding_moments(const DNode* d_nodes, uint32_t n_nodes, const uint32_t* d_parent, uint32_t* d_cnt,
                                  const DTriCorners* d_corners, uint32_t n_tris, DWindingMoment* d_mom, hipStream_t st) {
    static_assert(sizeof(DWindingMoment) == 64 && sizeof(DTriCorners) == 96, "records are moved 32 bytes at a time");
    if (n_nodes == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(d_cnt, 0, (((size_t)n_nodes * sizeof(uint32_t)) + 15) & ~(size_t)15, st);
    if (e != hipSuccess) return e;
    k_winding_moments<<<(n_nodes + kBlock - 1) / kBlock, kBlock, 0, st>>>(d_nodes, n_nodes, d_parent, d_cnt, d_corners, n_tris, d_mom);
    return hipSuccess;
}

// One batch of queries through K8.  stack_depth: entries per lane (what the resident tree can need); d_ctr->next_item is
// zero (the call slot's start clears the counters).
hipError_t launch_winding_number(const DScene& S, const DTriCorners* d_corners, const DWindingMoment* d_mom, const PrtPointQuery* d_q, size_t n,
                                 double beta, double* d_out, DCounters* d_ctr, bool count, int stack_depth, int n_cu, hipStream_t st) {
    static_assert(sizeof(PrtPointQuery) == 32, "query record");
    if (n == 0) return hipSuccess;
    WindingArgs A;
    A.nodes = S.nodes;
    A.corners = d_corners;
    A.mom = d_mom;
    A.q = d_q;
    A.out = d_out;
    A.ctr = d_ctr;
    A.n = n;
    A.beta = beta;
    A.n_tris = S.n_tris;
    A.n_nodes = S.n_nodes;
    A.stack_depth = std::min(std::max(stack_depth, 1), PRT_STACK_DEPTH);
    const size_t lds = (size_t)PRT_BLOCK * A.stack_depth * sizeof(uint32_t); // at most 40 KB
    const auto k = count ? k_winding_number<true> : k_winding_number<false>;
    unsigned grid = 0;
    const hipError_t e = point_query_grid(reinterpret_cast<const void*>(k), n, lds, n_cu, false, grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(PRT_BLOCK), lds, st, A);
    return hipGetLastError();
}

} // namespace prt
