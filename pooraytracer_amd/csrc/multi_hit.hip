// multi_hit.hip — K7: batched multi-hit queries, the first k hits along each ray in (t, prim) order (prt_trace_multi,
// include/prt.h).  A sibling of K1 (prt_kernels.hip) in a translation unit of its own: the same persistent waves, the same
// wave-local ray pool, the same refill of finished lanes, K4's `perm`, the lane-strided LDS stack, and Trav's box stepping
// (inner_step / box4) under the same park-at-leaf round.  What is new is the leaf step: every triangle the closest-hit
// test accepts over [max(tmin, cursor t), bound] goes into a per-lane list of at most k entries sorted by (t, prim).
//
// Contraction is OFF in this translation unit (the pragma below stands before the includes, so it covers tri_test and
// the vector helpers of prt_device.h as they are compiled here): t, alpha and beta of a (ray, record) pair are then the
// same bits in every instantiation (COUNT, PAD) and at both places the test runs (the leaf step and the write-out), which
// the byte-equality and paging contracts rest on.  K1's arithmetic is compiled with contraction on, so slot 0 is a
// closest hit by the same test but not promised bit-equal to prt_trace_closest* (prt.h, contract 5).
// The slab pad with unfused products.  slab_axis's derivation (prt_device.h) already counts the roundings of r, 1/d,
// gs * id, the product c = r * id and box4's fma one by one: 6 * 2^-24 (|r| + E) |id| against a pad of 2^-20 (16 * 2^-24).
// box4's plane parameters are explicit fmaf calls, which stay fused.  The only expressions of slab_axis a contraction
// could have fused are c -+ pad (pad = fmaf(..) * 2^-20: here the product is rounded before the sum, one more rounding
// of 2^-24 of the PAD, i.e. 2^-44 of the quantity the pad covers) - the margin of 10 * 2^-24 takes it.
//
// Why the bytes do not depend on the tree (prt.h, contract 3).  `bound` is the ray's tmax until the list holds k entries,
// then the t of its k-th entry; it only ever shrinks.  (a) A child is skipped only when its fp32 entry parameter n exceeds
// f = min(exit, tbestf) with tbestf = f32_up(bound) >= bound (Trav::box4's `n <= f`).  The box test is conservative: a
// triangle below the box that the test accepts at t has n <= t.  So a skipped subtree holds only candidates with
// t > bound-at-that-time >= the final bound: none of them belongs to the k smallest, and a candidate TYING the k-th t
// (t == bound, a smaller prim) is never culled.  Entries already on the stack are not re-tested at the pop, which only
// tests more.  (b) The leaf step calls tri_test with tmax = bound, INCLUSIVE, so a tie with the k-th entry reaches the
// (t, prim) comparison.  (c) Every tested candidate is placed by an exact comparison of (t, prim), prim being the
// description index (S.shade[tri].prim), and every triangle sits in exactly one leaf, visited at most once.  Hence the list
// is the min(k, #candidates) smallest candidates by (t, prim), whatever order the leaves came in: host tree, device tree,
// rebuilt tree, sorted or plain batch, counting or not.
// The cursor.  Candidates must exceed (after.t, after.prim) lexicographically; the traversal runs over
// [max(tmin, after.t), tmax] (nothing before the cursor's t is fetched) and a candidate AT after.t must have a larger prim.
// A page fed its predecessor's last record continues exactly there, also through a run of equal t.
//
// The list: PRT_MULTI_HIT_MAX (t, leaf position) pairs in registers, indexed statically (every loop over it is fully
// unrolled; a run-time index would send it to scratch).  alpha, beta and front are not kept: the write-out runs tri_test
// once more on the at most k winners - the same function on the same values, identical bits - which costs 12 bytes per
// slot in fp64 instead of 28.  One capacity is compiled (DESIGN.md §7 has the register numbers and the reason).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/prt.h"
#include "prt_device.h"
#include "prt_launch.h"

#ifndef PRT_F32_TU
#define PRT_F32_TU 0
#endif
#if PRT_F32_TU
#define PRT_NS prt32
#else
#define PRT_NS prt
#endif

// Resident waves per SIMD the register allocator must leave room for.  Three, not K1's four: with that freedom the plain
// fp64 instantiations come out at 126 registers without scratch and are resident four to a SIMD all the same (what the 40 KB
// of stacks per block allow); asked for four, the padded-record one spills 12 bytes per lane.  The counting instantiations
// take 132 and run three.  The launcher asks the runtime how many blocks of the instantiation at hand a CU holds.
#ifndef PRT_K7_WAVES
#define PRT_K7_WAVES 3
#endif

namespace {

constexpr int CAP = PRT_MULTI_HIT_MAX;

template <bool COUNT, bool PAD>
__global__ __launch_bounds__(PRT_BLOCK, PRT_K7_WAVES) void k_trace_multi(DScene S, const PrtRay* __restrict__ rays,
                                                                         const PrtHitCursor* __restrict__ after, size_t n, int k,
                                                                         PrtHit* __restrict__ out, DCounters* ctr,
                                                                         const uint32_t* __restrict__ perm) { // K4's order or null
    __shared__ uint32_t s_stack[PRT_BLOCK / 64][PRT_STACK_DEPTH][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* stk = &s_stack[wave][0][lane];
    WorkCount wc{0, 0, 0, 0, 0};
    uint32_t nrays = 0;
    Trav<PAD> tr; // tr.hit.t is the bound, tr.tmin the lower end max(tmin, cursor t)
    tr.init(S, mk3(0, 0, 0), mk3(0, 0, 1), RL(0.0), RL(0.0));
    tr.active = false;
    real lt[CAP];    // the list: t ascending, ties in ascending prim
    int32_t li[CAP]; // ... and the leaf position of each entry, -1: empty
#pragma unroll
    for (int i = 0; i < CAP; ++i) lt[i] = PRT_INF, li[i] = -1;
    real cur_t = -PRT_INF; // the cursor
    int32_t cur_prim = -1;
    bool have = false;
    size_t my = 0;
    WavePool<PRT_K1_CHUNK> pool; // the wave's rays, K1's chunk and keep (prt_wave.h)
    for (;;) {
        if (!tr.active && have) { // the lane's traversal has ended: its k records, 32 bytes at a time
            double4* o = reinterpret_cast<double4*>(out + my * (size_t)k);
#pragma unroll
            for (int i = 0; i < CAP; ++i) {
                if (i < k) {
                    double4 rec = make_double4(__builtin_huge_val(), 0.0, 0.0, __longlong_as_double(0xffffffffll)); // the miss record
                    if (li[i] >= 0) {
                        const DTri* T = tri_at<PAD>(S, (uint32_t)li[i]);
                        real t = lt[i], al = RL(0.0), be = RL(0.0);
                        tri_test(T, tr.o, tr.d, tr.tmin, lt[i], t, al, be); // the leaf step's test once more: the same bits
                        const int32_t front = dot(tr.d, mk3(T->n[0], T->n[1], T->n[2])) < RL(0.) ? 1 : 0; // HitRecord::SetFaceNormal
                        const uint32_t prim = (uint32_t)S.shade[li[i]].prim;
                        rec = make_double4((double)t, (double)al, (double)be,
                                           __longlong_as_double((long long)(((unsigned long long)(uint32_t)front << 32) | prim)));
                    }
                    o[i] = rec;
                }
            }
            have = false;
        }
        {
            const unsigned long long need = __ballot(!tr.active);
            if (pool.wants(need)) {
                pool.refill(need, lane, n, &ctr->next_item);
                if (!pool.exhausted && !tr.active) {
                    const unsigned long long idx = pool.index(need, lane);
                    if (idx < pool.end) {
                        const size_t ri = perm ? (size_t)perm[idx] : (size_t)idx; // the idx-th ray of the sorted order
                        const double4* rp = reinterpret_cast<const double4*>(rays + ri);
                        const double4 r0 = rp[0], r1 = rp[1];
                        cur_t = -PRT_INF, cur_prim = -1;
                        bool dead = false;
                        if (after) {
                            const double2 c = *reinterpret_cast<const double2*>(after + ri);
                            cur_t = (real)c.x; // (fp32: rounded to float once, here)
                            cur_prim = (int32_t)(uint32_t)__double_as_longlong(c.y);
                            dead = c.x != c.x; // nothing is greater than a NaN cursor: the miss records
                        }
                        const real tmin = (real)r0.w;
                        tr.init(S, mk3((real)r0.x, (real)r0.y, (real)r0.z), mk3((real)r1.x, (real)r1.y, (real)r1.z),
                                cur_t > tmin ? cur_t : tmin, (real)r1.w);
                        if (dead) tr.active = false;
#pragma unroll
                        for (int i = 0; i < CAP; ++i) lt[i] = PRT_INF, li[i] = -1;
                        my = ri;
                        have = true;
                        nrays++;
                    }
                }
                pool.advance(need);
            }
        }
        if (__ballot(tr.active || have) == 0ULL && pool.exhausted) break;
        do { // Trav::round with this kernel's leaf step
            if (COUNT && __ballot(tr.active && tr.cur >= 0) != 0ULL) wc.inner_rounds++;
            if (tr.active && tr.cur >= 0) tr.template inner_step<COUNT>(S, stk, wc);
            const bool has_leaf = tr.active && tr.cur < 0 && tr.cur != PRT_NOCUR; // parked at a leaf
            const int n_parked = __popcll(__ballot(tr.active && tr.cur < 0));
            const int n_inner = __popcll(__ballot(tr.active && tr.cur >= 0));
            if (n_parked >= PRT_LEAF_BATCH || n_inner <= PRT_INNER_MIN) {
                if (COUNT && __ballot(has_leaf) != 0ULL) wc.leaf_rounds++;
                if (has_leaf) {
                    const uint32_t enc = ~(uint32_t)tr.cur;
                    const uint32_t first = enc >> 3, cnt = (enc & 7u) + 1u;
                    real4 q0n = *reinterpret_cast<const real4*>(tri_at<PAD>(S, first)); // the next plane ahead of its test, as test_leaf
                    for (uint32_t j = 0; j < cnt; ++j) {
                        real t, al, be;
                        if (COUNT) wc.tris++;
                        const real4 q0c = q0n;
                        if (j + 1 < cnt) q0n = *reinterpret_cast<const real4*>(tri_at<PAD>(S, first + j + 1));
                        if (!tri_test(tri_at<PAD>(S, first + j), tr.o, tr.d, tr.tmin, tr.hit.t, t, al, be, &q0c, COUNT ? &wc.tris_full : nullptr))
                            continue;
                        const int32_t tri = (int32_t)(first + j);
                        const int32_t prim = S.shade[tri].prim;
                        if (t == cur_t && prim <= cur_prim) continue; // at or before the cursor
                        int pos = 0; // entries that sort before the candidate
#pragma unroll
                        for (int i = 0; i < CAP; ++i) {
                            bool before = false;
                            if (li[i] >= 0) {
                                if (lt[i] < t) before = true;
                                else if (lt[i] == t) before = S.shade[li[i]].prim < prim; // an exact tie: the description index decides
                            }
                            pos += before ? 1 : 0;
                        }
                        if (pos >= k) continue; // ties the k-th t with a larger prim
#pragma unroll
                        for (int i = CAP - 1; i >= 0; --i) {
                            if (i > 0 && i > pos) lt[i] = lt[i - 1], li[i] = li[i - 1];
                            else if (i == pos) lt[i] = t, li[i] = tri;
                        }
#pragma unroll
                        for (int i = 0; i < CAP; ++i)
                            if (i == k - 1 && li[i] >= 0) { // the list is full: its last t bounds what can still enter
                                tr.hit.t = lt[i];
                                tr.tbestf = f32_up(lt[i]);
                            }
                    }
                    if (tr.sp == 0) {
                        tr.cur = PRT_NOCUR;
                        tr.active = false;
                    } else {
                        tr.sp--;
                        tr.cur = (int32_t)stk[tr.sp * 64];
                    }
                }
            }
        } while (wave_count(tr.active) > PRT_K1_KEEP);
    }
    flush_trace_counts<COUNT>(ctr, lane, &ctr->rays_closest, nrays, wc);
}

} // namespace

namespace PRT_NS {

// One batch of rays through K7: k records per ray into d_out (32-byte aligned), d_after null or one cursor per ray;
// d_ctr->next_item is zero (the call slot's start clears the counters); 1 <= k <= PRT_MULTI_HIT_MAX is the caller's check.
hipError_t launch_multi_hit(const DScene& S, const PrtRay* d_rays, const PrtHitCursor* d_after, size_t n, int k, PrtHit* d_out,
                            DCounters* d_ctr, bool count, int n_cu, hipStream_t st, const uint32_t* d_perm) {
    static_assert(sizeof(PrtHit) == 32 && sizeof(PrtHitCursor) == 16, "a hit is one 32-byte store, a cursor one 16-byte load");
    if (n == 0) return hipSuccess;
    if (k < 1 || k > CAP) return hipErrorInvalidValue;
    const size_t want = (n + PRT_BLOCK - 1) / PRT_BLOCK;
    const bool pad = S.tri_stride == PRT_TRI_PAD_STRIDE(real) && sizeof(DTri) != PRT_TRI_PAD_STRIDE(real);
    auto go = [&](auto kern) {
        // persistent waves: as many blocks as can be resident (registers and the 40 KB of stacks decide: three or four per CU)
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, PRT_BLOCK, 0) != hipSuccess || per_cu < 1) per_cu = PRT_K7_WAVES;
        const unsigned grid = (unsigned)std::min<size_t>(want, (size_t)std::max(n_cu, 1) * (size_t)per_cu);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(PRT_BLOCK), 0, st, S, d_rays, d_after, n, k, d_out, d_ctr, d_perm);
        return hipGetLastError();
    };
    switch ((count ? 2 : 0) | (pad ? 1 : 0)) {
    case 0: return go(k_trace_multi<false, false>);
    case 1: return go(k_trace_multi<false, true>);
    case 2: return go(k_trace_multi<true, false>);
    default: return go(k_trace_multi<true, true>);
    }
}

} // namespace PRT_NS
