// light_tables.hip — the O(1) light-pick tables (prt_types.h, DLightTable) of a resident scene rebuilt on the GPU when an
// emitter moves (prt_scene_set_dynamic_lights, include/prt.h).  The host keeps what defines the order and the sums — the
// Triangle precompute of the emitter triangles, the reference's two std::sort passes, areas and pdfs, and the PLAN of the
// tables (scene_setup.cpp, plan_light_tables: headers, offsets, the part of the tree above the tables); the device does
// the part that is exact and independent per word, the host's fill_light_tables / verify_light_tables word for word:
//
//   k_light_thresholds  one lane per threshold word: thr[0] = 0, thr[n] = +inf, thr[i] = the smallest float pattern whose
//                       descent of the table's subtree reaches leaf first + i or one to its right (a 31-step bisection,
//                       each step one descent)
//   k_light_buckets     one lane per bucket: the smallest pattern that falls into the bucket (bisection through the kernels'
//                       own bucket expression), one descent from it, entry {leaf, thr[leaf + 1]}; an unreachable bucket
//                       gets {n - 1, thr[n]}.  Runs after the thresholds on the same stream.
//   k_light_verify      the host's deterministic verification points, one lane per word: every threshold and the patterns
//                       beside it, both ends of every bucket — the table pick (prt_light_pick.h: the render kernels' code)
//                       against the descent of the full tree
//   k_light_verify_rnd  per table 0 / area / 3e38 / 1e-30 and 2^16 random patterns below twice the area; 2^18 random
//                       patterns up to the total area, the 129 patterns around it and 0 through the WHOLE pick (top nodes,
//                       then table) against the full tree.  Every lane draws from a sub-stream of its own (xorshift64
//                       seeded from the lane index), so the random points are not the host's draws; the fixed ones are.
//
// The lanes of a wave walk the same top nodes of a subtree and part ways near the leaves: the 16-byte DLightNode reads are
// served by L1 / L2 as they are (a 6,400-triangle tree is 100 KB); nothing is staged in LDS.
// fp64 compare and subtract, a round to float per level, fp32 multiply and min for the bucket: all IEEE-exact here as on
// the host (contraction off; fp32 denormals are on by default — the bisection visits denormal patterns).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "prt_light_pick.h"
#include "prt_types.h"

#pragma clang fp contract(off)

#include "prt_launch.h"

namespace prt {
namespace {

constexpr unsigned kBlock = 256;
constexpr int kMaxLevels = 128; // no light tree is that deep (median splits of at most 2^31 leaves, twice); bounds every descent
constexpr uint32_t kInf = 0x7f800000u, kMaxFinite = 0x7f7fffffu;

struct Hdr {
    uint32_t first, n, thr_off, bkt_off, n_bkt;
    float inv_w;
};
__device__ inline Hdr header(const uint32_t* tab, uint32_t t) {
    const uint4 a = *reinterpret_cast<const uint4*>(tab + 8u * t);
    const uint2 b = *reinterpret_cast<const uint2*>(tab + 8u * t + 4u);
    return Hdr{a.x, a.y, a.z, a.w, b.x, __uint_as_float(b.y)};
}
// the table whose thresholds or buckets hold word w (w >= 8 * n_tables; the tables' words follow each other in table order)
__device__ inline uint32_t table_of_word(const uint32_t* tab, uint32_t n_tables, uint32_t w) {
    uint32_t lo = 0, hi = n_tables - 1u; // the last table whose thr_off <= w
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (tab[8u * mid + 2u] <= w) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// scene_setup.cpp, descend: TraverseSample on the flattened nodes.  The leaf's CDF index; -1 for a ref out of range or a
// descent that does not end (neither happens on a tree the host flattened).
__device__ inline int32_t descend(const DLightNodeT<double>* __restrict__ nodes, uint32_t n_nodes, int32_t node, float p) {
    for (int level = 0; node >= 0; ++level) {
        if ((uint32_t)node >= n_nodes || level >= kMaxLevels) return -1;
        const DLightNodeT<double> ln = nodes[node];
        if ((double)p < ln.left_area) node = ln.left;
        else {
            p = (float)((double)p - ln.left_area);
            node = ln.right;
        }
    }
    return ~node;
}
__device__ inline uint32_t bucket_of(float p, float inv_w, uint32_t n_bkt) { // the kernels' expression (prt_light_pick.h)
    return (uint32_t)fminf(p * inv_w, (float)(n_bkt - 1u));
}
// scene_setup.cpp, first_pattern: the smallest pattern in [0, 0x7f7fffff] with pred, 0x7f800000 if none
template <typename Pred>
__device__ inline uint32_t first_pattern(Pred pred) {
    if (!pred(__uint_as_float(kMaxFinite))) return kInf;
    uint32_t lo = 0, hi = kMaxFinite;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pred(__uint_as_float(mid))) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}
__device__ inline uint32_t bucket_first_pattern(const Hdr& H, uint32_t b) {
    return first_pattern([&](float p) { return bucket_of(p, H.inv_w, H.n_bkt) >= b; });
}

__global__ void __launch_bounds__(kBlock) k_light_thresholds(DLightTableBuild A) {
    const uint64_t x = 8ull * A.n_tables + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= A.n_words) return;
    const uint32_t w = (uint32_t)x, t = table_of_word(A.tab, A.n_tables, w);
    const Hdr H = header(A.tab, t);
    if (w < H.thr_off || w >= H.bkt_off) return; // a bucket word
    const uint32_t i = w - H.thr_off;            // 0 .. n
    uint32_t pat = 0u;
    if (i >= H.n) pat = kInf;
    else if (i > 0) {
        const int32_t k = A.table_node[t], want = (int32_t)(H.first + i);
        pat = first_pattern([&](float p) { return descend(A.full, A.n_full, k, p) >= want; });
    }
    A.tab[w] = pat;
}

__global__ void __launch_bounds__(kBlock) k_light_buckets(DLightTableBuild A) {
    const uint64_t x = 8ull * A.n_tables + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= A.n_words) return;
    const uint32_t w = (uint32_t)x, t = table_of_word(A.tab, A.n_tables, w);
    const Hdr H = header(A.tab, t);
    if (w < H.bkt_off || ((w - H.bkt_off) & 1u) || w + 1u >= A.n_words) return; // one lane per {leaf, next threshold} pair
    const uint32_t b = (w - H.bkt_off) >> 1;
    if (b >= H.n_bkt) return;
    const uint32_t pat = bucket_first_pattern(H, b);
    uint32_t i = H.n - 1u; // a bucket no p falls into: anything valid
    if (pat != kInf) i = (uint32_t)descend(A.full, A.n_full, A.table_node[t], __uint_as_float(pat)) - H.first;
    if (i >= H.n) i = H.n - 1u; // (never on a well-formed tree; the verification then refuses the table)
    A.tab[w] = i;
    A.tab[w + 1u] = A.tab[H.thr_off + i + 1u];
}

__device__ inline bool same_sub(const DLightTableBuild& A, uint32_t t, float p) {
    return light_table_leaf<true>(A.tab, t, p) == descend(A.full, A.n_full, A.table_node[t], p);
}
// the whole pick as sample_lights runs it (prt_device.h): the top nodes, then the table
__device__ inline bool same_whole(const DLightTableBuild& A, float p) {
    int32_t node = A.root;
    float pf = p;
    for (int level = 0; (uint32_t)node < (uint32_t)PRT_LIGHT_TABLE_BIT; ++level) {
        if ((uint32_t)node >= A.n_top || level >= kMaxLevels) return false;
        const DLightNodeT<double> ln = A.top[node];
        if ((double)pf < ln.left_area) node = ln.left;
        else {
            pf = (float)((double)pf - ln.left_area);
            node = ln.right;
        }
    }
    int32_t leaf = ~node;
    if (node >= 0) {
        const uint32_t t = (uint32_t)node & ~(uint32_t)PRT_LIGHT_TABLE_BIT;
        if (t >= A.n_tables) return false;
        leaf = light_table_leaf<true>(A.tab, t, pf);
    }
    return leaf == descend(A.full, A.n_full, A.full_root, p);
}

__global__ void __launch_bounds__(kBlock) k_light_verify(DLightTableBuild A) {
    const uint64_t x = 8ull * A.n_tables + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= A.n_words) return;
    const uint32_t w = (uint32_t)x, t = table_of_word(A.tab, A.n_tables, w);
    const Hdr H = header(A.tab, t);
    bool ok = true;
    if (w < H.thr_off) ok = false;
    else if (w < H.bkt_off) { // a threshold, one pattern below and one above
        const uint32_t b = A.tab[w];
        if (b != kInf) ok = ok && same_sub(A, t, __uint_as_float(b));
        if (b != 0u && b <= kInf) ok = ok && same_sub(A, t, __uint_as_float(b - 1u));
        if (b < kMaxFinite) ok = ok && same_sub(A, t, __uint_as_float(b + 1u));
    } else if (!((w - H.bkt_off) & 1u)) { // both ends of a bucket
        const uint32_t b = (w - H.bkt_off) >> 1;
        const uint32_t pat = b < H.n_bkt ? bucket_first_pattern(H, b) : kInf;
        if (pat != kInf) {
            ok = ok && same_sub(A, t, __uint_as_float(pat));
            if (pat) ok = ok && same_sub(A, t, __uint_as_float(pat - 1u));
        }
    }
    if (!ok) *A.flag = 1u;
}

__device__ inline uint64_t lane_stream(uint64_t lane) { // a xorshift64 sub-stream per lane: the host's seed mixed with the lane index
    uint64_t z = 0x9E3779B97F4A7C15ull + lane * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 30;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    if (!z) z = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 2; ++k) {
        z ^= z << 13;
        z ^= z >> 7;
        z ^= z << 17;
    }
    return z;
}

constexpr uint32_t kRndPerTable = 65536u, kRndWhole = 262144u, kWrap = 129u;

__global__ void __launch_bounds__(kBlock) k_light_verify_rnd(DLightTableBuild A) {
    const uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t per_table = (uint64_t)A.n_tables * kRndPerTable;
    bool ok = true;
    if (x < per_table) {
        const uint32_t t = (uint32_t)(x / kRndPerTable), r = (uint32_t)(x % kRndPerTable);
        const double area = A.table_area[t];
        const uint32_t top_pat = __float_as_uint((float)(2.0 * area));
        ok = same_sub(A, t, __uint_as_float((uint32_t)(lane_stream(x) % ((uint64_t)top_pat + 1u))));
        if (r < 4u) ok = ok && same_sub(A, t, r == 0u ? 0.f : r == 1u ? (float)area : r == 2u ? 3.0e38f : 1e-30f);
    } else {
        const uint64_t y = x - per_table;
        const uint32_t tot_pat = __float_as_uint(A.total);
        if (y < kRndWhole) ok = same_whole(A, __uint_as_float((uint32_t)(lane_stream(x) % ((uint64_t)tot_pat + 1u))));
        else if (y < kRndWhole + kWrap) { // the wrap-around region
            const uint32_t b = (tot_pat > 64u ? tot_pat - 64u : 0u) + (uint32_t)(y - kRndWhole);
            if (b <= tot_pat + 64u) ok = same_whole(A, __uint_as_float(b));
        } else if (y == kRndWhole + kWrap) ok = same_whole(A, 0.f);
    }
    if (!ok) *A.flag = 1u;
}

inline unsigned blocks_for(uint64_t items) { return (unsigned)std::max<uint64_t>(1, (items + kBlock - 1) / kBlock); }

} // namespace

// Fill and verify the planned tables of A on `st`; *A.flag (zeroed here) is 1 afterwards if the tables must not be used.
hipError_t launch_light_tables(const DLightTableBuild& A, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(A.flag, 0, sizeof(uint32_t), st);
    if (e != hipSuccess || A.n_tables == 0 || A.n_words <= 8u * A.n_tables) return e;
    const unsigned words = blocks_for((uint64_t)A.n_words - 8ull * A.n_tables);
    k_light_thresholds<<<words, kBlock, 0, st>>>(A);
    k_light_buckets<<<words, kBlock, 0, st>>>(A);
    k_light_verify<<<words, kBlock, 0, st>>>(A);
    k_light_verify_rnd<<<blocks_for((uint64_t)A.n_tables * kRndPerTable + kRndWhole + kWrap + 1u), kBlock, 0, st>>>(A);
    return hipGetLastError();
}

} // namespace prt
