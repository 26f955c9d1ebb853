// prt_wave.h — the wave-level scheduling code the batch kernels share: the wave reduction, the wave-local work pool of the
// persistent-wave kernels (K1 / K1s, K7, K6, K8), their scheduling constants and the counter flush of the two point-query
// kernels.  Integer code only: no floating-point expression lives here, so the header compiles to the same instructions
// whatever the `fp contract` state of the file that includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "prt_types.h"

// The stepping loop of a wave runs while MORE than KEEP of its lanes are still traversing (K1, K7) / descending (K6) /
// walking (K8); below it the finished lanes write their records and are dealt new items.  CHUNK: items a wave takes from
// the global counter at a time.
#ifndef PRT_K1_KEEP
#define PRT_K1_KEEP 48
#endif
#ifndef PRT_K1_CHUNK
#define PRT_K1_CHUNK 1024
#endif
#ifndef PRT_K6_KEEP
#define PRT_K6_KEEP 48
#endif
#ifndef PRT_K6_CHUNK
#define PRT_K6_CHUNK 256
#endif
#ifndef PRT_K8_KEEP
#define PRT_K8_KEEP 48
#endif
#ifndef PRT_K8_CHUNK
#define PRT_K8_CHUNK 256
#endif

namespace {

// the sum over the wave, valid in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The wave-local pool of work items [next, end) of a persistent wave: refilled CHUNK items at a time by ONE atomic per wave
// (a single global counter saturates at ~90 dequeues/us on this chip), dealt to the idle lanes in lane order.
// Invariant: all three members are wave-uniform; next <= end <= n until `exhausted`, which is set by the first fetch whose
// base is at or past n and never cleared: from then on nothing is dealt.  Every index below n is inside exactly one wave's chunk
// and handed to exactly one lane: lane l of the idle set `need` gets next + (idle lanes below l), advance() then moves
// next past all of them (clamped to end: the lanes whose index reached end took nothing and ask again next time).
// Use, in this order and with the kernel's own set-up in between (it is floating-point code and stays in the kernel):
//     const unsigned long long need = __ballot(idle);
//     if (pool.wants(need)) {
//         pool.refill(need, lane, n, counter);
//         if (!pool.exhausted && idle) { idx = pool.index(need, lane); if (idx < pool.end) { ...start item idx... } }
//         pool.advance(need);
//     }
// The pieces keep the statement order the kernels had when each carried this block itself; that, and the condition being
// tested by the kernel and not returned from refill(), is what keeps the kernels' vector instructions what they were
// ("Shared scheduling code of the batch kernels").
template <unsigned long long CHUNK>
struct WavePool {
    unsigned long long next = 0, end = 0;
    bool exhausted = false;

    // whether the idle lanes `need` may be dealt items
    __device__ __forceinline__ bool wants(unsigned long long need) const { return need != 0ULL && !exhausted; }
    // fetches the next chunk when the pool is empty
    __device__ __forceinline__ void refill(unsigned long long need, int lane, size_t n, unsigned long long* counter) {
        if (next >= end) {
            unsigned long long base = 0;
            if (lane == (int)__builtin_ctzll(need)) base = atomicAdd(counter, CHUNK);
            base = __shfl(base, (int)__builtin_ctzll(need), 64);
            next = base;
            end = base + CHUNK < (unsigned long long)n ? base + CHUNK : (unsigned long long)n;
            if (base >= (unsigned long long)n) exhausted = true;
        }
    }
    // the item of idle lane `lane`; taken only if it is below `end`
    __device__ __forceinline__ unsigned long long index(unsigned long long need, int lane) const {
        const unsigned long long below = need & ((1ULL << lane) - 1ULL);
        return next + (unsigned long long)__popcll(below);
    }
    __device__ __forceinline__ void advance(unsigned long long need) {
        if (!exhausted) {
            const unsigned long long taken = (unsigned long long)__popcll(need);
            next = next + taken < end ? next + taken : end;
        }
    }
};

// K6 / K8 after their loop: the wave's four work counts into the call's counters (COUNT instantiations only)
template <bool COUNT>
__device__ __forceinline__ void flush_query_counts(DCounters* ctr, int lane, uint32_t nodes, uint32_t tests, uint32_t c, uint32_t d) {
    if (COUNT) {
        const unsigned long long sa = wave_sum((unsigned long long)nodes), sb = wave_sum((unsigned long long)tests);
        const unsigned long long sc = wave_sum((unsigned long long)c), sd = wave_sum((unsigned long long)d);
        if (lane == 0) {
            atomicAdd(&ctr->node_fetches, sa);
            atomicAdd(&ctr->tri_tests, sb);
            atomicAdd(&ctr->inner_rounds, sc);
            atomicAdd(&ctr->leaf_rounds, sd);
        }
    }
}

} // namespace
