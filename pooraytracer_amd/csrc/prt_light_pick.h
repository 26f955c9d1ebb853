// prt_light_pick.h — the O(1) light-table lookup (prt_types.h, DLightTable), shared by the render kernels' sample_lights
// (prt_device.h) and by the device-side verification of freshly built tables (light_tables.hip): what is verified is the
// code that picks.  Plain float / uint32 arithmetic, no dependence on the kernels' precision.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The leaf (index into the table's own leaves, 0 .. n-1, plus DLightTable::first) that the float `pf` reaches in the table
// whose header starts at `tab + 8 * table`: one bucket read gives the first leaf pf can reach and the threshold of the next
// one, then a short walk along thr[].  thr[n] = +inf ends every walk of a well-formed table.
// CHECKED (the verification only; the render kernels instantiate false): a walk that would leave thr[0..n] or a bucket
// index beyond n_bkt answers -1 instead of reading on.
template <bool CHECKED>
__device__ __forceinline__ int32_t light_table_leaf(const uint32_t* tab, uint32_t table, float pf) {
    const uint4* h = reinterpret_cast<const uint4*>(tab + 8u * table);
    const uint4 h0 = h[0];                                   // first, n, thr_off, bkt_off
    const uint2 h1 = *reinterpret_cast<const uint2*>(h + 1); // n_bkt, inv_w
    const uint32_t k = (uint32_t)fminf(pf * __uint_as_float(h1.y), (float)(h1.x - 1u));
    if (CHECKED && k >= h1.x) return -1;
    const uint2 e = *reinterpret_cast<const uint2*>(tab + h0.w + 2u * k);
    uint32_t i = e.x;
    float next = __uint_as_float(e.y);
    if (CHECKED && i >= h0.y) return -1;
    while (next <= pf) {
        ++i;
        if (CHECKED && i >= h0.y) return -1;
        next = __uint_as_float(tab[h0.z + i + 1u]);
    }
    return (int32_t)(h0.x + i);
}
