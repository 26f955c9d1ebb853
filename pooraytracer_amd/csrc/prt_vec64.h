// prt_vec64.h — the fp64 vector helpers and the corner-record reader of the files that work on the scene's DTriCorners table
// (closest_point.hip, winding_number.hip, pseudonormals.hip, bvh_refit.hip).
//
// INCLUDE IT AFTER `#pragma clang fp contract(off)`, and nowhere contraction is on: every expression here is meant to be
// evaluated operation by operation (the numpy models of the tests evaluate the same expressions), and the pragma in force
// where this text is compiled decides that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prt_types.h"

namespace prt {
namespace {

struct V {
    double x, y, z;
};
__device__ __forceinline__ V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V add(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V scale(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V cross(V a, V b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

struct Corners {
    V v0, v1, v2;
};
// One 96-byte record of the corner table: two 32-byte loads and the last coordinate.  A caller that asks for `prim`, the
// triangle's index in description order, gets it from the same 16-byte load (it sits behind v2.z); the others load 8 bytes.
__device__ __forceinline__ Corners load_corners(const DTriCorners* t, int32_t* prim = nullptr) {
    const double4* rec = reinterpret_cast<const double4*>(t);
    const double4 c0 = rec[0], c1 = rec[1];
    double2 c2;
    if (prim) {
        c2 = *reinterpret_cast<const double2*>(rec + 2);
        *prim = (int32_t)(uint32_t)__double_as_longlong(c2.y);
    } else {
        c2.x = *reinterpret_cast<const double*>(rec + 2);
    }
    return {V{c0.x, c0.y, c0.z}, V{c0.w, c1.x, c1.y}, V{c1.z, c1.w, c2.x}};
}

} // namespace
} // namespace prt
