// pseudonormals.hip — the angle-weighted pseudonormals of a scene that answers signed distance queries
// (prt_scene_set_signed_queries, include/prt.h; Baerentzen and Aanaes, IEEE TVCG 2005), from the resident corner table.
//
//   k_face_terms       one thread per leaf position: the triangle's unit normal and its three interior angles, written to the
//                      slot of its prim (the corner record carries it) - the only kernel here that sees the leaf order
//   k_vertex_normals   one thread per vertex: vn = sum of angle * nu over the vertex's (prim, corner) list
//   k_edge_normals     one thread per edge:   en = sum of nu over the edge's prim list
//
// Both lists ascend by prim and each sum starts from +0.0 and is taken in list order by one thread: no atomics, the same
// bits on every run and for every tree over the same triangles.  Work is linear in the list lengths (a vertex of valence
// 3000 is one thread's 3000 additions; a million-triangle soup is three million one-term vertices).  A face that must not
// contribute holds zeros, and adding +0.0 or angle * 0.0 leaves a sum's bits alone (a sum that starts at +0.0 is never -0.0).
//
// fp64 with contraction OFF: tests/signed_distance_model.py evaluates the same expressions in numpy.  Division and sqrt
// are correctly rounded; atan2 is the device library's (a few ulp: the tests' tolerance is derived for that).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/prt.h"
#include "prt_types.h"

#pragma clang fp contract(off)

#include "prt_launch.h"
#include "prt_vec64.h"

namespace prt {
namespace {

constexpr uint32_t kNoSlot = 0xffffffffu;

__device__ __forceinline__ double angle(V e1, V e2) {
    const V c = cross(e1, e2);
    return atan2(sqrt(dot(c, c)), dot(e1, e2));
}

__global__ void __launch_bounds__(256) k_face_terms(const DTriCorners* __restrict__ corners, const uint32_t* __restrict__ slot, uint32_t n,
                                                    double* __restrict__ face) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = (uint32_t)corners[i].prim;
    if (t >= n) return; // (the leaf order is a permutation; never write out of the table)
    const Corners c = load_corners(corners + i);
    const V a = c.v0, b = c.v1, d = c.v2;
    const V nrm = cross(sub(b, a), sub(d, a));
    const double nn = dot(nrm, nrm);
    const uint32_t* s = slot + (size_t)t * 6;
    double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (nn > 0.0 && nn < __builtin_huge_val() && s[0] != kNoSlot && s[1] != kNoSlot && s[2] != kNoSlot) {
        const double len = sqrt(nn);
        o[0] = nrm.x / len, o[1] = nrm.y / len, o[2] = nrm.z / len;
        o[3] = angle(sub(b, a), sub(d, a));
        o[4] = angle(sub(d, b), sub(a, b));
        o[5] = angle(sub(a, d), sub(b, d));
    }
    double* f = face + (size_t)t * 6;
    for (int k = 0; k < 6; ++k) f[k] = o[k];
}

__global__ void __launch_bounds__(256) k_vertex_normals(const uint32_t* __restrict__ start, const uint32_t* __restrict__ list, uint32_t n_vertices,
                                                        uint32_t n_tris, const double* __restrict__ face, double* __restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices) return;
    double x = 0.0, y = 0.0, z = 0.0;
    for (uint32_t i = start[v], end = start[v + 1]; i < end; ++i) {
        const uint32_t t = list[i] >> 2, k = list[i] & 3u;
        if (t >= n_tris || k > 2u) continue;
        const double* f = face + (size_t)t * 6;
        const double w = f[3 + k];
        x = x + w * f[0], y = y + w * f[1], z = z + w * f[2];
    }
    out[(size_t)v * 3] = x, out[(size_t)v * 3 + 1] = y, out[(size_t)v * 3 + 2] = z;
}

__global__ void __launch_bounds__(256) k_edge_normals(const uint32_t* __restrict__ start, const uint32_t* __restrict__ list, uint32_t n_edges,
                                                      uint32_t n_tris, const double* __restrict__ face, double* __restrict__ out) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    double x = 0.0, y = 0.0, z = 0.0;
    for (uint32_t i = start[e], end = start[e + 1]; i < end; ++i) {
        const uint32_t t = list[i];
        if (t >= n_tris) continue;
        const double* f = face + (size_t)t * 6;
        x = x + f[0], y = y + f[1], z = z + f[2];
    }
    out[(size_t)e * 3] = x, out[(size_t)e * 3 + 1] = y, out[(size_t)e * 3 + 2] = z;
}

} // namespace

// The face terms from the corner table, then every edge's and every vertex's pseudonormal: three launches on `st`, behind
// the launch that wrote the corners.  The ids and lists of T belong to the resident triangles (T.n_tris of them).
void launch_pseudonormals(const DTriCorners* d_corners, const DSignedTables& T, hipStream_t st) {
    if (T.n_tris == 0) return;
    k_face_terms<<<(T.n_tris + 255) / 256, 256, 0, st>>>(d_corners, T.slot, T.n_tris, T.face);
    if (T.n_edges) k_edge_normals<<<(T.n_edges + 255) / 256, 256, 0, st>>>(T.e_start, T.e_list, T.n_edges, T.n_tris, T.face, T.normal);
    if (T.n_vertices)
        k_vertex_normals<<<(T.n_vertices + 255) / 256, 256, 0, st>>>(T.v_start, T.v_list, T.n_vertices, T.n_tris, T.face,
                                                                    T.normal + (size_t)T.n_edges * 3);
}

} // namespace prt
