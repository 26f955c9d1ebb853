// prt_launch.h — every launcher and device-side helper that prt_api.cpp calls, declared once.  Declarations only (but for
// point_query_grid, the launch sizing K6 and K8 share): the file that defines a function includes this header too, so a
// definition that drifts from its declaration (a default argument, a struct passed by value) does not compile.  Scene types are spelled with their precision, so the fp64 and the
// fp32 translation units read the same text.  Default arguments live here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string> // ray_sort's and the device builder's `std::string* err`

#include "../../include/prt.h"
#include "prt_types.h"

namespace prt {
// prt_kernels.hip
int render_blocks_per_cu(bool count, int feat, size_t table_bytes, int stack_depth, bool pad, bool extra, bool rays, bool plain, bool diffuse);
// whether a K3 launch with these values uses the PLAIN form of its kernel (k_render): the one decision, for the occupancy query and the launch
bool render_plain(int feat, bool count, bool rays, int n_lights, int ltri_lds, int jitter, int scramble, int sample_lights);
// ... and its DIFFUSE form on top of the PLAIN one (k_render): render_plain holds, the permutation is the lean one, and the scene's
// material table is all untextured Lambertians and emitters (`all_diffuse`, the host's flag of the table).  fp64 only.
bool render_diffuse(int feat, bool count, bool rays, int n_lights, int ltri_lds, int jitter, int scramble, int sample_lights, bool all_diffuse);
int render_permutation(int feat);
int render_lds_budget(int feat, int stack_depth);
size_t render_table_bytes(int light_lds, int mat_lds, int ltri_lds);
hipError_t launch_trace(const DSceneT<double>& S, const PrtRay* d_rays, size_t n, void* d_out, DCounters* d_ctr, bool count, int mode,
                        int n_cu, hipStream_t st, const uint32_t* d_perm);
// K4 (ray_sort.hip): a permutation of a ray batch in which consecutive rays start close together
size_t ray_sort_scratch_bytes(size_t n, std::string* err);
const uint32_t* ray_sort(const PrtRay* d_rays, size_t n, const float grid_origin[3], const float grid_step[3], void* scratch,
                         size_t scratch_bytes, hipStream_t st, std::string* err);
void launch_render(const DSceneT<double>& S, const DCameraT<double>& C, const DRenderParamsT<double>& P, double* d_partial,
                   DCounters* d_ctr, bool count, int feat, unsigned grid, hipStream_t st, bool rays, bool plain, bool diffuse);
void launch_finalize(const DCameraT<double>& C, const DRenderParamsT<double>& P, const double* d_partial, double* d64, float* d32,
                     hipStream_t st);
void launch_finalize_rays(const DRenderParamsT<double>& P, const double* d_partial, double* d64, float* d32, hipStream_t st);
void launch_accumulate(const DCameraT<double>& C, const DRenderParamsT<double>& P, const double* d_partial, double* d_sum,
                       hipStream_t st);
void launch_resolve(const double* d_sum, size_t n, uint64_t samples, const uint32_t* d_counts, double* d64, float* d32,
                    uint8_t* d8, hipStream_t st);
// adaptive sampling: the active pixels of a round (d_seg holds adapt_segments(owned items) words), and one launch's sums
uint32_t adapt_segments(uint64_t owned_items);
void launch_adapt_select(const DCameraT<double>& C, const DRenderParamsT<double>& P, const DAdaptRule& R, const double* d_sum,
                         const double* d_moment, const uint32_t* d_count, uint32_t* d_seg, int32_t* d_list, uint32_t* d_total,
                         hipStream_t st);
void launch_accumulate_list(const DRenderParamsT<double>& P, const double* d_partial, const int32_t* d_list, uint32_t batch,
                            uint32_t samples, double* d_sum, double* d_moment, uint32_t* d_count, hipStream_t st);
void launch_accum_variance(const double* d_sum, const double* d_moment, const uint32_t* d_count, size_t npx, uint32_t batch,
                           float* d_var, hipStream_t st);
void launch_sample_lights(const DSceneT<double>& S, const double* d_origins, size_t n, uint64_t seed, PrtLightSample* d_out,
                          hipStream_t st);
void launch_tonemap(const float* d_in, size_t n, uint8_t* d_out, hipStream_t st);
void launch_features(const DSceneT<double>& S, const DCameraT<double>& C, uint64_t seed_key, int jitter, int spp, float* albedo,
                     float* normal, float* depth, int32_t* prim, hipStream_t st);
void launch_add_f32(float* dst, const float* src, size_t n, hipStream_t st);
void launch_material_eval(const DSceneT<double>& S, int material, const double* wi, const double* wo, const double* uv, size_t n,
                          uint64_t seed, double* out, hipStream_t st);
void launch_material_scatter(const DSceneT<double>& S, int material, const double* rd, const double* normal, const double* tangent,
                             const double* uv, size_t n, uint64_t seed, double* wi_out, double* att_out, int32_t* ok_out,
                             hipStream_t st);
void launch_texture_value(const DSceneT<double>& S, int texture, const double* uv, size_t n, double* out, hipStream_t st);
// prt_denoise.hip
size_t denoise_scratch_bytes(int w, int h);
void launch_denoise(int w, int h, const float* rgb, const float* albedo, const float* normal, const float* depth,
                    int iterations, int demod, const float sigma[4], void* scratch, float* out, hipStream_t st);
void launch_denoise_guided(int w, int h, const float* rgb, const float* var, const float* albedo, const float* normal,
                           const float* depth, int iterations, int demod, const float sigma[4], void* scratch, float* out,
                           float* out_var, hipStream_t st);
// light_tables.hip: thresholds, buckets and verification of the planned tables of a light update
hipError_t launch_light_tables(const DLightTableBuild& A, hipStream_t st);
// bvh_refit.hip.  RefitCheck: result of the first phase (device memory; the host reads it back once)
struct RefitCheck {
    double lo[3], hi[3]; // bounds of the triangles' padded boxes (HostTri::lo / hi)
    double scale;        // max(1, largest |coordinate| of those boxes)
    uint32_t flags;      // bit 0: a coordinate is not finite or beyond 1e18; bit 1: a light triangle's vertex moved
    uint32_t pad_;
};
static_assert(sizeof(RefitCheck) == 64, "RefitCheck layout (the kernels write it, prt_api.cpp reads it back)");
size_t refit_scratch_bytes();
void launch_refit_check(const double* d_verts, uint32_t n, const DLightTriT<double>* d_ltris, uint32_t n_lights, void* d_scratch,
                        RefitCheck* d_out, hipStream_t st, const double* d_normals, double* d_gather_v, double* d_gather_n);
void launch_refit_tris(const double* d_verts, const double* d_normals, const uint32_t* d_order, uint32_t n, void* d_tris,
                       uint32_t tri_stride, DTriShadeT<double>* d_shade, float* d_tbox, const double origin[3], double delta,
                       hipStream_t st);
void launch_refit_parents(const DNode* d_nodes, uint32_t n_nodes, uint32_t* d_parent, hipStream_t st);
void launch_prim_boxes(const double* d_verts, uint32_t n, float* d_boxes, const double origin[3], double delta, hipStream_t st);
void launch_permute_shade(const DTriShadeT<double>* d_shade_old, const uint32_t* d_old_order, const uint32_t* d_new_order,
                          uint32_t n, uint32_t* d_inv, DTriShadeT<double>* d_shade_new, hipStream_t st);
hipError_t launch_refit_boxes(DNode* d_nodes, uint32_t n_nodes, const uint32_t* d_parent, uint32_t* d_cnt, const float* d_tbox,
                              uint32_t n_tris, const float step[3], hipStream_t st);
void launch_refit_sah(const DNode* d_nodes, uint32_t n_nodes, const float origin[3], const float step[3], void* d_scratch,
                      double* d_out, hipStream_t st);
// bvh_build_gpu.hip: the device builder on boxes that are on the device already, on a stream (build_bvh_device: prt_host.h,
// which also defines the two structs)
struct PrimBox;
struct DeviceBVH;
bool build_bvh_device_boxes(const PrimBox* d_boxes, const float box_origin[3], size_t n, DeviceBVH& out, std::string* err,
                            hipStream_t st);
void launch_gather_tris(const DTriT<double>* tri_in, const DTriShadeT<double>* shade_in, const uint32_t* order, uint32_t n,
                        void* tri_out, uint32_t tri_out_stride, DTriShadeT<double>* shade_out, hipStream_t st);
// The grid of a point-query launch (K6, K8) with `lds` bytes of dynamic LDS for the lanes' stacks; the kernel `k` is allowed
// that much where it is more than a launch may ask for by default.  plain: a block per PRT_BLOCK queries; otherwise
// persistent waves, as many blocks as can be resident (LDS: 160 KB per CU; registers: at most four waves per SIMD).
// (The one definition in this header: both files size their launch by it.)
inline hipError_t point_query_grid(const void* k, size_t n, size_t lds, int n_cu, bool plain, unsigned& grid) {
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const size_t want = (n + PRT_BLOCK - 1) / PRT_BLOCK;
    const size_t per_cu = std::max<size_t>(1, std::min<size_t>(4, (160u * 1024u) / lds));
    grid = (unsigned)(plain ? want : std::min<size_t>(want, (size_t)std::max(n_cu, 1) * per_cu));
    return hipSuccess;
}
// closest_point.hip: the corner table of a scene that answers distance queries, and K6
void launch_gather_corners(const double* d_verts, const uint32_t* d_order, uint32_t n, DTriCorners* d_out, hipStream_t st);
hipError_t launch_closest_point(const DSceneT<double>& S, const DTriCorners* d_corners, const PrtPointQuery* d_q, size_t n,
                                PrtClosestPoint* d_out, DCounters* d_ctr, bool count, int stack_depth, int n_cu, bool plain,
                                hipStream_t st);
// ... and K6 with the sign of the nearest feature's pseudonormal (prt_signed_distance): the persistent-wave schedule only
struct DSignedTables;
hipError_t launch_signed_distance(const DSceneT<double>& S, const DTriCorners* d_corners, const DSignedTables& T, const PrtPointQuery* d_q,
                                  size_t n, PrtSignedDistance* d_out, DCounters* d_ctr, bool count, int stack_depth, int n_cu,
                                  hipStream_t st);
// pseudonormals.hip: the device tables of a scene that answers signed distance queries (all in description order; ids
// and lists from mesh_topology.cpp, uploaded once per topology), and the refresh of `face` and `normal` from the corner table
struct DSignedTables {
    const uint32_t* slot = nullptr;    // [n_tris][6]: index into `normal` of edge v0v1, v1v2, v2v0, vertex v0, v1, v2; 0xffffffff: none
    const uint32_t* v_start = nullptr; // CSR vertex -> (prim << 2 | corner), ascending
    const uint32_t* v_list = nullptr;
    const uint32_t* e_start = nullptr; // CSR edge -> prim, ascending
    const uint32_t* e_list = nullptr;
    double* face = nullptr;            // [n_tris][6]: the unit normal, the interior angles at v0, v1, v2 (zeros: contributes nothing)
    double* normal = nullptr;          // [n_edges + n_vertices][3]: en of every edge, then vn of every vertex
    uint32_t n_tris = 0, n_vertices = 0, n_edges = 0;
};
void launch_pseudonormals(const DTriCorners* d_corners, const DSignedTables& T, hipStream_t st);
// winding_number.hip: the moments table of a scene that answers winding-number queries ([n_nodes][4], one record per child
// slot, zeros for an unused slot; include/prt.h has the formulas), its bottom-up refresh with the refit's parent array and
// counters, and K8
struct alignas(64) DWindingMoment {
    double N[3]; // the sum of the area vectors below the slot
    double c[3]; // the area-weighted centroid
    double r;    // every corner below the slot lies within r of c
    double A;    // the area
};
hipError_t launch_winding_moments(const DNode* d_nodes, uint32_t n_nodes, const uint32_t* d_parent, uint32_t* d_cnt,
                                  const DTriCorners* d_corners, uint32_t n_tris, DWindingMoment* d_mom, hipStream_t st);
hipError_t launch_winding_number(const DSceneT<double>& S, const DTriCorners* d_corners, const DWindingMoment* d_mom, const PrtPointQuery* d_q,
                                 size_t n, double beta, double* d_out, DCounters* d_ctr, bool count, int stack_depth, int n_cu,
                                 hipStream_t st);
// K7 (multi_hit.hip / multi_hit_f32.hip): one batch of rays, k records per ray into d_out (32-byte aligned), d_after null
// or one cursor per ray, d_perm K4's order or null
hipError_t launch_multi_hit(const DSceneT<double>& S, const PrtRay* d_rays, const PrtHitCursor* d_after, size_t n, int k, PrtHit* d_out,
                            DCounters* d_ctr, bool count, int n_cu, hipStream_t st, const uint32_t* d_perm);
} // namespace prt

// fp32 fast mode (prt_kernels_f32.hip): K1 and K3 on float records derived from the resident fp64 ones
namespace prt32 {
int render_blocks_per_cu(bool count, int feat, size_t table_bytes, int stack_depth, bool pad, bool extra, bool rays, bool plain, bool diffuse);
// whether a K3 launch with these values uses the PLAIN form of its kernel (k_render): the one decision, for the occupancy query and the launch
bool render_plain(int feat, bool count, bool rays, int n_lights, int ltri_lds, int jitter, int scramble, int sample_lights);
int render_permutation(int feat);
int render_lds_budget(int feat, int stack_depth);
size_t render_table_bytes(int light_lds, int mat_lds, int ltri_lds);
hipError_t launch_trace(const DSceneT<float>& S, const PrtRay* d_rays, size_t n, void* d_out, DCounters* d_ctr, bool count, int mode,
                        int n_cu, hipStream_t st, const uint32_t* d_perm);
void launch_render(const DSceneT<float>& S, const DCameraT<float>& C, const DRenderParamsT<float>& P, double* d_partial,
                   DCounters* d_ctr, bool count, int feat, unsigned grid, hipStream_t st, bool rays, bool plain, bool diffuse);
void launch_convert_tris(const void* in, uint32_t in_stride, uint32_t n, void* out, uint32_t out_stride, hipStream_t st);
void launch_convert_shade(const DTriShadeT<double>* in, uint32_t n, DTriShadeT<float>* out, hipStream_t st);
void launch_convert_reals(const double* in, size_t n, float* out, hipStream_t st);
hipError_t launch_multi_hit(const DSceneT<float>& S, const PrtRay* d_rays, const PrtHitCursor* d_after, size_t n, int k, PrtHit* d_out,
                            DCounters* d_ctr, bool count, int n_cu, hipStream_t st, const uint32_t* d_perm);
} // namespace prt32
