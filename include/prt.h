/*
 * prt.h — C ABI of libprt_hip.so, the MI355X (gfx950) path-tracing hot path.
 *
 * This is the drop-in boundary for the reference's per-pixel / per-sample hot path
 *     Camera::Render -> RayColor -> BVHNode::Hit -> Triangle::Hit / AABB::Hit
 * (reference: Source/Camera.cpp:21-204, Source/BVH.cpp:51-61, Source/Triangle.cpp:54-83,
 *  Source/AABB.cpp:38-64).  The reference has no FFI layer of its own; the
 * entry points below are what a binding for that path would call:
 *
 *   prt_scene_create      replaces the object graph main.cpp:36-45 builds
 *                         (Mesh/Triangle ctor precompute Source/Triangle.cpp:11-53,
 *                          two-level BVHNode build Source/BVH.cpp:6-49, lights list main.cpp:40-45)
 *   prt_trace_closest     replaces world.Hit(ray, Interval(tmin,tmax), record)
 *   prt_trace_occluded    the same call where only its bool result is wanted (any-hit)
 *                         (Source/HittableList.h:26-39 -> Source/BVH.cpp:51-61)
 *   prt_render            replaces Camera::Render(world, lights)      (Source/Camera.cpp:21-73)
 *   prt_render_device     same, framebuffer left in device memory for an RCCL reduce
 *   prt_ray_color         replaces RayColor(ray, maxDepth, world, lights) (Source/Camera.cpp:119-204) for a batch of the
 *                         caller's own rays: probes, lightmap texels, camera models the reference lacks
 *   prt_render_multi      same over several GPUs of this process: tiles + one RCCL reduce of the fp32 framebuffer
 *                         (replaces the std::thread row bands of Source/Camera.cpp:46-71)
 *   prt_closest_point     new: for a batch of points, the nearest point of the mesh and its distance, against the same resident
 *                         BVH (the reference has no point query); needs prt_scene_set_distance_queries
 *   prt_trace_multi       new: the first k hits along each ray of a batch, in (t, prim) order, with an exact paging cursor
 *                         (the reference reports one hit per world.Hit call)
 *   prt_sample_lights     replaces lights.Sample(origin, record, pdf) (Source/HittableList.h:44-59,
 *                          Source/BVH.cpp:62-67,86-100, Source/Triangle.cpp:84-93) — test hook
 *   prt_scene_refit       new vertex positions for a resident scene: records and BVH boxes follow on the GPU, the tree's
 *                         topology stays (the reference rebuilds its BVHNode graph instead, Source/BVH.cpp:7-48)
 *   prt_scene_rebuild     new vertex positions and a NEW tree of them from the device builder; textures, materials and
 *                         light tables stay resident
 *   prt_get_counters      rays / node fetches / triangle tests / kernel ms of the last call
 *   prt_accum_*           progressive, resumable rendering: the same frame built up over several calls
 *                         (replaces a ladder of separate Camera::Render calls at rising samplesPerPixel);
 *                         the *_adaptive ones stop each pixel once its noise estimate meets a tolerance
 *   prt_render_features   first-hit albedo / normal / depth / triangle per pixel (the inputs of a denoiser)
 *   prt_denoise           edge-aware a-trous filter guided by those; prt_accum_*_denoised: an accumulator's frame, denoised
 *   prt_denoise_guided    the same filter with SVGF-style colour weights from a per-pixel variance (prt_accum_variance)
 *
 * Conventions: every function returns 0 on success or a negative PRT_E_* code and never throws;
 * prt_last_error() returns a thread-local message for the last failure.  All input buffers are
 * owned by the caller and may be freed as soon as the call returns.  Handles are opaque.  One
 * host thread per device; calls on different handles are independent.  No CPU fallback exists:
 * without a HIP device every compute entry point fails with PRT_E_NO_DEVICE.
 */
#ifndef PRT_H
#define PRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_ABI_VERSION 6

/* error codes */
#define PRT_OK 0
#define PRT_E_INVALID (-1)    /* bad argument / inconsistent scene description / non-finite vertex coordinate */
#define PRT_E_NO_DEVICE (-2)  /* no HIP device visible */
#define PRT_E_HIP (-3)        /* a HIP runtime call failed (message has the HIP error string) */
#define PRT_E_OOM (-4)        /* host or device allocation failed */
#define PRT_E_LIMIT (-5)      /* scene exceeds a compiled-in limit (BVH depth, leaf encoding, 2^26 BVH nodes) */

/* Material kinds — reference enum MaterialType, Source/Material.h:48-51 */
#define PRT_MAT_LAMBERTIAN 0    /* Source/Material.h:101-155 */
#define PRT_MAT_PHONG 1         /* PhoneReflectance, Source/Material.h:172-330 */
#define PRT_MAT_MIRROR 2        /* PerfectMirror, Source/Material.h:332-366 */
#define PRT_MAT_COOKTORRANCE 3  /* Source/Material.h:368-521 */
#define PRT_MAT_DIFFUSE_LIGHT 4 /* Source/Material.h:157-170 */
#define PRT_MAT_DEBUG 5         /* Source/Material.h:523-535 (emits its albedo) */
#define PRT_MAT_EMPTY 6         /* Source/Material.h:537-540 */

typedef struct PrtMaterial {
    int32_t type;      /* PRT_MAT_* */
    int32_t texture;   /* index into PrtSceneDesc.textures for the Kd map, or -1 (SolidColor) */
    double kd[3];      /* Lambertian albedo / Phong Kd / Debug albedo */
    double ks[3];      /* Phong Ks (ignored when texture >= 0: reference stores mapKd in both, Material.h:178-181) */
    double ns;         /* Phong exponent */
    double emission[3];/* DiffuseLight radiance (XML <light radiance>, Source/Model.cpp:332-360) */
    double eta[3];     /* CookTorrance conductor eta */
    double k[3];       /* CookTorrance conductor k */
    double alpha_x, alpha_y; /* CookTorrance roughness */
} PrtMaterial;

/* 8-bit interleaved texels exactly as stbi_load returns them (Source/Texture.cpp:10-21). */
typedef struct PrtTexture {
    int32_t width, height, channels, reserved;
    const uint8_t* data; /* width*height*channels bytes; NULL => reference's "missing" colour (0,1,1) */
} PrtTexture;

/*
 * Scene = list of meshes; a mesh = contiguous triangle range + one material
 * (reference: Mesh, Source/Triangle.h:36-43; one material per shape, Source/Model.cpp:118).
 * Triangle order inside a mesh and mesh order are significant: they are the input order of the
 * reference's std::sort-based light-tree build, which fixes the NEE light CDF order.
 */
typedef struct PrtSceneDesc {
    uint64_t n_tris;
    const double* vertices;  /* [n_tris][3 verts][xyz] */
    const double* normals;   /* [n_tris][3][xyz] vertex normals (degenerate-face fallback only) or NULL */
    const double* texcoords; /* [n_tris][3][uv] or NULL (all zero) */
    uint32_t n_meshes;
    uint32_t n_materials;
    const uint64_t* mesh_first_tri; /* [n_meshes+1], ascending, last == n_tris */
    const int32_t* mesh_material;   /* [n_meshes] index into materials */
    const PrtMaterial* materials;
    uint32_t n_textures;
    uint32_t flags;          /* PRT_SCENE_* bits; 0 = defaults */
    const PrtTexture* textures;
    /* The `lights` argument of Camera::Render(world, lights) (Source/Camera.h:27): indices of the meshes that were
     * added to the lights list, in that order.  NULL = what main.cpp:40-45 builds — every mesh whose material
     * HasEmission(), in mesh order.  A non-NULL pointer with n_light_meshes == 0 is an empty list (no NEE). */
    const int32_t* light_meshes;
    uint32_t n_light_meshes;
    uint32_t reserved;
} PrtSceneDesc;

/* Build the traversal BVH on the GPU at prt_scene_upload time instead of on the host at create time
 * (reference: BVHNode constructors, Source/BVH.cpp:7-48, always CPU).  Results do not depend on the
 * builder; the host builder stays the default because its trees traverse a few percent faster. */
#define PRT_SCENE_DEVICE_BVH 1u

/* Public camera fields of the reference, Source/Camera.h:14-24. */
typedef struct PrtCamera {
    int32_t width, height;
    double fovy; /* degrees */
    double eye[3], look_at[3], up[3];
} PrtCamera;

#define PRT_PRECISION_F64 0 /* reference arithmetic (glm::dvec3 everywhere) */
/* fp32 fast mode: the same kernels with every real number a float (48-byte triangle records, hardware rcp / rsq / sqrt).
 * Same random streams, same tree; results agree with PRT_PRECISION_F64 within the second tolerance tier (hits
 * |dt|/t <= 1e-5, images statistically: knife-edge branches differ), not to 1e-9.  The float tables are derived from
 * the resident fp64 ones on the first call that asks for them (that call is synchronous). */
#define PRT_PRECISION_F32 1

typedef struct PrtRenderParams {
    int32_t spp;           /* Camera::samplesPerPixel */
    int32_t max_depth;     /* Camera::maxDepth (maxDepth+1 path vertices, Camera.cpp:121) */
    double russian_roulette; /* Camera::russianRoulette */
    int32_t sample_lights; /* Camera::bSampleLights */
    int32_t precision;     /* PRT_PRECISION_* */
    double background[3];  /* Camera::background */
    uint64_t seed;         /* per-sample RNG key = (seed, j*W+i, s) */
    int32_t tile_size;     /* multi-GPU tile edge in pixels (0 => 32) */
    int32_t rank, nranks;  /* this device renders tiles k with k % nranks == rank; others stay 0 */
    int32_t sample_chunks; /* 0 => auto; partial sums per pixel are combined in fixed order */
    int32_t pixel_jitter;  /* 0 = reference behaviour (pixel centre).  1 = the anti-aliasing the reference has
                              commented out (Camera.cpp:110-111): SampleSquare() offset, drawn per sample as
                              the first two numbers of the sample's stream (offset.y first, offset.x second) */
    int32_t reserved;      /* must be 0 */
} PrtRenderParams;

/* One ray of a batch: world.Hit(Ray(o,d), Interval(tmin,tmax)). */
typedef struct PrtRay {
    double o[3];
    double tmin;
    double d[3];
    double tmax;
} PrtRay;

/* HitRecord subset that identifies the hit (Source/Hittable.h:17-28). */
typedef struct PrtHit {
    double t;      /* HitRecord::time; +inf on miss */
    double alpha;  /* barycentric of v1 (Triangle.cpp:69) */
    double beta;   /* barycentric of v2 (Triangle.cpp:70) */
    int32_t prim;  /* triangle index in PrtSceneDesc order, -1 on miss */
    int32_t front; /* HitRecord::bFrontFace */
} PrtHit;

/* lights.Sample() result (test hook). */
typedef struct PrtLightSample {
    double position[3];
    double normal[3]; /* face-forwarded against (p - origin), Triangle.cpp:89-90 */
    double pdf;       /* 1 / total light area */
    int32_t prim;
    int32_t front;
} PrtLightSample;

typedef struct PrtCounters {
    uint64_t rays_closest;  /* camera + continuation traversals executed (the camera ray of a pixel is traced once per work item, not per sample) */
    uint64_t rays_shadow;   /* NEE visibility traversals */
    uint64_t node_fetches;  /* BVH node records read (counting runs only; PrtBvhInfo.node_bytes each) */
    uint64_t tri_tests;     /* triangle plane / interval tests = the first 32 bytes (n, D) of a 96-byte record (counting runs only) */
    uint64_t samples;       /* camera samples of the call (pixels rendered x spp) */
    double kernel_ms;       /* hipEvent time of the dominant kernel of the last call */
    uint64_t bvh_nodes;     /* static: nodes in the flattened tree */
    uint64_t bvh_depth;     /* static: max depth */
    uint64_t inner_rounds;  /* counting runs: wave-level node-visit rounds (64 lanes each) */
    uint64_t leaf_rounds;   /* counting runs: wave-level leaf rounds */
    uint64_t refills;       /* counting runs: wave-level shade/refill passes */
    uint64_t tri_full;      /* counting runs: tests that passed the interval check and fetched the 64 bytes of edge functions */
} PrtCounters;

/* Which builder made the traversal BVH and what it cost. */
typedef struct PrtBvhInfo {
    uint64_t n_nodes;
    uint32_t depth;
    uint32_t built_on_device;
    double build_ms;  /* host builder: wall time inside prt_scene_create; device builder: HIP-event time */
    double sort_ms, tree_ms, split_ms; /* device builder phases: Morton sort / box segment tree / SAH levels */
    uint32_t node_bytes; /* size of one node record in HBM */
    uint32_t width;      /* children per node */
    uint32_t tri_bytes;  /* payload of one intersection record: 32 (plane: n, D) + the part read after the interval test */
    uint32_t tri_stride; /* bytes between records in HBM once uploaded (0 before): tri_bytes, or 128 for scenes that stream from HBM */
    /* image textures as resident on the device (0 before upload; ImageTexture::Value, Source/Texture.cpp:22-71).  A scene's
     * textures are stored as bilinear footprints (per texel cell the four taps of a lookup: 128 bytes per texel, one line per
     * lookup) while ALL of them together stay within 256 MiB; a scene beyond that keeps plain texel arrays (24 bytes per
     * texel).  The fp32 fast mode adds a float copy of half the size on first use. */
    uint64_t texture_bytes;           /* fp64 bytes of all texel arrays */
    uint64_t texture_footprint_bytes; /* ... of which footprint records */
    uint32_t texture_layouts;         /* 0: no textures; 1: footprints; 2: plain texel arrays (one layout per scene) */
    /* how the fp64 render kernel (K3) of this scene is launched (0 before upload) */
    uint32_t render_blocks_per_cu;    /* resident 256-thread blocks per CU (= waves per SIMD) of the production instantiation */
    uint32_t render_blocks_wanted;    /* ... the register allocation of the scene's material permutation leaves room for */
    uint32_t lds_materials, lds_light_nodes, lds_light_tris; /* shading tables K3 stages in LDS (0: read from global memory) */
    uint32_t stack_need;              /* traversal stack entries this tree can need (<= 40, the builders' bound) */
    /* which production instantiation of K3 a render of this scene launches: bits 0-7 the fp64 kernel, bits 8-15 the fp32 one
     * (0 until the first PRT_PRECISION_F32 call has made the fp32 tables); each byte is a PRT_VARIANT_* word (0 before upload) */
    uint32_t render_variant;
} PrtBvhInfo;

/* PrtBvhInfo.render_variant, per precision byte */
#define PRT_VARIANT_PERM_MASK 0x07u /* material permutation: 0 lean, 1 textures, 2 Phong, 4 CookTorrance, 7 all of them */
#define PRT_VARIANT_LLDS 0x08u      /* shading tables staged in LDS */
#define PRT_VARIANT_PAD 0x10u       /* intersection records padded to one cache line each */
#define PRT_VARIANT_EXTRA 0x20u     /* light tables or plain texel arrays (the scene's kernels compiled with both paths) */
#define PRT_VARIANT_VALID 0x80u     /* the byte describes a kernel */

typedef struct PrtScene PrtScene;

int prt_abi_version(void);
/* 1 when this build reads the developer / test environment hooks (PRT_TUNE_*, PRT_TEST_*; -DPRT_DEV_HOOKS=1 builds only —
 * libprt_hip_dev.so of the test suite).  The shipped libprt_hip.so returns 0 and reads no environment variable. */
int prt_dev_hooks(void);
/* Developer query (dev-hooks build): the form of the render kernel (K3) that this library's most recent launch used, in any
 * scene and precision — PRT_RENDER_FORM_PLAIN: the instantiation compiled for a frame with default settings (no pixel
 * jitter, light sampling on, a scene with emitters whose light triangles are staged in LDS, no pixel list, no counting,
 * no ray batch); PRT_RENDER_FORM_GENERIC: every other launch, and every launch under PRT_TUNE_GENERIC=1.  The two forms
 * compute the same frame bit for bit.  The shipped libprt_hip.so keeps no record and returns PRT_RENDER_FORM_UNKNOWN, as
 * does the dev-hooks build before its first launch. */
#define PRT_RENDER_FORM_UNKNOWN 0
#define PRT_RENDER_FORM_GENERIC 1
#define PRT_RENDER_FORM_PLAIN 2
int prt_last_render_form(void);
/* Developer query (dev-hooks build): the sub-form of that launch.  PRT_RENDER_SUBFORM_DIFFUSE: a PLAIN launch (prt_last_render_form
 * says PLAIN) of the lean fp64 kernel in a scene whose material table holds nothing but untextured Lambertians and emitters,
 * none of which skips light sampling: the material tests of Eval and Scatter are compiled out as well.  PRT_RENDER_SUBFORM_NONE:
 * every other launch, every launch under PRT_TUNE_NO_DIFFUSE=1 (a qualifying launch then uses the PLAIN kernel) and under
 * PRT_TUNE_GENERIC=1.  All forms compute the same frame bit for bit.  The shipped libprt_hip.so returns
 * PRT_RENDER_SUBFORM_UNKNOWN, as does the dev-hooks build before its first launch. */
#define PRT_RENDER_SUBFORM_UNKNOWN 0
#define PRT_RENDER_SUBFORM_NONE 1
#define PRT_RENDER_SUBFORM_DIFFUSE 2
int prt_last_render_subform(void);
const char* prt_last_error(void);
int prt_device_count(int* n);

int prt_scene_create(const PrtSceneDesc* desc, PrtScene** out);
void prt_scene_destroy(PrtScene* scene);
/* Upload nodes / triangles / materials / textures / light tree to `device` (the tree was built in prt_scene_create on
 * the host, or is built here on the GPU with PRT_SCENE_DEVICE_BVH).  All or nothing: on failure nothing stays resident
 * and the scene is back in the not-uploaded state. */
int prt_scene_upload(PrtScene* scene, int device);

/* New vertex positions ([n_tris][3][xyz], same layout as PrtSceneDesc.vertices; normals may be NULL) for a
 * scene whose topology, materials and texture coordinates stay as created: re-runs the Triangle constructor
 * precompute and the light tree; on an uploaded scene the BVH is REBUILT on the GPU (PRT_SCENE_DEVICE_BVH
 * path: 4 ms per 126k triangles, 17 ms per 8M).  Limitation: there is no topology-preserving refit (the
 * reference has none either — it rebuilds, Source/BVH.cpp:7-48); a caller that moves geometry every frame pays
 * the rebuild plus a re-upload of the triangle records each time.  (prt_scene_refit below is the in-place alternative for
 * an uploaded scene whose emitters stay put.)  Replaces every host position: clears the stale mark prt_scene_refit_device sets.
 * This call takes HOST positions and goes through prt_scene_upload, which frees and re-sends every table (materials,
 * light tables, textures) and drops the fp32 tables.  A caller whose positions are on the device and whose emitters stay
 * put refits every frame and, when PrtRefitInfo.sah_ratio says so, rebuilds on the device with prt_scene_rebuild_device
 * (below): a new tree while everything else stays resident. */
int prt_scene_update_vertices(PrtScene* scene, const double* vertices, const double* normals);

/*
 * In-place geometry update of an UPLOADED scene with a BVH refit on the GPU: new positions for every triangle
 * ([n_tris][3][xyz] fp64, the layout of PrtSceneDesc.vertices; normals in the same layout or NULL), the acceleration
 * structure follows without a rebuild and nothing is reloaded.
 *
 * Scene state.  PRT_E_NO_DEVICE unless the scene is uploaded.  Topology, materials, texture coordinates, the leaf order
 * and every node's refs stay as they are.  What changes is the geometry-derived data: the intersection records (the
 * Triangle constructor precompute, Source/Triangle.cpp:11-53, incl. the degenerate-face fallback to the vertex normals),
 * the tangent of the shading records, and the boxes of every resident node array (the 32-entry collapse of a deep
 * host-built tree included: it shares the leaf order).  Host-built and device-built trees, 96- and 128-byte record
 * strides.  Nothing is freed or re-uploaded: textures, materials, light tables, LDS sizing, render_variant, stack_need
 * and n_nodes are untouched.  The first refit after an upload allocates its own working arrays (28 bytes per triangle,
 * 8 per node) and keeps them.
 * Grid.  The quantisation grid of the 16-bit boxes (origin, step, the slab test's scale) is recomputed from the new scene
 * bounds on every refit by the builders' rule, so a scene that grows, shrinks or moves far away keeps tight,
 * conservative boxes.
 * Emitters stay in place by default: if a vertex of any triangle of a light mesh differs bitwise from the resident
 * light triangle, the call fails with PRT_E_INVALID (use prt_scene_update_vertices, which rebuilds the light tree) -
 * unless the scene allows it with prt_scene_set_dynamic_lights (below): then the light tree, its records and its O(1)
 * tables follow on the device, and the call has a second host synchronisation.
 * A vertex coordinate that is not finite or beyond 1e18 is PRT_E_INVALID, as in prt_scene_update_vertices; the check
 * runs on the device, where the coordinates are.
 * All or nothing.  Both checks run in a read-only first phase over the new vertices, which also reduces the scene
 * bounds; one small read-back then decides before anything resident is written.  A refused refit leaves the scene, its
 * generation and its frames exactly as they were.  (A HIP error once the writing phases have been queued is no refusal:
 * as in prt_scene_update_vertices the generation and the grid are already the new ones, the records may be partly
 * rewritten, and the scene wants a prt_scene_update_vertices before it is used again.)
 * Ordering.  That read-back is the ONE host synchronisation of a call (it waits for the first phase on hip_stream, not
 * for the renders in flight).  The writing phases then wait, on hip_stream, for the in-flight work of both call slots and
 * of the last prt_render_features* call, and every later call on any stream waits for the refit's end.  The vertex
 * buffers must stay valid until the work on hip_stream has completed.
 * Generation.  A successful refit bumps the scene's generation: accumulators and their feature caches behave as after
 * prt_scene_update_vertices (PRT_E_INVALID until prt_accum_reset).
 * fp32 tables, if they exist, are re-derived on the device from the new fp64 records.
 * Host geometry.  prt_scene_refit (host pointers) also updates the scene's host triangles, so a later prt_scene_upload or
 * prt_scene_update_vertices sees the new geometry (that upload builds a fresh tree on the GPU).  prt_scene_refit_device
 * marks the host geometry stale: while it is, prt_scene_upload is refused with PRT_E_INVALID; prt_scene_update_vertices
 * and prt_scene_refit replace every host position and clear the mark.
 * Quality.  A refit keeps the tree's topology, so the tree decays as the geometry deforms; PrtRefitInfo.sah_ratio is the
 * caller's signal that a rebuild is due: prt_scene_rebuild* below (a new tree, nothing re-uploaded) or
 * prt_scene_update_vertices.  The library never rebuilds on its own.
 * With PRT_TEST_DUMP_BVH (dev-hooks build) the refitted tree is dumped after every successful refit (synchronous).
 */
typedef struct PrtRefitInfo {
    uint64_t refits;      /* successful refits since the last upload */
    double records_ms;    /* hipEvent time of the last refit's triangle set-up (with the fp32 re-derivation, if any) */
    double boxes_ms;      /* ... of its box refit over every resident node array, with the SAH reduction */
    double sah_ratio;     /* SAH cost of the wide tree now / at the last build (node 1.0, triangle 1.5: the builders'
                             constants); 1.0 before the first refit */
    float grid_origin[3]; /* the current quantisation grid: box coordinate = grid_origin + q * grid_step */
    float grid_step[3];
    float slab_scale;     /* the largest extent of that grid (the slab test's pad scale) */
    uint32_t host_stale;  /* 1 after prt_scene_refit_device until every host position is replaced */
} PrtRefitInfo;
int prt_scene_refit(PrtScene* scene, const double* vertices, const double* normals); /* host pointers */
int prt_scene_refit_device(PrtScene* scene, const void* d_vertices, const void* d_normals, void* hip_stream);
/* Synchronous: waits for the last refit's end (the times and the SAH ratio come from the device). */
int prt_scene_refit_info(const PrtScene* scene, PrtRefitInfo* out);

/*
 * Device-side REBUILD of the acceleration structure of an UPLOADED scene from new positions: the inputs and the read-only
 * first phase are those of prt_scene_refit* (same layouts, same PRT_E_NO_DEVICE, same refusals: a coordinate that is not
 * finite or beyond 1e18, a moved emitter vertex - PRT_E_INVALID, use prt_scene_update_vertices or allow it with
 * prt_scene_set_dynamic_lights), but the result is a NEW
 * topology from the device builder, while everything that does not depend on the positions stays resident.  The
 * pattern: prt_scene_refit_device every frame, prt_scene_rebuild_device when PrtRefitInfo.sah_ratio says the tree has
 * decayed; the library does not decide that for the caller.
 *
 * What is replaced.  The device builder (PRT_SCENE_DEVICE_BVH's) runs on the fp32 boxes of the new positions, computed
 * on the device by the rule of the builders relative to the new grid origin.  The node array (n_nodes may change) and the
 * leaf order are replaced; the shading records (uv, material, prim) are permuted on the device from the old leaf
 * position of each triangle to its new one; the intersection records and the tangents are rewritten from the new
 * vertices through the new order; the quantisation grid and the slab test's scale are the builder's.  Textures,
 * materials, light tables, the record stride and the call slots are untouched: nothing is re-uploaded.
 * Derived state.  stack_need is recomputed as at upload and the render kernels are sized again (the fp32 ones too if
 * the fp32 tables exist: their records are re-converted, their tree is the new one).  The 32-entry collapse of a deep
 * host-built tree is dropped: a device-built tree has none.  PrtBvhInfo afterwards reports built_on_device = 1, the new
 * n_nodes, depth, stack_need and render_variant, and the builder's build_ms / sort_ms / tree_ms / split_ms.  The refit
 * state follows the new topology: sah_ratio is 1.0 again and is measured against the new tree; refits keeps counting.
 * Generation and host geometry: as for the refit.  The generation is bumped (accumulators: PRT_E_INVALID until
 * prt_accum_reset); prt_scene_rebuild updates the host triangles, prt_scene_rebuild_device marks them stale.
 * Ordering.  The call waits for the last refit; its writing phase waits, on hip_stream, for the work in flight on both
 * call slots and for the last prt_render_features* call.  Unlike the refit it is SYNCHRONOUS: it returns when the new tree
 * is resident (the builder reads counts back, and the old node array is freed).  The kernels of the device form run on
 * hip_stream, and every later call orders itself after it.
 * All or nothing.  The new tree, the new order and every new allocation are made BEFORE anything resident is written: a
 * refusal, an allocation failure or a HIP error up to that point frees what the call made and leaves the scene, its
 * generation, its frames and prt_scene_refit_info exactly as they were.  Afterwards the refit's wording applies: the
 * generation and the grid are already the new ones.
 * Small scenes.  The builder needs two triangles: with fewer the call behaves as prt_scene_refit* does (no triangles:
 * PRT_OK).
 * With PRT_TEST_DUMP_BVH (dev-hooks build) the rebuilt tree is dumped; PRT_TEST_FAIL_REBUILD=k (dev-hooks build) makes
 * the k-th allocation of a rebuild (from 0; the builder's run counts as one) report PRT_E_OOM.
 */
int prt_scene_rebuild(PrtScene* scene, const double* vertices, const double* normals); /* host pointers */
int prt_scene_rebuild_device(PrtScene* scene, const void* d_vertices, const void* d_normals, void* hip_stream);

/*
 * Moving emitters.  Off by default: prt_scene_refit* / prt_scene_rebuild* refuse a moved emitter vertex as described above,
 * with the same code, message and single host synchronisation.  On: they accept it, and after a successful call the light
 * state of the scene is what a fresh scene created from the new vertices has - the CDF order (prt_scene_light_order), every
 * light record (vertices, normal, area, pdf), the total area, the tree and the O(1) table words, bit for bit - so
 * prt_sample_lights, frames, prt_ray_color and accumulators follow.  Which meshes are lights does not change.
 * Why it is cheap: the SHAPE of a mesh's light subtree depends only on its triangle count (every span is split at its
 * middle), so a motion changes which triangle sits at which leaf and the areas; with one or two light meshes every
 * resident light array keeps its size and layout (with three or more, the order of the meshes in the top of the tree
 * follows the motion, and the tables' places with it: see "Layout exceptions").  The host does what defines the order - the Triangle precompute of the emitter triangles, the
 * reference's two std::sort passes, areas and pdfs (a sort per tree level: n log^2 n on the emitter triangles) - and plans the tables; the device
 * fills the thresholds and buckets and verifies them (the host's verification points; its random draws are replaced by a
 * sub-stream per lane).
 * Phases of a call.  No emitter vertex differs bitwise: the call is the one described above (one host synchronisation),
 * except that its read-back also carries the emitters' new vertices: 72 bytes per EMITTER triangle (144 with normals) - it
 * scales with the emitter triangles, not with the scene's.  One differs: at most TWO host synchronisations, that read-back
 * and the verification flag (which brings the filled table words, 4 bytes each, for the host's copy); a scene whose
 * lights have no table (no clean subtree of 16 or more light triangles) has only the first.  The refit's ordering rules apply to the
 * light writes unchanged.
 * All or nothing.  The scene keeps two device copies of the light arrays: the new nodes, records and tables are built
 * and verified in the spare one while calls in flight read the resident one, and the two are exchanged in the call's
 * writing phase.  A refusal (a non-finite coordinate anywhere, an allocation failure) leaves lights, frames and
 * prt_scene_refit_info exactly as they were.
 * Layout exceptions (PrtLightUpdateInfo.relaid = 1).  The plan of the new geometry differs from the resident layout - the
 * meshes of a list of three or more changed places, or a subtree whose area gives no finite positive bucket width gets
 * no table and its children are tried - or the device verification fails: then the scene keeps the full tree and no tables (tables_dropped = 1), as the host builder
 * decides.  Either way larger arrays are made before anything is written and the render kernels are sized again
 * (PrtBvhInfo.lds_light_nodes / lds_light_tris / render_variant may change).
 * fp32 tables, if they exist, are re-derived (the small light tables on the host).  The host triangles of the EMITTERS are
 * always updated (their vertices are on the host anyway); PrtRefitInfo.host_stale keeps its meaning for the rest.  The
 * generation is bumped as for any refit.
 * PRT_TEST_FAIL_LIGHT_VERIFY=1 (dev-hooks build) makes the device verification report a failure;
 * PRT_TEST_FAIL_LIGHT_STAGE=k makes the k-th allocation (from 0) of a light update's spare arrays report PRT_E_OOM.
 */
int prt_scene_set_dynamic_lights(PrtScene* scene, int on); /* any time; survives prt_scene_upload / prt_scene_update_vertices */
int prt_scene_get_dynamic_lights(const PrtScene* scene, int* on);

typedef struct PrtLightUpdateInfo {
    uint64_t updates;        /* light updates since the last upload (calls in which an emitter vertex differed) */
    double gather_ms;        /* hipEvent: the first phase that gathers the emitters' new vertices, with its read-back */
    double host_tree_ms;     /* wall: Triangle precompute of the emitter triangles + the sort replay + the plan, on the host */
    double tables_ms;        /* hipEvent: thresholds + buckets + verification on the device, with the read-back of the words */
    uint32_t n_tables, table_words; /* of the resident light state */
    uint32_t tables_dropped; /* 1 if the last update's verification failed and the scene now descends the full tree */
    uint32_t relaid;         /* 1 if the last update changed the layout */
} PrtLightUpdateInfo;
/* Synchronous, like prt_scene_refit_info (the times are of the last light update). */
int prt_scene_light_update_info(const PrtScene* scene, PrtLightUpdateInfo* out);

/* Test hook, beside prt_scene_light_order: the resident O(1) table words (DLightTable headers, thresholds, buckets), read
 * back from the device (synchronous).  *n = word count (0: no tables); copies min(*n, cap) words.  PRT_E_NO_DEVICE unless
 * the scene is uploaded. */
int prt_scene_light_table_words(PrtScene* scene, uint32_t* words, uint64_t cap, uint64_t* n);

/* Number of light triangles and their order in the reference's area-CDF descent (BVH.cpp:86-100). */
int prt_scene_bvh_info(const PrtScene* scene, PrtBvhInfo* out);

int prt_scene_light_count(const PrtScene* scene, uint64_t* n);
int prt_scene_light_order(const PrtScene* scene, int32_t* prims, uint64_t cap);

/* K1: closest hit for a batch of host rays; with count_work != 0 the counting instantiation runs. */
int prt_trace_closest(PrtScene* scene, const PrtRay* rays, size_t n, PrtHit* hits, int count_work);
/* K1 on device-resident buffers (d_rays/d_hits are device pointers); stream may be NULL. */
int prt_trace_closest_device(PrtScene* scene, const void* d_rays, size_t n, void* d_hits,
                             int count_work, void* hip_stream);
/* Same with a PRT_PRECISION_* choice (rays and hits stay fp64 records at the boundary). */
int prt_trace_closest_device_prec(PrtScene* scene, const void* d_rays, size_t n, void* d_hits,
                                  int count_work, int precision, void* hip_stream);

/* K4 + K1: the same batch traced in a locality order.  A pre-pass sorts (cell of the origin in the scene's box, octant of
 * the direction) keys on the device and K1 takes the rays in that order, so that the lanes of a wave walk the same part
 * of the tree — for scenes whose BVH and triangles exceed the caches (several million triangles) and batches of
 * incoherent rays, where every node visit is otherwise a line of its own from HBM.  hits[i] still answers rays[i], bit
 * for bit what prt_trace_closest_device_prec returns; the time reported by prt_get_counters covers keys + sort + trace.
 * Needs 16 bytes of scratch per ray (kept by the scene between calls); n < 2^32.  On cache-resident scenes the sort costs
 * more than it returns. */
int prt_trace_closest_sorted_device(PrtScene* scene, const void* d_rays, size_t n, void* d_hits,
                                    int count_work, int precision, void* hip_stream);

/* Any-hit occlusion queries: world.Hit(ray, Interval(tmin, tmax), record) != miss, for a batch.  occluded[i] = 1 iff some
 * triangle is accepted in [rays[i].tmin, rays[i].tmax], else 0 — one byte per ray, nothing else is written (bytes beyond n
 * stay as they are).  The any-hit form of K1: the traversal ends at the first accepted triangle and fetches neither the
 * triangle's normal nor its shading record, so a visibility / shadow / line-of-sight test does not pay for a
 * nearest-hit search and a PrtHit per ray.
 * Contract: occluded[i] == (hits[i].prim >= 0) of prt_trace_closest_device_prec for the same ray record and the same
 * precision, on EVERY ray — whichever builder made the tree, and whether or not the batch was sorted.  (A triangle is
 * accepted by the same test against the same interval in both kernels; exact ties, which may change WHICH triangle the
 * closest-hit call reports, cannot change a boolean.)
 * Arguments, checks and error codes are those of the closest-hit calls: PRT_E_NO_DEVICE on a scene that is not uploaded,
 * PRT_E_INVALID for a null buffer with n > 0, an unknown precision, or n >= 2^32 in the sorted call; n == 0 is PRT_OK.
 * Afterwards prt_get_counters reports rays_shadow == n, rays_closest == 0, samples == 0 and kernel_ms (keys + sort + trace
 * for the sorted call); with count_work != 0 also node_fetches / tri_tests / tri_full. */
int prt_trace_occluded(PrtScene* scene, const PrtRay* rays, size_t n, uint8_t* occluded, int count_work);
/* On device-resident buffers (d_rays: n PrtRay, d_occluded: n bytes); stream may be NULL. */
int prt_trace_occluded_device(PrtScene* scene, const void* d_rays, size_t n, void* d_occluded,
                              int count_work, int precision, void* hip_stream);
/* K4 first, as prt_trace_closest_sorted_device: same bytes, the batch traced in a locality order. */
int prt_trace_occluded_sorted_device(PrtScene* scene, const void* d_rays, size_t n, void* d_occluded,
                                     int count_work, int precision, void* hip_stream);

/* Surface queries: the whole HitRecord of world.Hit(ray, Interval(tmin, tmax), record) for a batch, plus the response of
 * the hit's material that prt_render_features defines (albedo, emission).  The surface form of K1: same traversal, same
 * accept test, and at the point where the closest-hit call writes its PrtHit the lane also reads the triangle's shading
 * record and material and writes 192 bytes.  192 bytes, the first 32 ARE the ray's PrtHit. */
typedef struct PrtSurface {
    double t, alpha, beta;  /* as PrtHit */
    int32_t prim, front;    /* as PrtHit */
    double position[3];     /* ray(t) = o + t d  (Ray::operator(), d not normalised) */
    double normal[3];       /* unit geometric normal on the ray's side (HitRecord::SetFaceNormal): what K3 shades with */
    double tangent[3];      /* Triangle.cpp:31-46, as stored (not flipped) */
    double uv[2];           /* (1-alpha-beta) uv0 + alpha uv1 + beta uv2 */
    double albedo[3];       /* prt_render_features' rule, unaveraged: Lambertian/Debug Kd (texture if any); Phong Kd + Ks (the
                               texture twice); Mirror, CookTorrance, DiffuseLight, Empty (1,1,1) */
    double emission[3];     /* Material::GetEmission(): DiffuseLight radiance, Debug albedo, else 0; not face-dependent (as K3) */
    int32_t material;       /* index into PrtSceneDesc.materials */
    int32_t material_type;  /* PRT_MAT_* */
    int32_t reserved[4];    /* written as 0 */
} PrtSurface;
/* On a miss: t = +inf, alpha = beta = 0, prim = -1, front = 0 (the miss PrtHit), every other double 0,
 * material = material_type = -1, reserved 0.
 * Contract:
 *  1. For every ray, bytes 0-31 of out[i] equal the PrtHit that prt_trace_closest_device_prec / _sorted_device writes for
 *     the same ray record and precision, bit for bit (one traversal, one accept test).
 *  2. The rest is a pure function of that head, the ray and the resident scene tables.  With PRT_PRECISION_F32 it is
 *     computed from the float tables in float and widened at the boundary (tolerance tier 2).
 *  3. The records reflect the resident geometry: after prt_scene_refit* they follow the refitted records and tangents, and
 *     the call orders itself after a refit like every other trace call.
 *  4. Exactly n records are written; bytes beyond them stay as they are.  n == 0 is PRT_OK.
 *  5. Arguments, checks and error codes are those of the occlusion calls: PRT_E_NO_DEVICE on a scene that is not uploaded
 *     (the message names the function), PRT_E_INVALID for a null buffer with n > 0, an unknown precision, n >= 2^32 in the
 *     sorted call — and for a d_out that is not 32-byte aligned (the kernel stores 32 bytes at a time).
 *  6. Afterwards prt_get_counters reports rays_closest == n, rays_shadow == 0, samples == 0 and kernel_ms (keys + sort +
 *     trace for the sorted call); with count_work != 0 node_fetches / tri_tests / tri_full are those of the closest-hit
 *     call on the same batch. */
int prt_trace_surface(PrtScene* scene, const PrtRay* rays, size_t n, PrtSurface* out, int count_work); /* host buffers, fp64 */
/* On device-resident buffers (d_rays: n PrtRay, d_out: n PrtSurface, 32-byte aligned); stream may be NULL. */
int prt_trace_surface_device(PrtScene* scene, const void* d_rays, size_t n, void* d_out,
                             int count_work, int precision, void* hip_stream);
/* K4 first, as prt_trace_closest_sorted_device: same bytes, the batch traced in a locality order. */
int prt_trace_surface_sorted_device(PrtScene* scene, const void* d_rays, size_t n, void* d_out,
                                    int count_work, int precision, void* hip_stream);

/*
 * Closest-point queries: for each of n points, the nearest point of the mesh and its distance - the point form of
 * prt_trace_closest, against the same resident 4-wide BVH (the reference has no such query).  K6 (closest_point.hip): one
 * lane per query, a best-first descent with fp32 lower bounds of the point-box distance, fp64 point-triangle tests.
 *
 * The switch.  A ray needs a triangle's plane and edge functions (what the scene keeps); a point query needs its corners.
 * prt_scene_set_distance_queries(scene, 1) makes the scene keep them on the device: 96 bytes per triangle in BVH leaf
 * order, nothing while the switch is off (the default).  Any time; survives prt_scene_upload / prt_scene_update_vertices.
 * While it is on, every path that moves the resident geometry keeps the table in step: prt_scene_upload and
 * prt_scene_update_vertices make it from the host triangles, prt_scene_refit* and prt_scene_rebuild* from the caller's
 * positions through the resident (the rebuild's NEW) leaf order, on the call's stream in its writing phase; nothing else
 * those calls write changes.  Switching on for an uploaded scene builds the table at once from the host triangles
 * (synchronous; PRT_E_OOM / PRT_E_HIP leave the switch off) - and is refused with PRT_E_INVALID while the host geometry is
 * stale (PrtRefitInfo.host_stale: prt_scene_refit_device / prt_scene_rebuild_device moved the geometry past the host
 * copy): switch on before moving geometry, or call prt_scene_refit or prt_scene_update_vertices first.  Switching off
 * frees the table (after the queries in flight).
 */
int prt_scene_set_distance_queries(PrtScene* scene, int on);
int prt_scene_get_distance_queries(const PrtScene* scene, int* on);

typedef struct PrtPointQuery {
    double p[3];     /* the query point */
    double max_dist; /* search radius: +inf = unbounded, 0 is legal */
} PrtPointQuery; /* 32 bytes */

typedef struct PrtClosestPoint { /* 64 bytes */
    double dist;        /* |p - point|; +inf on a miss */
    double point[3];    /* the nearest point of the mesh */
    double alpha, beta; /* point = (1-alpha-beta) v0 + alpha v1 + beta v2 of triangle prim; alpha, beta >= 0, alpha+beta <= 1 */
    int32_t prim;       /* PrtSceneDesc order; -1 on a miss */
    int32_t feature;    /* 0 face, 1/2/3 edge v0v1 / v1v2 / v2v0, 4/5/6 vertex v0 / v1 / v2; -1 on a miss */
    int32_t side;       /* sign of dot(cross(v1-v0, v2-v0), p - point): +1, -1, 0; 0 on a miss */
    int32_t reserved;   /* written as 0 */
} PrtClosestPoint;
/* Contract:
 *  1. Candidates.  A triangle is a candidate iff its computed squared distance d2 satisfies d2 <= max_dist * max_dist,
 *     evaluated in fp64.  With no candidate the miss record is written: dist = +inf, prim = feature = -1, side = 0, every
 *     other field 0.
 *  2. d2, alpha, beta and feature come from the region-classifying point-triangle algorithm of Ericson, Real-Time Collision
 *     Detection 5.1.5, run in fp64 (no fused multiply-adds) on the resident corners; point = v0 + alpha (v1 - v0) +
 *     beta (v2 - v0), d2 = |p - point|^2, dist = sqrt(d2): a pure function of the query and the three corners.  At a vertex
 *     (alpha, beta) is exactly (0,0), (1,0) or (0,1); on edge v0v1 beta == 0, on v2v0 alpha == 0, on v1v2 alpha == 1 - beta.
 *     (A query that is bitwise some triangle's v0 therefore has d2 == 0 and is found with max_dist = 0; at a v1 or v2 the
 *     expression v0 + 1 (v1 - v0) can round to a neighbour of the corner, and d2 to a rounding above 0.)
 *  3. Ties.  The winner is the candidate with the smallest (d2, prim) in lexicographic order: the record does not depend on
 *     the tree, the builder, the leaf order or the batch order, bit for bit.  (Stricter than the ray calls' "later-tested
 *     wins": the traversal skips a subtree only when its lower bound is STRICTLY greater than the best d2 so far.)
 *  4. Culling is conservative: the fp32 lower bound of a box never exceeds the computed d2 of a triangle below it (the
 *     derivation is at box_bound, closest_point.hip).  The point is taken relative to the grid origin, so a unit scene at
 *     coordinate 1e6 is culled as well as one at the origin.
 *  5. fp64 only: there is no precision argument, no fp32 form and no sorted (K4) form.
 *  6. Exactly n records are written; bytes beyond them stay as they are.  n == 0 is PRT_OK.  d_out must be 32-byte aligned
 *     (the kernel stores 32 bytes at a time), else PRT_E_INVALID.
 *  7. Errors: PRT_E_NO_DEVICE on a scene that is not uploaded (the message names the function); PRT_E_INVALID when the
 *     switch is off (the message names the function and prt_scene_set_distance_queries), for a null buffer with n > 0, or
 *     n >= 2^32.  The host-buffer call also returns PRT_E_INVALID for a query with a non-finite p, or a max_dist that is NaN
 *     or negative (it checks the batch before anything else).  The device call does not read the queries on the host: its
 *     record for such a query is unspecified, but the call terminates.
 *  8. The call goes through the scene's two call slots like the trace calls: it orders itself after a refit or rebuild and
 *     is asynchronous on hip_stream.  Afterwards prt_get_counters reports kernel_ms, rays_closest == 0, rays_shadow == 0 and
 *     samples == 0; with count_work != 0 also node_fetches (node records read) and tri_tests (point-triangle tests), and in
 *     inner_rounds / leaf_rounds the stack entries (of inner nodes / of leaves) that were dropped at the pop by the bound
 *     they carry, without a fetch. */
int prt_closest_point(PrtScene* scene, const PrtPointQuery* q, size_t n, PrtClosestPoint* out, int count_work); /* host buffers, synchronous */
/* On device-resident buffers (d_q: n PrtPointQuery, d_out: n PrtClosestPoint, 32-byte aligned); stream may be NULL. */
int prt_closest_point_device(PrtScene* scene, const void* d_q, size_t n, void* d_out, int count_work, void* hip_stream);

/*
 * Signed distance queries: prt_closest_point with a sign that is right at edges and vertices too.  PrtClosestPoint.side is
 * the side of the winning triangle's plane, which is the inside/outside answer only where the nearest feature is a face: at
 * an edge or a vertex it depends on which incident triangle wins the (d2, prim) tie, and across an acute dihedral angle some
 * of them face away from the query.  The exact answer for closed meshes is the angle-weighted pseudonormal (Baerentzen and
 * Aanaes, "Signed distance computation using the angle weighted pseudonormal", IEEE TVCG 2005): the face normal at a face,
 * the sum of the unit normals of its faces at an edge, the sum of (interior angle x unit face normal) over the incident
 * faces at a vertex.
 *
 * Topology.  The triangles of the WHOLE scene are welded (objects are routinely split into meshes by material): two corners
 * are one vertex iff their three coordinates are bitwise equal after -0.0 -> +0.0; vertex ids ascend in order of first
 * appearance in (prim, corner) order.  An edge is an unordered pair of distinct vertex ids, numbered in first-appearance
 * order over (prim, edge v0v1, v1v2, v2v0); a triangle edge whose ends welded to one vertex has no id and its triangle counts
 * as degenerate.  prt_scene_topology_info reports what the weld found, computed on demand from the host triangles: it works
 * on any created scene, without a device and without the switch, and returns PRT_E_INVALID while PrtRefitInfo.host_stale is
 * set.
 */
typedef struct PrtTopologyInfo {
    uint64_t n_vertices, n_edges;
    uint64_t boundary_edges;     /* one face */
    uint64_t nonmanifold_edges;  /* three or more faces */
    uint64_t inconsistent_edges; /* two faces that traverse the edge in the same direction */
    uint64_t degenerate_tris;    /* two corners welded, or cross(v1-v0, v2-v0) is exactly zero */
    uint64_t max_valence;        /* faces at the busiest vertex */
    uint64_t table_bytes;        /* device bytes the signed-query tables hold (0 while off / not uploaded) */
    uint32_t closed;             /* 1 iff boundary == nonmanifold == inconsistent == 0 */
    uint32_t reserved;
} PrtTopologyInfo;
int prt_scene_topology_info(const PrtScene* scene, PrtTopologyInfo* out);

/*
 * The switch.  prt_scene_set_signed_queries(scene, 1) makes an uploaded scene keep, beside the corner table of the distance
 * queries, six uint32 ids per triangle (vertex ids, edge ids, in description order), the two adjacency lists (vertex ->
 * (prim, corner), edge -> prim, each ascending), per triangle its unit normal and corner angles, and one fp64 pseudonormal
 * per vertex and per edge: PrtTopologyInfo.table_bytes, about 152 bytes per triangle of a closed mesh.  Any time; survives
 * prt_scene_upload / prt_scene_update_vertices.  Switching on also switches distance queries on (a failure leaves both
 * switches as they were), and prt_scene_set_distance_queries(scene, 0) while signed queries are on is PRT_E_INVALID.
 * Switching on for an uploaded scene is synchronous (a host pass: weld + adjacency), and refused while the host geometry is
 * stale, by prt_scene_set_distance_queries' rule.  Switching off frees the tables (distance queries stay on).
 * The ids are made by prt_scene_upload, by prt_scene_update_vertices and by switch-on for an uploaded scene.
 * prt_scene_refit* and prt_scene_rebuild* KEEP them (they are in description order: a new leaf order needs no permutation)
 * and recompute the pseudonormals from the new positions on the call's stream, in their writing phase.  A caller who moves
 * two welded corners apart with one of those calls therefore gets the sign of the OLD connectivity;
 * prt_scene_update_vertices welds again.
 *
 * Pseudonormals (pseudonormals.hip; fp64, no fused multiply-adds).  Per triangle n = cross(v1-v0, v2-v0), nu = n / sqrt(dot(n,n)),
 * the interior angle at corner k = atan2(|cross(e1,e2)|, dot(e1,e2)) with e1 = v[k+1]-v[k], e2 = v[k+2]-v[k].  A triangle
 * whose dot(n,n) is 0 or not finite, or one of whose edges has no id, contributes nothing.  vn[v] = sum of angle * nu over
 * the vertex's faces, en[e] = sum of nu over the edge's faces, each in ascending prim order from 0.0: the same bits on every
 * run and for every builder or leaf order.  Neither is normalised: only a sign is taken from them.
 *
 * prt_scene_pseudonormals (test hook): out[t][0..2] = en of edges v0v1, v1v2, v2v0 and out[t][3..5] = vn of v0, v1, v2 of
 * triangle t in description order (features 1..6), zeros for a slot without an id; *n = the scene's triangles, of which
 * min(*n, cap_tris) are written.  Synchronous.  PRT_E_INVALID while the switch is off, PRT_E_NO_DEVICE unless uploaded.
 */
int prt_scene_set_signed_queries(PrtScene* scene, int on);
int prt_scene_get_signed_queries(const PrtScene* scene, int* on);
int prt_scene_pseudonormals(PrtScene* scene, double* out /* [n_tris][6][3] */, uint64_t cap_tris, uint64_t* n);

typedef struct PrtSignedDistance { /* 64 bytes, the layout of PrtClosestPoint */
    double sdist;       /* sign < 0 ? -dist : dist; +inf on a miss */
    double point[3];
    double alpha, beta;
    int32_t prim;
    int32_t feature;
    int32_t side;       /* as PrtClosestPoint.side */
    int32_t sign;       /* of dot(N, p - point), N the pseudonormal of the nearest feature: +1, -1, 0 */
} PrtSignedDistance;
/* Contract:
 *  1. Every field but sdist and sign is, bit for bit, what prt_closest_point* writes for the same query, and |sdist| equals
 *     that call's dist bit for bit.
 *  2. sign.  s = dot(N, p - point) evaluated as x*x + y*y + z*z in fp64 without contraction.  Feature 0: N = cross(v1-v0,
 *     v2-v0) of the winner, so s is side's expression and sign == side.  Features 1-3: N = en[eid[feature-1]]; features
 *     4-6: N = vn[vid[feature-4]], of the winning triangle.  sign = +1 for s > 0, -1 for s < 0, 0 otherwise: s == 0, s NaN,
 *     a slot without an id, a miss.  sdist = sign < 0 ? -dist : dist; +inf on a miss.
 *  3. Meaning.  On a scene with PrtTopologyInfo.closed == 1 whose faces are counter-clockwise seen from outside, sign == -1
 *     means inside.  On any other scene the formula still defines the value; nothing is promised about it.
 *  4. The record does not depend on the tree, the builder, the leaf order or the batch order, bit for bit (the (d2, prim)
 *     rule, and sums in prim order).
 *  5. Items 1, 5, 6, 7 and 8 of the closest-point contract apply, with this difference: PRT_E_INVALID while the signed
 *     switch is off (the message names the function and prt_scene_set_signed_queries) is reported before PRT_E_NO_DEVICE. */
int prt_signed_distance(PrtScene* scene, const PrtPointQuery* q, size_t n, PrtSignedDistance* out, int count_work); /* host buffers, synchronous */
int prt_signed_distance_device(PrtScene* scene, const void* d_q, size_t n, void* d_out, int count_work, void* hip_stream);

/*
 * Winding-number queries: inside / outside that survives open meshes.  The sign of prt_signed_distance means something only
 * where PrtTopologyInfo.closed == 1, and crossing parity from prt_trace_multi flips at every hole.  The generalized winding
 * number (Jacobson, Kavan and Sorkine-Hornung, "Robust inside-outside segmentation using generalized winding numbers",
 * SIGGRAPH 2013) is the signed solid angle the mesh subtends at the query point, over 4 pi: exactly 0 or 1 for a closed
 * mesh, and it degrades smoothly across holes, seams, duplicated faces and self-intersections; w > 0.5 is a usable "inside".
 * The exact sum costs O(triangles) per query; the fast form (Barill, Dickson, Schmidt, Levin and Jacobson, "Fast winding
 * numbers for soups and clouds", SIGGRAPH 2018) replaces a far cluster of the BVH by its dipole and costs O(log n).  Only
 * the dipole (first-order) term is used.
 *
 * The switch.  prt_scene_set_winding_queries(scene, 1) makes an uploaded scene keep, beside the corner table of the distance
 * queries, one 64-byte fp64 record {N[3], c[3], r, A} for every child slot of every node of the resident tree: 256 bytes per
 * node, indexed [node][slot], all zero for an unused slot.  The rules are those of prt_scene_set_signed_queries: any time;
 * survives prt_scene_upload / prt_scene_update_vertices; switching on also switches distance queries on (a failure leaves
 * both as they were), and prt_scene_set_distance_queries(scene, 0) while winding queries are on is PRT_E_INVALID; refused
 * while the host geometry is stale; synchronous for an uploaded scene; switching off frees the table (distance queries stay
 * on).  The table is made again wherever the tree or the corners change: by prt_scene_upload and
 * prt_scene_update_vertices, by prt_scene_refit* on the call's stream behind the box refit (no new host synchronisation),
 * and by prt_scene_rebuild* for the new node array (allocated before anything resident is written: all or nothing).
 *
 * Records (winding_number.hip; fp64, no fused multiply-adds; every sum starts from 0.0 and is taken in the stated order).
 *   Leaf slot, its triangles in leaf order, resident corners v0, v1, v2:  av = 0.5 cross(v1 - v0, v2 - v0), a = sqrt(dot(av,
 *   av)), g = ((v0 + v1) + v2) / 3; a triangle whose a is 0 or not finite contributes nothing;  A = sum a, N = sum av,
 *   G = sum a g;  c = A > 0 ? G / A : v0 of the first triangle;  r = the largest sqrt(|v - c|^2) over all corners of the slot.
 *   Inner slot that refers to node m, m's used slots s in slot order:  A = sum A_s, N = sum N_s, G = sum A_s c_s;
 *   c = A > 0 ? G / A : c of m's first used slot;  r = max over s of (sqrt(|c_s - c|^2) + r_s).
 * One tree and one corner table always give the same bits (a bottom-up pass without floating-point atomics).
 *
 * prt_scene_winding_moments (test hook): out[node][slot][0..7] = N, c, r, A as the device holds them; *n = the nodes of the
 * resident tree, of which min(*n, cap_nodes) are written.  Synchronous.  PRT_E_INVALID while the switch is off,
 * PRT_E_NO_DEVICE unless uploaded.
 */
int prt_scene_set_winding_queries(PrtScene* scene, int on);
int prt_scene_get_winding_queries(const PrtScene* scene, int* on);
int prt_scene_winding_moments(PrtScene* scene, double* out /* [n_nodes][4][8] */, uint64_t cap_nodes, uint64_t* n);

#define PRT_WINDING_BETA_DEFAULT 2.0
/* Contract:
 *  1. out[i] = S / (4 pi), S from this walk, started at the root.  For each used slot of the node, with its record:
 *     d = c - p, dd = dot(d, d), br = beta * r;  if dd > br * br (far): S += dot(N, d) / (dd * sqrt(dd));  else, for a leaf:
 *     S += Omega of each of its triangles;  else: the child is walked.  Omega = 2 atan2(num, den) with a = v0 - p, b = v1 - p,
 *     c = v2 - p, num = dot(a, cross(b, c)), den = |a||b||c| + dot(a,b)|c| + dot(b,c)|a| + dot(c,a)|b| (Van Oosterom and
 *     Strackee 1983).  All of it in fp64 without contraction; dot(x, y) is x0 y0 + x1 y1 + x2 y2.  The ORDER in which the
 *     terms of one query are added is fixed by the tree (a node's far terms in slot order, then its near slots in slot
 *     order, depth first) and not part of the contract beyond that: the value is within a few ulps of |terms| of any order.
 *     (A leaf slot whose ref equals that of the slot before it is skipped: the root of a one-triangle tree lists its leaf twice.)
 *  2. Sign: +1 inside a closed mesh whose faces are counter-clockwise seen from outside.
 *  3. beta = +inf takes no far term: the value is the exact sum over every triangle.  Larger beta: smaller error, more work.
 *  4. The value is a pure function of the query, beta, the resident tree and the tables: batch order, batch splitting,
 *     count_work and the refill schedule change no bit.
 *  5. The value DOES depend on the tree, unlike the other point queries: the two builders, a refit and a rebuild give
 *     values that differ by the approximation error (beta = +inf: by rounding only).
 *  6. For a query on the surface the value is finite; nothing else is promised there.  max_dist is not read.
 *  7. fp64 only: no fp32 form and no sorted form.
 *  8. Errors, in this order: PRT_E_INVALID while the switch is off (the message names the function and
 *     prt_scene_set_winding_queries; before PRT_E_NO_DEVICE); PRT_E_INVALID for beta NaN or <= 1; then items 6 to 8 of the
 *     closest-point contract, with an output of n doubles that must be 8-byte aligned.
 *  9. With count_work != 0 prt_get_counters reports node_fetches = nodes walked, tri_tests = Omega evaluations,
 *     inner_rounds = far terms taken at inner slots, leaf_rounds = far terms taken at leaf slots. */
int prt_winding_number(PrtScene* scene, const PrtPointQuery* q, size_t n, double beta, double* out, int count_work); /* host buffers, synchronous */
/* d_q: n PrtPointQuery (one device buffer serves all three point queries), d_out: n doubles; stream may be NULL. */
int prt_winding_number_device(PrtScene* scene, const void* d_q, size_t n, double beta, void* d_out, int count_work, void* hip_stream);

/*
 * Multi-hit queries: for each of n rays, the first k surfaces along it, in order - thickness and X-ray measurements,
 * crossing parity, entry/exit pairs of closed shells, layered transparency done by the caller, depth layers.  K7
 * (multi_hit.hip): K1's persistent waves and box stepping with a leaf step that keeps a sorted per-lane list.  One
 * traversal instead of k closest-hit calls with tmin moved past the previous t - and, unlike such a peel, exact at ties:
 * two triangles hit at a bit-identical t (shared edges, coplanar neighbours, duplicated geometry) are both reported.
 */
#define PRT_MULTI_HIT_MAX 8
typedef struct PrtHitCursor {
    double t;         /* the t of the record to continue after; -inf: from the start of the interval */
    int32_t prim;     /* ... and its prim; -1 with t = -inf */
    int32_t reserved; /* must be 0 */
} PrtHitCursor; /* 16 bytes */
/* hits holds n * k PrtHit records: ray i owns hits[i*k .. i*k + k-1].
 * Contract:
 *  1. Candidates.  A triangle is a candidate for ray i iff the closest-hit call's triangle test accepts it over the
 *     INCLUSIVE interval [tmin, tmax] (tri_test, prt_device.h: |n.d| >= 1e-8, tmin <= t <= tmax, alpha, beta >= 0,
 *     alpha + beta <= 1, no NaN) and, if `after` is given, the pair (t, prim) is lexicographically greater than
 *     (after[i].t, after[i].prim).  after == NULL means no cursor for any ray; {t = -inf, prim = -1} is the neutral cursor
 *     for one ray.  prim is the PrtSceneDesc index, as everywhere at this boundary.
 *  2. Result.  The min(k, #candidates) smallest candidates by (t, prim), in ascending order, each written as the PrtHit the
 *     closest-hit call writes for that triangle (t, alpha, beta, prim, front); every remaining slot holds the miss record
 *     (t = +inf, alpha = beta = 0, prim = -1, front = 0).  No primitive appears twice.
 *  3. Independence.  The bytes do not depend on the builder, the tree, the leaf order, the batch order, sorted or plain, or
 *     count_work.  (Stricter than the closest-hit call's "later-tested wins": a subtree is skipped only when its fp32 entry
 *     bound lies beyond the k-th t rounded up, so a tying triangle with a smaller prim is never culled; the argument is at
 *     the kernel.)
 *  4. Paging.  Feed the last non-miss record of a page back as that ray's cursor to get the next page: for k1 * m <=
 *     PRT_MULTI_HIT_MAX, m pages of size k1 are, bit for bit, the first k1 * m records of one call with k = k1 * m - also
 *     when a tie straddles a page boundary.  (A ray whose page ends in a miss record has no further hits.)
 *  5. Relation to the closest-hit call.  Slot 0 without a cursor is a closest hit by the same test, but is not promised
 *     bit-equal to prt_trace_closest*: ties resolve differently (smallest prim here, later-tested there), and this kernel's
 *     triangle arithmetic is compiled with floating-point contraction off, K1's is not.  Both are within the tier-1 (fp64)
 *     or tier-2 (fp32) tolerance of the exact value.
 *  6. Precision.  Both precisions at the device calls; rays, cursors and hits stay fp64 records at the boundary.  In fp32 the
 *     cursor's t is rounded to float on load; a hit's t is a widened float, so paging is exact within fp32 as well.
 *  7. Errors.  PRT_E_NO_DEVICE on a scene that is not uploaded (the message names the function); PRT_E_INVALID for k < 1 or
 *     k > PRT_MULTI_HIT_MAX, a null rays or hits with n > 0, an unknown precision, n >= 2^32 in the sorted call, or a d_hits
 *     that is not 32-byte aligned (the kernel stores 32 bytes at a time).  n == 0 is PRT_OK.  The host call also refuses a
 *     cursor whose t is NaN or whose reserved != 0.  The device call does not read cursors on the host: a NaN t there has no
 *     candidate after it (miss records), reserved is not read, and the call terminates on any input.
 *  8. Written range.  Exactly n * k records are written; bytes beyond them stay as they are.
 *  9. Ordering and counters.  The call goes through the scene's two call slots and orders itself after a refit or rebuild,
 *     like the trace calls.  Afterwards prt_get_counters reports rays_closest == n, rays_shadow == 0, samples == 0 and
 *     kernel_ms (keys + sort + trace for the sorted call); with count_work != 0 also node_fetches / tri_tests / tri_full
 *     (the at most k re-evaluations of the winners at the write-out are not counted). */
int prt_trace_multi(PrtScene* scene, const PrtRay* rays, const PrtHitCursor* after, size_t n, int32_t k,
                    PrtHit* hits, int count_work); /* host buffers, fp64, synchronous */
/* On device-resident buffers (d_rays: n PrtRay, d_after: n PrtHitCursor or NULL, d_hits: n * k PrtHit, 32-byte aligned);
 * stream may be NULL. */
int prt_trace_multi_device(PrtScene* scene, const void* d_rays, const void* d_after, size_t n, int32_t k,
                           void* d_hits, int count_work, int precision, void* hip_stream);
/* K4 first, as prt_trace_closest_sorted_device: same bytes, the batch traced in a locality order. */
int prt_trace_multi_sorted_device(PrtScene* scene, const void* d_rays, const void* d_after, size_t n, int32_t k,
                                  void* d_hits, int count_work, int precision, void* hip_stream);

/* NEE point selection for (pixel, sample) keys 0..n-1 of `seed` from given origins (test hook). */
int prt_sample_lights(PrtScene* scene, const double* origins, size_t n, uint64_t seed,
                      PrtLightSample* out);

/*
 * Test hooks for the material arithmetic K3 shades with (the device functions themselves, on caller-supplied
 * directions).  Item i draws from the stream keyed (seed, i, 0).  `material` / `texture` index the scene's tables.
 *   prt_material_eval     Material::Eval(wi, ctx{wo, uv}), wi / wo LOCAL (z = shading normal):
 *                         Lambertian Material.h:128-130, PhoneReflectance :227-248 (draws one number), CookTorrance :474-496
 *   prt_material_scatter  Material::Scatter(Ray(0, rd_i), record{normal, tangent, uv}) (Material.h:131-151,263-285,
 *                         344-363,497-516): scattered direction in WORLD space, attenuation = f cos / pdf, ok = its return value
 *   prt_texture_value     ImageTexture::Value(u, v) (Texture.cpp:22-49)
 * uv may be NULL (all zero).
 */
int prt_material_eval(PrtScene* scene, int32_t material, size_t n, const double* wi, const double* wo, const double* uv,
                      uint64_t seed, double* f);
int prt_material_scatter(PrtScene* scene, int32_t material, size_t n, const double* rd, const double* normal,
                         const double* tangent, const double* uv, uint64_t seed, double* wi_world, double* attenuation,
                         int32_t* ok);
int prt_texture_value(PrtScene* scene, int32_t texture, size_t n, const double* uv, double* rgb);

/*
 * K3+K5: render one frame.  rgb_f64 / rgb_f32 are W*H*3 row-major host buffers (either may be
 * NULL).  Pixels of tiles owned by other ranks are written as 0 so a sum over ranks is exact.
 */
int prt_render(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params,
               double* rgb_f64, float* rgb_f32);
/* Same, outputs are device pointers on the scene's device; asynchronous on hip_stream.  A scene keeps two sets of
 * per-call state (counters, partial sums, events): two calls — render or trace — may be in flight at once on different
 * streams; a third one first waits (on its stream) for the call that last used its set.  A PrtScene is not thread-safe:
 * issue its calls from one host thread. */
int prt_render_device(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params,
                      void* d_rgb_f64, void* d_rgb_f32, int count_work, void* hip_stream);

/*
 * Radiance queries: RayColor for caller-supplied rays.  K3 itself, the path tracer of prt_render, with the batch as its ray
 * source instead of a pinhole camera: one work item per (ray, sample chunk), the primary ray traced once per work item.
 * Contract:
 *  1. out[i][0..2] = the mean over samples s in [sample_begin, sample_begin + params->spp) of
 *     RayColor(Ray(rays[i].o, rays[i].d), max_depth, world, lights) (Source/Camera.cpp:119-204).  Sample s of ray i draws from
 *     the stream keyed (seed, key_i, s) with key_i = keys ? keys[i] : (uint32_t)i — a frame's keying with "pixel index"
 *     replaced by "key": a batch of a camera's rays with key = j*W+i is that camera's frame.  Every term is scaled by 1/spp
 *     as it is added, a work item sums its chunk in sample order and the chunks are added in ascending order: the rules of
 *     prt_render and its K5.
 *  2. Rays: d is not normalised (camera directions are not either).  tmin and tmax are NOT read: the primary ray is traced
 *     over Interval(0.0001, inf) as RayColor traces it.
 *  3. Parameters: spp, max_depth, russian_roulette, sample_lights, precision, background, seed and sample_chunks mean what
 *     they mean in prt_render.  tile_size, rank and nranks are ignored (a batch has no tiles; a caller splits a batch
 *     itself).  pixel_jitter and reserved must be 0: there is no pixel to jitter.
 *  4. Both precisions.  With PRT_PRECISION_F32 the fp64 ray records are rounded to float on load (tolerance tier 2); partial
 *     sums and outputs stay fp64.
 *  5. Either output may be NULL, not both.  Exactly n triples are written; bytes beyond them stay as they are.  n == 0 is
 *     PRT_OK.  max_depth < 0 gives zeros.
 *  6. Errors: PRT_E_NO_DEVICE on a scene that is not uploaded (the message names the function); PRT_E_INVALID for a null
 *     `rays` with n > 0, both outputs null, spp < 1, sample_begin < 0, sample_begin + spp > INT32_MAX, an unknown
 *     precision, a nonzero pixel_jitter or reserved; PRT_E_LIMIT when n x sample chunks reaches 2^32.  The host-buffer call
 *     also returns PRT_E_INVALID for a ray whose origin or direction is not finite or whose direction is zero.  The device
 *     call does not check the rays: the result for such a ray is unspecified.
 *  7. The call goes through the scene's two call slots like prt_render_device: it orders itself after a refit, and two
 *     calls may be in flight on two streams.  Afterwards prt_get_counters reports rays_closest, rays_shadow,
 *     samples == n * spp and K3's kernel_ms.  There is no count_work form and no trace signature.
 * keys may be NULL.  The ray order is the caller's: neighbouring rays that start and point alike traverse together.
 */
int prt_ray_color(PrtScene* scene, const PrtRay* rays, const uint32_t* keys, size_t n, const PrtRenderParams* params,
                  int32_t sample_begin, double* rgb_f64, float* rgb_f32); /* host buffers, synchronous */
/* On device-resident buffers (d_rays: n PrtRay, d_keys: n uint32 or NULL, outputs: n triples); asynchronous on hip_stream,
 * which may be NULL. */
int prt_ray_color_device(PrtScene* scene, const void* d_rays, const void* d_keys, size_t n, const PrtRenderParams* params,
                         int32_t sample_begin, void* d_rgb_f64, void* d_rgb_f32, void* hip_stream);

/*
 * Camera::Render over several GPUs of one process — the reference's only parallel split is the thread fan-out over row
 * bands inside Camera::Render (Source/Camera.cpp:46-71); here the frame is cut into 16x16 tiles dealt over the scenes:
 * scenes[r] is the SAME scene description uploaded to a different device each (prt_scene_upload).  Every device renders
 * its tiles into a zeroed full-size fp32 framebuffer, ONE RCCL reduce(sum, float) to scenes[0]'s device assembles the
 * frame (disjoint tiles: x + 0 + ... + 0 — an exact reduce; the single-GPU fp32 image bit for bit when sample_chunks is
 * explicit, else up to the fp64 rounding of a share's own chunking, ~1e-15) and one copy brings it to rgb_f32
 * (W*H*3 floats).  n == 1 is prt_render's fp32 output.  All scenes on ONE device (tile-share replicas) are summed on
 * that device without a collective; any other mix is refused.  If the RCCL communicator cannot be created, or the
 * reduce fails, the call fails (PRT_E_HIP): there is no host-side sum to fall back to; the scenes stay usable and the
 * caller's current HIP device is restored on every way out.  Communicators are cached per device list until prt_shutdown.
 * EXPERIMENTAL for n > 1 on different devices: that branch has so far only run with a communicator of one rank (no
 * multi-GPU box was available to rounds 1-4).  The result has fp32 precision (the element type of the reduce), where
 * prt_render's rgb_f64 is the fp64 frame.
 */
int prt_render_multi(PrtScene* const* scenes, int n, const PrtCamera* cam, const PrtRenderParams* params, float* rgb_f32);
/* Releases process-wide state: the RCCL communicators prt_render_multi cached (ncclCommDestroy).  Scenes are untouched.
 * Call before exit after multi-device renders; may be called repeatedly, and prt_render_multi re-creates what it needs. */
void prt_shutdown(void);

/*
 * Test hook: RayColor of single camera samples through K3 itself (the production instantiation of k_render when `trace`
 * is NULL, its counting instantiation otherwise) — what orc_render_samples is for the oracle.  Sample s of pixel
 * (pixel_xy[2k], pixel_xy[2k+1]) draws from the stream keyed (params->seed, j*W+i, s) like in a frame, whatever params->spp
 * says; radiance[k][s - sample_begin][3] is that sample's RayColor (not divided by spp).  params->precision must be
 * PRT_PRECISION_F64; rank / tile / chunk fields are ignored.
 * trace (optional) [n_pixels][sample_count][PRT_TRACE_WORDS]: the path's signature — word 0 = path vertices visited;
 * then per vertex v (at most PRT_TRACE_VERTS): word 1+2v = triangle hit (PrtSceneDesc order, -1 = miss), word 2+2v = flags:
 *   PRT_TRACE_NEE       the light sample passed n.wi > 0 and faces the shading point (Camera.cpp:153-154): a shadow ray was traced
 *   PRT_TRACE_VISIBLE   ... and it reached the light: direct light was added (Camera.cpp:155-172)
 *   PRT_TRACE_ROULETTE  RandomDouble() < russianRoulette (Camera.cpp:180)
 *   PRT_TRACE_SCATTER   Material::Scatter returned true (Camera.cpp:182)
 */
#define PRT_TRACE_WORDS 64
#define PRT_TRACE_VERTS 31
#define PRT_TRACE_NEE 1
#define PRT_TRACE_VISIBLE 2
#define PRT_TRACE_ROULETTE 4
#define PRT_TRACE_SCATTER 8
int prt_render_samples(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params, const int32_t* pixel_xy,
                       size_t n_pixels, int32_t sample_begin, int32_t sample_count, double* radiance, int32_t* trace);

int prt_get_counters(PrtScene* scene, PrtCounters* out);

/* K5 "next" row: NaN scrub + linear->sRGB + clamp -> 8-bit RGB (Camera.cpp:206-221,279-301). */
int prt_tonemap_srgb8(PrtScene* scene, const void* d_rgb_f32, int width, int height,
                      void* d_rgb_u8, void* hip_stream);

/*
 * Progressive, resumable rendering.  Camera::Render adds every sample's RayColor * (1/spp) into colorAttachment as it
 * goes (Source/Camera.cpp:46-83; pixelSamplesScale, :83).  An accumulator reorders that scale: it keeps the RAW fp64
 * sum of every sample rendered so far per pixel and channel, and divides by the sample count only when a frame is
 * resolved.  Sample s of pixel (i, j) draws from the stream keyed (seed, j*W+i, s) whatever the pass, so after n samples
 * the resolved frame is prt_render's frame at spp = n: the same samples, summed in another order (prt_render scales each
 * term by 1/n and sums per sample chunk; the accumulator sums raw terms per pass chunk, then per pass, then divides) —
 * about 1e-13 relative apart, not bit for bit.  A ladder of spp 10/50/100/500 frames costs one spp-500 render plus four
 * resolves instead of the sum of the rungs, a render can be previewed while it runs, stopped, and continued later.
 *
 * Camera and render parameters are frozen at create time; params->spp is ignored (the pass size is the argument of
 * prt_accum_render) and params->reserved must be 0.  sample_chunks applies to each pass; both precisions are supported
 * (PRT_PRECISION_F32 renders in fp32 and still accumulates in fp64); pixel_jitter, tile_size, rank and nranks behave as
 * in prt_render: pixels of other ranks' tiles are never touched and stay 0, so the sums of the ranks' accumulators add
 * up to the single-rank one.  Each pass goes through the scene's two per-call slots like prt_render_device:
 * prt_get_counters afterwards reports that pass (K3 time only), and two accumulators on two streams behave like two
 * prt_render_device calls.  Passes and resolves of ONE accumulator are ordered by the library (each waits on its stream
 * for the previous use of the sums), whatever streams they are issued on.  Each pass retraces the camera ray of every
 * work item once (the parked primary hit is not kept between passes).
 *
 * The sums belong to one geometry: prt_scene_update_vertices bumps a generation counter of the scene, and a pass on
 * sums of an older generation fails with PRT_E_INVALID until prt_accum_reset.  The fingerprint is a 64-bit hash of the
 * camera, every parameter that changes a sample's value or a pixel's owner (max_depth, russian_roulette, sample_lights,
 * precision, background, seed, tile size, rank, nranks, pixel_jitter) and the scene's triangle, mesh and material
 * COUNTS.  It does NOT detect a different scene that happens to have the same counts: importing a checkpoint into such
 * a scene silently mixes two scenes.
 *
 * LIFETIME: an accumulator holds its scene's pointer and device memory on the scene's device; destroy it before the
 * scene.  The scene must stay uploaded to the same device (PRT_E_INVALID otherwise).
 */
typedef struct PrtAccum PrtAccum;
/* Zeroed sums (W*H*3 doubles on the scene's device) and 0 samples.  PRT_E_NO_DEVICE if the scene is not uploaded. */
int prt_accum_create(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params, PrtAccum** out);
/* Waits for the accumulator's last pass or resolve, then frees it.  NULL is a no-op. */
void prt_accum_destroy(PrtAccum* acc);
/* Asynchronous on hip_stream: adds samples [n, n + n_samples) of every owned pixel, n = prt_accum_samples before the
 * call.  PRT_E_INVALID for n_samples < 1 or sums of an older scene generation; PRT_E_LIMIT if n + n_samples > INT32_MAX. */
int prt_accum_render(PrtAccum* acc, int32_t n_samples, void* hip_stream);
/* Samples per pixel accumulated so far (counted when a pass is issued). */
int prt_accum_samples(const PrtAccum* acc, uint64_t* n);
/* Synchronous: zero sums, 0 samples, and the scene's current geometry generation. */
int prt_accum_reset(PrtAccum* acc);
/* Asynchronous on hip_stream: the frame of the samples so far into W*H*3 device buffers (any may be NULL, not all):
 * rgb_f64 = sum / n, rgb_f32 = its float rounding, rgb_u8 = exactly the bytes prt_tonemap_srgb8 makes of rgb_f32 (the
 * same device code).  With 0 samples the frame is all zeros. */
int prt_accum_resolve(PrtAccum* acc, void* d_rgb_f64, void* d_rgb_f32, void* d_rgb_u8, void* hip_stream);
/* Synchronous: the resolved frame into W*H*3 host buffers (either may be NULL, not both). */
int prt_accum_read(PrtAccum* acc, double* rgb_f64, float* rgb_f32);
/* Synchronous checkpoint: the W*H*3 raw sums, the sample count and the fingerprint. */
int prt_accum_export(const PrtAccum* acc, double* sums, uint64_t* samples, uint64_t* fingerprint);
/* Resume from a checkpoint, in another process or on another PrtScene built from the same description: PRT_E_INVALID if
 * the fingerprint differs from this accumulator's, PRT_E_LIMIT above INT32_MAX samples.  The sums are taken to belong to
 * the scene's current geometry. */
int prt_accum_import(PrtAccum* acc, const double* sums, uint64_t samples, uint64_t fingerprint);

/*
 * Adaptive sampling.  An adaptive accumulator gives each pixel samples until its own noise estimate meets a tolerance.
 * Per pixel it keeps the raw fp64 RGB sum (as above), `moment` (fp64) and `count` (uint32, the pixel's samples n_p);
 * it also keeps one global count n.  Every pixel still running has count == n, so a round renders samples [n, n + k)
 * of every pixel it renders, and a pixel that stopped after n_p samples holds exactly prt_render(spp = n_p)'s value for
 * that pixel (up to summation order, as above).
 *
 * Samples come in batches of `batch` consecutive samples; a batch is one work item of the path tracer, so its sum is a
 * chunk partial.  With Y(rgb) = 0.2126 R + 0.7152 G + 0.0722 B and T_c = Y(batch c's RGB sum):
 *     moment_p  = sum_c T_c^2 / batch                              (batches added in sample order)
 *     C = n_p / batch,  S = Y(sum_p),  mean = S / n_p
 *     var       = max(0, moment_p - S^2 / n_p) / (C - 1)            (batch means: unbiased per-sample variance)
 *     se        = sqrt(var / n_p)
 *     converged = se <= max(rel_tol * |mean|, abs_tol)              (false for NaN: a NaN pixel runs to max_spp)
 * A pixel is ACTIVE iff it is owned by this rank, count == n, count < max_spp and not (count >= min_spp and
 * converged).  A stopped pixel's state never changes again, so the rule never revives it.  The outcome of a pixel
 * depends on its own samples only: the tile shares of nranks accumulators add up to the single-rank state.
 *
 * prt_accum_resolve / prt_accum_read divide each pixel by its own count (0 where the count is 0); prt_accum_samples is
 * n (the largest count); prt_accum_reset zeroes sums, moments, counts and n.  prt_accum_render, prt_accum_export and
 * prt_accum_import fail with PRT_E_INVALID on an adaptive accumulator (a plain checkpoint has no per-pixel counts).
 * The adaptive fingerprint hashes the plain one's fields plus min_spp, max_spp, the effective batch, rel_tol and
 * abs_tol under a layout tag of its own: plain and adaptive checkpoints never cross.
 */
typedef struct PrtAdaptiveParams {
    int32_t min_spp;  /* no pixel stops before this: a multiple of batch, >= 2 * batch */
    int32_t max_spp;  /* no pixel goes beyond this: a multiple of batch, >= min_spp */
    int32_t batch;    /* samples per batch (= per work item); 0 = PRT_ADAPTIVE_DEFAULT_BATCH */
    int32_t reserved; /* must be 0 */
    double rel_tol;   /* >= 0, finite */
    double abs_tol;   /* >= 0, finite */
} PrtAdaptiveParams;
#define PRT_ADAPTIVE_DEFAULT_BATCH 8 /* measured: tools/adaptive_timing.py, DESIGN.md §7 */

/* An adaptive accumulator: zeroed state and n = 0.  Params as for prt_accum_create; PRT_E_INVALID for a bad
 * PrtAdaptiveParams field. */
int prt_accum_create_adaptive(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params,
                              const PrtAdaptiveParams* adaptive, PrtAccum** out);
/* One round: (1) on the device, apply the rule above to every owned pixel and compact the active ones, in tile order,
 * into a list; (2) read the list's length back (the one synchronisation of a round); (3) if it is not 0, render samples
 * [n, n + min(n_samples, max_spp - n)) of the listed pixels in work items of `batch` samples; (4) add their sums,
 * moments and counts.  *n_active = pixels rendered (0: the frame is done, nothing was launched).  Steps (3) and (4)
 * are asynchronous on hip_stream.  n_samples must be a positive multiple of batch.  prt_get_counters afterwards reports
 * the round's last launch, with samples = listed pixels x that launch's samples. */
int prt_accum_render_adaptive(PrtAccum* acc, int32_t n_samples, uint64_t* n_active, void* hip_stream);
/* Synchronous: the W*H per-pixel sample counts (row-major, j*W+i).  Works on plain accumulators too (every owned
 * pixel has n samples there, the others 0). */
int prt_accum_pixel_samples(PrtAccum* acc, uint32_t* counts);
/* Synchronous checkpoint of an adaptive accumulator: W*H*3 sums, W*H moments, W*H counts, n and the fingerprint. */
int prt_accum_export_adaptive(const PrtAccum* acc, double* sums, double* moments, uint32_t* counts, uint64_t* samples,
                              uint64_t* fingerprint);
/* Resume from prt_accum_export_adaptive.  PRT_E_INVALID for another fingerprint, a count above `samples` or not a
 * multiple of batch, a nonzero count on a pixel this rank does not own, or a negative or non-finite moment;
 * PRT_E_LIMIT above INT32_MAX samples. */
int prt_accum_import_adaptive(PrtAccum* acc, const double* sums, const double* moments, const uint32_t* counts,
                              uint64_t samples, uint64_t fingerprint);

/*
 * First-hit feature buffers (AOVs) and an edge-aware a-trous denoiser.
 *
 * Features.  prt_render_features traces the camera rays of the first feature_spp samples of every pixel of the frame (all
 * of it, whatever rank / nranks / tile_size say) with the closest-hit traversal, always in fp64 (params->precision is
 * ignored).  The rays are K3's: with pixel_jitter = 0 every sample is the pixel centre, so the one ray is traced once; with
 * pixel_jitter = 1 sample s is offset by the SampleSquare() draws of the stream keyed (seed, j*W+i, s), as in a frame.  Per
 * pixel, written as fp32 (each output pointer may be NULL = skip):
 *   albedo [H][W][3]  at a hit: Lambertian, Debug: Kd (the texture if the material has one); Phong: Kd + Ks (the texture
 *                     twice when the material has one, as PhoneReflectance stores it); Mirror, CookTorrance, DiffuseLight,
 *                     Empty: (1,1,1).  At a miss: (1,1,1)
 *   normal [H][W][3]  at a hit: the unit geometric normal K3 shades with, facing the incoming ray (SetFaceNormal); miss: 0
 *   depth  [H][W]     at a hit: t * |d|, the world distance (camera directions are not normalised); miss: +inf
 *   prim   [H][W]     triangle index (PrtSceneDesc order) of sample 0's hit, -1 on a miss
 * With feature_spp > 1 albedo and normal are means over the samples (the normal mean is not renormalised) and depth is the
 * mean over the samples that hit (+inf if none did).  Sums are fp64; each output is the float rounding of its mean.
 *
 * Filter (Dammertz et al., HPG 2010), spatial only, fp32, deterministic.  Level i = 0 .. iterations-1 is a 5x5 gather with
 * step 2^i and weights h = [1,4,6,4,1]/16 per axis; each level's output colour is the next level's input, the features
 * stay fixed.  For a centre pixel p and a tap q inside the image:
 *     w = h(dx) h(dy) exp(-(|c_p-c_q|^2 / (sigma_color 2^-i)^2 + |n_p-n_q|^2 / sigma_normal^2
 *                          + Dz + |a_p-a_q|^2 / sigma_albedo^2))
 *     Dz = (z_p-z_q)^2 / (sigma_depth^2 z_p^2) if both hit (finite depth), 0 if both miss; w = 0 if exactly one misses
 *     out_p = sum w c_q / sum w
 * A tap with a non-finite colour gets weight 0; a non-finite centre outputs 0 at that level (as WriteColorAttachment maps
 * NaN to 0).  A sigma that is <= 0 or +inf switches its term off (for sigma_depth: the hit / miss rule as well); NaN is
 * refused.  demodulate = 1: the filter runs on c / max(a, 1e-3) per channel and multiplies the result back by the same
 * max(a, 1e-3).  iterations = 0 copies the input.  The restatement in numpy is tests/denoise_model.py.
 * Precision: the fp32 result follows the fp64 rule within about 1e-6 relative while the exponents stay small.  Where the
 * colour term's exponent is in the tens (demodulated colours of albedo near 1e-3 reach 1e3-1e4 beside colours near 1;
 * inputs spanning many decades), exp() multiplies each level's fp32 rounding by about that exponent, and the gap grows
 * with the levels: about 1e-4 relative after 10 levels on such pixels (dark pixels next to those taps), not a bug.
 */
typedef struct PrtDenoiseParams {
    int32_t iterations;   /* levels, 0..10; 0 copies the input */
    int32_t demodulate;   /* 0 or 1 */
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;
    int32_t feature_spp;  /* >= 1; used where features are traced (prt_accum_*_denoised) */
    int32_t reserved;     /* must be 0 */
} PrtDenoiseParams;
/* The defaults, measured on cornell-box, veach-mis and bathroom2 (tools/denoise_timing.py). */
void prt_denoise_defaults(PrtDenoiseParams* p);

/* Synchronous: features of the frame into host buffers. */
int prt_render_features(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params, int32_t feature_spp,
                        float* albedo, float* normal, float* depth, int32_t* prim);
/* Same into device buffers, asynchronous on hip_stream. */
int prt_render_features_device(PrtScene* scene, const PrtCamera* cam, const PrtRenderParams* params, int32_t feature_spp,
                               void* d_albedo, void* d_normal, void* d_depth, void* d_prim, void* hip_stream);
/* Synchronous: the filter on host buffers (rgb / albedo / normal [h][w][3], depth [h][w], out [h][w][3]; out may not alias
 * an input).  The scene only supplies the device and the filter's scratch (64 bytes per pixel, kept between calls). */
int prt_denoise(PrtScene* scene, int32_t w, int32_t h, const float* rgb, const float* albedo, const float* normal,
                const float* depth, const PrtDenoiseParams* params, float* out);
/* Same on device buffers, asynchronous on hip_stream.  Calls on one scene are ordered by the library (they share the scratch). */
int prt_denoise_device(PrtScene* scene, int32_t w, int32_t h, const void* d_rgb, const void* d_albedo, const void* d_normal,
                       const void* d_depth, const PrtDenoiseParams* params, void* d_out, void* hip_stream);
/* The accumulator's frame, denoised: prt_accum_resolve's fp32 frame through prt_denoise_device, guided by
 * prt_render_features of the accumulator's frozen camera and params (params->feature_spp samples).  Works on plain and
 * adaptive accumulators.  The features are traced once and cached; the cache is dropped on prt_accum_reset and on a scene
 * generation change (prt_scene_update_vertices), and retraced for another feature_spp.  d_rgb_f32 / d_rgb_u8 (W*H*3, either
 * may be NULL, not both): the denoised frame and exactly the bytes prt_tonemap_srgb8 makes of it.  Asynchronous on
 * hip_stream.  PRT_E_INVALID for nranks > 1: a tile share lacks its neighbours' pixels. */
int prt_accum_resolve_denoised(PrtAccum* acc, const PrtDenoiseParams* params, void* d_rgb_f32, void* d_rgb_u8, void* hip_stream);
/* Synchronous: the denoised frame into a W*H*3 host buffer. */
int prt_accum_read_denoised(PrtAccum* acc, const PrtDenoiseParams* params, float* rgb_f32);

/*
 * Variance-guided filter (the spatial colour weights of SVGF: Schied et al., HPG 2017), driven by the moments an adaptive
 * accumulator keeps.  A pixel's colour tolerance is its own estimated standard deviation: a firefly has a large variance,
 * accepts its calm neighbours and is pulled down; a lamp has a small one and stays sharp.
 *
 * Variance of the mean, from an adaptive accumulator (the quantities of the adaptive rule above): per pixel
 *     var_mean = max(0, moment - S^2 / n_p) / (C - 1) / n_p,   C = n_p / batch,  S = Y(sum)
 * in fp64 without fused multiply-adds, rounded to fp32; 0 where n_p == 0 (not owned, or nothing rendered).  It is the
 * variance of the pixel's mean luminance, in the units of the resolved frame.  An adaptive accumulator with min_spp ==
 * max_spp is a uniform render, so every user has the variance for the price of the moments.
 *
 * Filter: the inputs of prt_denoise plus a variance plane [h][w] (fp32).  A variance that is negative, NaN or infinite is
 * taken as 0; with demodulate = 1 it is divided by Y(max(a, 1e-3))^2 on the way in and multiplied back on the way out.
 * Level i (step 2^i, the 5x5 B3 taps and the tap-skipping rules of prt_denoise: taps outside the image, taps with a
 * non-finite colour, and hit / miss pairs while the depth term is on):
 *     g_p  = 3x3 binomial blur ((1,2,1) x (1,2,1) / 16) of the current variance plane around p, with step 1 at every
 *            level, renormalised over the taps inside the image
 *     e_c  = |Y(c_p) - Y(c_q)| / (sigma_color sqrt(g_p) + 1e-4)      (the kernel evaluates it as |Y(c_p - c_q)|: Y is
 *            linear, so the two are equal, and in fp32 close colours subtract exactly before the weighting)
 *     w    = h(dx) h(dy) exp(-(e_c + |n_p-n_q|^2 / sigma_normal^2 + Dz + |a_p-a_q|^2 / sigma_albedo^2))
 *     c'_p = sum w c_q / sum w,    v'_p = sum w^2 v_q / (sum w)^2
 * sigma_color multiplies the standard deviation and is NOT halved per level (the shrinking variance does that job);
 * sigma_color <= 0 or +inf switches the colour term off.  A non-finite centre colour gives colour 0 and variance 0.
 * iterations = 0 copies the colour and the sanitised variance.  The restatement in numpy is
 * tests/denoise_guided_model.py.  fp32, deterministic; the scratch is prt_denoise's (the variance rides in the colour
 * plane's fourth lane).
 */
/* prt_denoise_defaults with the guided filter's sigma_color and levels (tools/denoise_guided_timing.py). */
void prt_denoise_guided_defaults(PrtDenoiseParams* p);
/* Synchronous, host buffers; variance [h][w], out_variance [h][w] may be NULL.  PRT_E_INVALID for a null required buffer
 * or an output that aliases an input. */
int prt_denoise_guided(PrtScene* scene, int32_t w, int32_t h, const float* rgb, const float* variance, const float* albedo,
                       const float* normal, const float* depth, const PrtDenoiseParams* params, float* out, float* out_variance);
/* Same on device buffers, asynchronous on hip_stream; ordered with prt_denoise_device calls on the scene (one scratch). */
int prt_denoise_guided_device(PrtScene* scene, int32_t w, int32_t h, const void* d_rgb, const void* d_variance,
                              const void* d_albedo, const void* d_normal, const void* d_depth, const PrtDenoiseParams* params,
                              void* d_out, void* d_out_variance, void* hip_stream);
/* The variance of the mean of every pixel into a W*H fp32 device buffer, asynchronous on hip_stream.  PRT_E_INVALID for a
 * plain accumulator (it keeps no moments) and before 2 * batch samples (a pixel needs two batches). */
int prt_accum_variance(PrtAccum* acc, void* d_var_f32, void* hip_stream);
/* Synchronous: the same into a W*H host buffer. */
int prt_accum_read_variance(PrtAccum* acc, float* var_f32);
/* prt_accum_resolve's fp32 frame and prt_accum_variance through prt_denoise_guided_device, with the cached features of
 * prt_accum_resolve_denoised (one cache, the same invalidation).  Outputs as there.  PRT_E_INVALID as for
 * prt_accum_variance, and for nranks > 1. */
int prt_accum_resolve_denoised_guided(PrtAccum* acc, const PrtDenoiseParams* params, void* d_rgb_f32, void* d_rgb_u8,
                                      void* hip_stream);
/* Synchronous: the guided-denoised frame into a W*H*3 host buffer. */
int prt_accum_read_denoised_guided(PrtAccum* acc, const PrtDenoiseParams* params, float* rgb_f32);

#ifdef __cplusplus
}
#endif
#endif /* PRT_H */
