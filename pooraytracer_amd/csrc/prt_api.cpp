// prt_api.cpp — the C ABI of libprt_hip.so (include/prt.h).  Host orchestration only: scene
// preparation on create, SoA upload, kernel launches, counters.  There is no CPU compute path:
// every compute entry point needs a HIP device and fails with PRT_E_NO_DEVICE / PRT_E_HIP otherwise.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "mesh_topology.h"
#include "prt_host.h"
#include "prt_launch.h" // every launcher of the .hip files, declared once

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
// A failure's text survives the cleanup that follows it (calls that may fail again, or succeed): restored on scope exit.
struct KeepError {
    const std::string msg = g_err;
    ~KeepError() { g_err = msg; }
};
// Developer / test hooks are environment variables (PRT_TUNE_*: scheduling thresholds, table sizes, layouts for A/B runs;
// PRT_TEST_*: failure injection; PRT_VALIDATE_BVH).  The shipped libprt_hip.so does NOT read them: only a build with
// -DPRT_DEV_HOOKS=1 does (pooraytracer_amd/build.py builds that one as libprt_hip_dev.so for the tests and sweep tools
// that need it), so no environment variable can change what the production library schedules or make it fail.
#ifndef PRT_DEV_HOOKS
#define PRT_DEV_HOOKS 0
#endif
#if PRT_DEV_HOOKS
const char* dev_env(const char* name) { return std::getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; } // (not constexpr: call sites pass the result on to atoi)
#endif

int hip_fail(const std::string& who, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? PRT_E_OOM : PRT_E_HIP, who + ": " + hipGetErrorString(e));
}

// Owners of device memory and events: freed (destroyed) when they go, on whatever device is current then.
struct HipFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
template <typename T = void>
using DevBuf = std::unique_ptr<T, HipFree>;
struct HipHostFree {
    void operator()(void* p) const { (void)hipHostFree(p); }
};
struct EventDestroy {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
using Event = std::unique_ptr<std::remove_pointer<hipEvent_t>::type, EventDestroy>;

template <typename T>
hipError_t dev_alloc(DevBuf<T>& out, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    out.reset(e == hipSuccess ? static_cast<T*>(p) : nullptr);
    return e;
}
hipError_t make_event(Event& out, unsigned flags) {
    hipEvent_t e = nullptr;
    const hipError_t r = hipEventCreateWithFlags(&e, flags);
    out.reset(r == hipSuccess ? e : nullptr);
    return r;
}

// A device buffer kept between calls and grown on demand.  A buffer whose users call used() gets a "last user done"
// event: a later call's stream waits for it first, so the buffer is the previous call's until that call has ended.
struct Scratch {
    DevBuf<> p;
    size_t cap = 0;
    Event done;
    // Waits (on st) for the last user, then makes room for `bytes` (hipFree of the old buffer waits for the device).
    hipError_t reserve(size_t bytes, hipStream_t st) {
        hipError_t e = done ? hipStreamWaitEvent(st, done.get(), 0) : hipSuccess;
        if (e != hipSuccess || cap >= bytes) return e;
        if (done && (e = hipEventSynchronize(done.get())) != hipSuccess) return e;
        p.reset();
        cap = 0;
        if ((e = dev_alloc(p, bytes)) == hipSuccess) cap = bytes;
        return e;
    }
    hipError_t used(hipStream_t st) {
        const hipError_t e = done ? hipSuccess : make_event(done, hipEventDisableTiming);
        return e == hipSuccess ? hipEventRecord(done.get(), st) : e;
    }
    template <typename T>
    T* get() const { return static_cast<T*>(p.get()); }
};

// Device copies of one call's host buffers, freed on every way out.  After the first failure every step is skipped and
// `e` keeps that failure.
struct Staging {
    std::vector<DevBuf<>> bufs;
    hipError_t e = hipSuccess;
    void* out(size_t bytes) {
        DevBuf<> b;
        if (e == hipSuccess) e = dev_alloc(b, std::max<size_t>(bytes, 16));
        bufs.push_back(std::move(b));
        return bufs.back().get();
    }
    void* in(const void* src, size_t bytes) { // nullptr in -> nullptr out
        if (!src) return nullptr;
        void* d = out(bytes);
        if (e == hipSuccess) e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    void sync(hipEvent_t ev = nullptr) { // the device, or the event's work
        if (e == hipSuccess) e = ev ? hipEventSynchronize(ev) : hipDeviceSynchronize();
    }
    void down(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    }
    int status(const std::string& who) const { return e == hipSuccess ? PRT_OK : hip_fail(who, e); }
};

// What the render kernels of one precision get: the scene tables, resident blocks per CU of the production, the counting
// and the PLAIN instantiation (k_render; 0: the scene's frames have no PLAIN form) and of its DIFFUSE form (0: none), the
// light-tree nodes / light triangles / materials staged in LDS (all 0 = the kernels without LDS tables), and the traversal stack entries per lane.
template <typename R>
struct KernelConfig {
    DSceneT<R> d{};
    int blocks_per_cu[4] = {0, 0, 0, 0};
    int blocks_per_cu_rays = 0; // ... and of the ray-batch instantiation (prt_ray_color), queried by its first call
    int light_lds = 0, ltri_lds = 0, mat_lds = 0;
    int stack_depth = PRT_STACK_DEPTH;
};
} // namespace

extern "C" int prt_dev_hooks(void) { return PRT_DEV_HOOKS; }

// The form of the last K3 launch (prt.h, prt_last_render_form): kept by the dev-hooks build only.
// A DIFFUSE launch is a PLAIN launch to prt_last_render_form; prt_last_render_subform tells the two apart.
#if PRT_DEV_HOOKS
static std::atomic<int> g_render_form{PRT_RENDER_FORM_UNKNOWN}, g_render_subform{PRT_RENDER_SUBFORM_UNKNOWN};
static void note_render_form(bool plain, bool diffuse) {
    g_render_form = plain ? PRT_RENDER_FORM_PLAIN : PRT_RENDER_FORM_GENERIC;
    g_render_subform = plain && diffuse ? PRT_RENDER_SUBFORM_DIFFUSE : PRT_RENDER_SUBFORM_NONE;
}
extern "C" int prt_last_render_form(void) { return g_render_form; }
extern "C" int prt_last_render_subform(void) { return g_render_subform; }
#else
static void note_render_form(bool, bool) {}
extern "C" int prt_last_render_form(void) { return PRT_RENDER_FORM_UNKNOWN; }
extern "C" int prt_last_render_subform(void) { return PRT_RENDER_SUBFORM_UNKNOWN; }
#endif

#define PRT_HIP_AS(who, call)                                                                           \
    do {                                                                                                \
        const hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return hip_fail(who, e_);                                                 \
    } while (0)
#define PRT_HIP(call) PRT_HIP_AS(#call, call)

struct PrtScene {
    // host side
    std::vector<prt::HostTri> tris;
    std::vector<DMaterial> mats;
    std::vector<DTexture> texs;
    std::vector<double> texels_lin; // GetPixel() of every texel (Texture.cpp:50-65)
    size_t n_texel_reals = 0;       // reals of the texel array resident on the device (16 per texel as footprints, 3 as plain texels)
    size_t tex_footprint_bytes = 0; // ... of which footprint records (fp64 bytes)
    uint32_t tex_layouts = 0;       // bit 0: some texture is stored as footprints, bit 1: some as plain texels
    prt::LightTree lights;
    prt::BuiltBVH bvh;
    std::vector<uint64_t> mesh_first; // mesh structure, kept for prt_scene_update_vertices
    std::vector<int32_t> mesh_mat;
    std::vector<int32_t> light_meshes; // PrtSceneDesc.light_meshes when given
    bool explicit_lights = false;
    bool device_bvh = false; // PRT_SCENE_DEVICE_BVH: the tree is built in prt_scene_upload, on the GPU
    uint64_t generation = 0; // bumped by every prt_scene_update_vertices: an accumulator's sums belong to one geometry
    PrtBvhInfo bvh_info{};
    // device side
    int device = -1;
    int n_cu = 0;
    int blocks_wanted = 0; // what the production kernel's register allocation allows (occupancy without LDS tables)
    int feat = 0; // material features of the scene (1 textures, 2 Phong, 4 CookTorrance) -> K3 permutation
    bool all_diffuse = false; // prt::materials_all_diffuse(mats), taken where the table is uploaded: the scene's PLAIN frames have the DIFFUSE form
    KernelConfig<double> k64;
    // fp32 fast mode: float copies of the tables, made on the first PRT_PRECISION_F32 call (ensure_f32)
    KernelConfig<float> k32;
    bool f32_ready = false;
    int stack_need = PRT_STACK_DEPTH;                   // stack entries a traversal of the resident tree can need at most
    const DNode* d_nodes_shallow = nullptr;             // the same binary tree collapsed for PRT_STACK_SHALLOW entries (host build, deep trees), or null
    uint32_t n_nodes_shallow = 0;
    std::vector<DevBuf<>> allocs;
    // prt_scene_refit: the leaf order stays resident from the upload on (4 bytes per triangle); the rest is allocated by
    // the first refit after an upload and lives as long as the upload (all of it in `allocs`)
    const uint32_t* d_order = nullptr; // BVH leaf position -> triangle index in description order
    struct Refit {
        float* d_tbox = nullptr;       // per leaf position the triangle's fp32 box (lo[3], hi[3]) relative to the grid origin
        uint32_t *d_parent = nullptr, *d_cnt = nullptr;       // per node of d.nodes: its parent, the climb's arrival counter
        uint32_t *d_parent_sh = nullptr, *d_cnt_sh = nullptr; // ... of d_nodes_shallow
        void* d_scratch = nullptr;     // partials of the reductions
        prt::RefitCheck* d_check = nullptr;
        double* d_sah = nullptr;       // [0] SAH cost of the tree as built, [1] after the last refit
        Event ev0, ev1, ev2;           // timed: start of the records, start of the boxes, end
        Event done;                    // behind the refit's last kernel: every later call waits for it
        bool pending = false;          // `done` has been recorded
        uint64_t count = 0;            // successful refits since the upload
    } refit;
    Scratch refit_in;        // prt_scene_refit: device copies of the caller's host arrays (kept between calls)
    bool host_stale = false; // prt_scene_refit_device moved the geometry past the host triangles
    Event feat_done;         // behind the last prt_render_features* kernel (it uses no call slot): a refit waits for it
    bool feat_pending = false;
    // prt_scene_set_dynamic_lights: an emitter may move under a refit or a rebuild, and the light tree, its records and its
    // O(1) tables follow.  The scene then keeps TWO device copies of the light arrays: the resident one (what k64.d / k32.d
    // point to) and a spare one, which a light update fills and verifies while calls in flight still read the resident
    // one; the writing phase swaps them.  (The spare's last readers were issued before the previous swap, and that update's
    // writing phase waited for them: a new update, which waits for the previous one, finds the spare free.)
    bool dynamic_lights = false; // survives upload / update_vertices
    struct LightArrays {         // capacities in elements (words for tab); every array is owned by `allocs`
        void *nodes = nullptr, *tris = nullptr, *tab = nullptr, *nodes32 = nullptr, *tris32 = nullptr;
        size_t cap_nodes = 0, cap_tris = 0, cap_tab = 0, cap_nodes32 = 0, cap_tris32 = 0;
    };
    LightArrays light_res, light_spare;
    // prt_scene_set_distance_queries: while it is on, an uploaded scene keeps the fp64 corners of every triangle in BVH leaf
    // order (96 bytes each, owned by `allocs`); upload, refit and rebuild keep the table in step with the resident geometry
    bool distance_queries = false; // survives upload / update_vertices
    DTriCorners* d_corners = nullptr;
    // prt_scene_set_signed_queries: while it is on (distance queries are then on too), an uploaded scene also keeps the ids,
    // adjacency lists, face terms and pseudonormals of pseudonormals.hip (all owned by `allocs`; `signed_bytes` of them).  The
    // ids and lists are in description order and belong to the topology: upload and switch-on make them, refit and rebuild
    // keep them and refresh face terms and pseudonormals behind the corner gather.
    bool signed_queries = false; // survives upload / update_vertices
    prt::DSignedTables sq;
    size_t signed_bytes = 0;
    // prt_scene_set_winding_queries: while it is on (distance queries are then on too), an uploaded scene also keeps the
    // moments of winding_number.hip, four 64-byte records per node of k64.d.nodes (owned by `allocs`).  They belong to the
    // tree and the corners: upload and switch-on make them, a refit refreshes them behind its boxes, a rebuild makes the new
    // tree's in an array of its own.
    bool winding_queries = false; // survives upload / update_vertices
    prt::DWindingMoment* d_moments = nullptr;
    struct LightUpdate {
        double* d_gather = nullptr;    // per light triangle, resident CDF order: 9 doubles of new vertices, then (second half) of vertex normals
        std::vector<double> h_gather;  // ... read back with the refit's decision
        Scratch tmp;                   // flag word, the full tree, per-table subtree roots and areas: inputs of the device fill
        prt::LightTree next;           // the tree of the new positions, resident after the swap
        prt::LightTablePlan plan;
        std::vector<uint32_t> words;   // the filled tables, read back with the verification flag
        uint32_t flag = 0;
        std::vector<DLightNodeT<float>> ln32;
        std::vector<DLightTriT<float>> lt32;
        std::vector<int32_t> prims;        // the emitter triangles and their host records before the update (a refusal or a
        std::vector<prt::HostTri> saved;   // failure before the swap puts them back)
        bool staged = false;               // the spare holds a verified copy for `next`, waiting for the swap
        bool staged_relaid = false, staged_dropped = false, staged_tables = false;
        Event g0, g1, t0, t1;              // timed: the gather (the refit's first phase), the table fill + verification
        bool tables_timed = false;
        uint64_t count = 0;                // light updates since the upload
        double host_tree_ms = 0.0, gather_ms = 0.0;            // of the last light update (taken over at the swap)
        double staged_host_tree_ms = 0.0, staged_gather_ms = 0.0; // of the update being staged
        int fail_alloc_at = -1, n_allocs = 0; // test hook (PRT_TEST_FAIL_LIGHT_STAGE=k): the k-th allocation of a staging reports out-of-memory
        uint32_t tables_dropped = 0, relaid = 0;
    } lu;
    // Every call that reads the geometry first waits, on its stream, for the last refit's end.
    hipError_t after_refit(hipStream_t st) const {
        return refit.pending ? hipStreamWaitEvent(st, refit.done.get(), 0) : hipSuccess;
    }
    // Per-call device state, double-buffered: consecutive calls alternate slots, so a caller that
    // alternates two streams (and two framebuffers) can have frame k+1 filling the GPU while the last
    // long paths of frame k drain — the two launches never share counters, partial sums or events.
    struct CallSlot {
        DevBuf<DCounters> d_ctr;
        Scratch partial; // K3's item sums (doubles)
        Event ev0, ev1;
        Event done; // recorded behind the last kernel of the call that used this slot
        bool timed = false;
        bool counted = false;
        uint64_t samples = 0; // camera samples of the call (render: owned pixels inside the image x spp; the kernel does not count them)
        // A call's start: counters cleared, then ev0 (the start of the timed part) ...
        hipError_t start(hipStream_t st) {
            const hipError_t e = hipMemsetAsync(d_ctr.get(), 0, sizeof(DCounters), st);
            return e == hipSuccess ? hipEventRecord(ev0.get(), st) : e;
        }
        // ... ev1 (its end) ...
        hipError_t stop(hipStream_t st) { return hipEventRecord(ev1.get(), st); }
        // ... and done, behind the call's last kernel.
        hipError_t finish(hipStream_t st, bool count, uint64_t n) {
            const hipError_t e = hipEventRecord(done.get(), st);
            if (e == hipSuccess) {
                timed = true;
                counted = count;
                samples = n;
            }
            return e;
        }
        // After the counters have been cleared: the pointers K3 reads from them (DCounters::pixel_list / trace).
        hipError_t set_pointers(hipStream_t st, const void* pixel_list, void* trace) {
            if (!pixel_list && !trace) return hipSuccess; // zeroed already
            const void* ptrs[2] = {pixel_list, trace};
            return hipMemcpyAsync(reinterpret_cast<char*>(d_ctr.get()) + offsetof(DCounters, pixel_list), ptrs, sizeof(ptrs),
                                  hipMemcpyHostToDevice, st);
        }
        // ... and the ray batch of prt_ray_color (DCounters::ray_list / key_list)
        hipError_t set_rays(hipStream_t st, const void* rays, const void* keys) {
            const void* ptrs[2] = {rays, keys};
            return hipMemcpyAsync(reinterpret_cast<char*>(d_ctr.get()) + offsetof(DCounters, ray_list), ptrs, sizeof(ptrs),
                                  hipMemcpyHostToDevice, st);
        }
    };
    // prt_trace_closest_sorted_device: K4's keys, values and the permutation — one scratch area per scene, kept between
    // calls; a call on another stream first waits for the previous sorted call's end
    Scratch sort;
    CallSlot slots[2];
    int cur = 0; // slot of the most recent call (prt_get_counters reads it)
    // Next slot for an asynchronous call on `st`.  A slot may still be in use by a call issued two calls ago on
    // another stream (three streams, or a trace call between two pipelined renders): its counters and partial
    // sums must not be reset under a running kernel, so the new call's stream first waits for that call's end.
    CallSlot* next_slot(hipStream_t st, hipError_t* err) {
        cur ^= 1;
        CallSlot& q = slots[cur];
        *err = q.timed ? hipStreamWaitEvent(st, q.done.get(), 0) : hipSuccess;
        if (*err == hipSuccess) *err = after_refit(st);
        return &q;
    }
    PrtCounters last{};
    Scratch multi_fb; // prt_render_multi: this device's full-size fp32 framebuffer (kept between frames)
    // prt_denoise_device: the filter's scratch (prt_denoise.hip), kept between calls; a call waits (on its stream) for the
    // previous call's end before it reuses it
    Scratch dn;

    int fail_upload_at = -1, n_uploads = 0; // test hook (PRT_TEST_FAIL_UPLOAD=k): the k-th table upload reports out-of-memory
    // One table to the device (at least 256 bytes); `inject`: it counts as an upload for PRT_TEST_FAIL_UPLOAD.
    int put(const void* src, size_t bytes, DevBuf<>& out, bool inject = true) {
        if (inject && n_uploads++ == fail_upload_at) return fail(PRT_E_OOM, "prt_scene_upload: injected allocation failure (PRT_TEST_FAIL_UPLOAD)");
        PRT_HIP_AS("hipMalloc", dev_alloc(out, std::max<size_t>(bytes, 256)));
        if (bytes) PRT_HIP(hipMemcpy(out.get(), src, bytes, hipMemcpyHostToDevice));
        return PRT_OK;
    }
    template <typename T>
    int up(const std::vector<T>& v, const T** out, bool inject = true) {
        DevBuf<> p;
        if (int rc = put(v.data(), v.size() * sizeof(T), p, inject)) return rc;
        *out = static_cast<const T*>(p.get());
        allocs.push_back(std::move(p));
        return PRT_OK;
    }
    // A device array that lives as long as the upload (at least 256 bytes).
    int alloc(size_t bytes, void** out) {
        DevBuf<> p;
        PRT_HIP_AS("hipMalloc", dev_alloc(p, std::max<size_t>(bytes, 256)));
        *out = p.get();
        allocs.push_back(std::move(p));
        return PRT_OK;
    }
    // The owner of a resident array, out of `allocs` (null, or not there: an empty owner).
    DevBuf<> take(const void* p) {
        DevBuf<> out;
        for (auto it = allocs.begin(); p && it != allocs.end(); ++it)
            if (it->get() == p) {
                out = std::move(*it);
                allocs.erase(it);
                break;
            }
        return out;
    }
    // What k32.d shares with k64.d: the light tables' place and totals (thresholds are floats in either mode), the tree (the
    // 32-entry collapse where the scene keeps one), the grid, the texture headers, the counts.  Called by whoever changes one.
    void share_with_f32() {
        const DScene& d = k64.d;
        DSceneT<float>& f = k32.d;
        f.light_tab = d.light_tab;
        f.light_root = d.light_root;
        f.n_lights = d.n_lights;
        f.light_area = (float)d.light_area;
        f.nodes = d_nodes_shallow ? d_nodes_shallow : d.nodes;
        f.n_nodes = d_nodes_shallow ? n_nodes_shallow : d.n_nodes;
        f.textures = d.textures;
        f.n_tris = d.n_tris;
        f.tex_compact = d.tex_compact;
        f.slab_scale = d.slab_scale;
        for (int a = 0; a < 3; ++a) {
            f.grid_origin[a] = d.grid_origin[a];
            f.grid_step[a] = d.grid_step[a];
        }
    }
    // The quantisation grid of the resident tree, in every copy: the host tree's and both DScenes'.
    void set_grid(const float origin[3], const float step[3], float coord_scale) {
        DScene& d = k64.d;
        // box coordinates reach the slab test relative to the grid origin: what bounds its rounding is the grid's extent
        double e = 0.0;
        for (int a = 0; a < 3; ++a) e = std::max(e, 65535.0 * (double)step[a]);
        bvh.coord_scale = coord_scale;
        for (int a = 0; a < 3; ++a) {
            bvh.grid_origin[a] = d.grid_origin[a] = origin[a];
            bvh.grid_step[a] = d.grid_step[a] = step[a];
        }
        d.slab_scale = std::nextafter((float)e, std::numeric_limits<float>::infinity());
        if (f32_ready) share_with_f32();
    }
    // A tree the device builder made is the scene's from here on (its arrays have an owner already): what the kernels, the
    // refit, the host tree's record and the reports get of it.
    void adopt_device_tree(const prt::DeviceBVH& db) {
        k64.d.nodes = db.d_nodes;
        k64.d.n_nodes = db.n_nodes;
        d_order = db.d_order;
        bvh.depth = db.depth;
        last.bvh_nodes = bvh_info.n_nodes = db.n_nodes;
        last.bvh_depth = bvh_info.depth = db.depth;
        bvh_info.built_on_device = 1;
        bvh_info.build_ms = db.ms_total;
        bvh_info.sort_ms = db.ms_sort;
        bvh_info.tree_ms = db.ms_tree;
        bvh_info.split_ms = db.ms_split;
    }
    void set_stack_need(int need) { stack_need = std::min(std::max(need, 1), PRT_STACK_DEPTH); }
    // The 32-entry collapse of a deep host-built tree becomes resident (same leaf order as the full tree: the records fit
    // both), unless it is already or the scene has none.  Not one of the uploads PRT_TEST_FAIL_UPLOAD counts.
    int shallow_resident() {
        if (stack_need <= PRT_STACK_SHALLOW || d_nodes_shallow || bvh_info.built_on_device || bvh.nodes_shallow.empty()) return PRT_OK;
        if (int rc = up(bvh.nodes_shallow, &d_nodes_shallow, false)) return rc;
        n_nodes_shallow = (uint32_t)bvh.nodes_shallow.size();
        return PRT_OK;
    }
    void release() {
        if (device >= 0) (void)hipSetDevice(device);
        allocs.clear();
        d_order = nullptr;
        d_corners = nullptr;
        sq = prt::DSignedTables();
        signed_bytes = 0;
        d_moments = nullptr;
        refit = Refit();
        light_res = light_spare = LightArrays();
        lu = LightUpdate();
        refit_in = Scratch();
        multi_fb = Scratch();
        sort = Scratch();
        dn = Scratch();
        for (CallSlot& q : slots) q = CallSlot();
        k64 = KernelConfig<double>();
        k32 = KernelConfig<float>();
        device = -1;
        f32_ready = false;
    }
};

// A tree of `n_nodes` nodes may become a scene's: PRT_E_LIMIT beyond PRT_MAX_NODES (prt::node_count_ok).  Asked where a tree
// is made, by either builder, before anything is allocated for it or traverses it.
// Test hook PRT_TEST_CLAIM_NODES=<n> (dev-hooks build only): the tree in question claims n nodes, whatever it has — the limit
// is tested without a tree of 4 GB.
static int check_node_count(const std::string& who, size_t n_nodes) {
    if (const char* e = dev_env("PRT_TEST_CLAIM_NODES")) n_nodes = (size_t)std::strtoull(e, nullptr, 10);
    std::string err;
    if (!prt::node_count_ok(n_nodes, &err)) return fail(PRT_E_LIMIT, who + ": " + err);
    return PRT_OK;
}

// Test hook PRT_TEST_DUMP_BVH=<file> (dev-hooks build only): the traversal tree of a scene, as the kernels get it, for the
// fp64 tree model of the tests (tests/bvh_model.py).  Little-endian: a 72-byte header
//   u32 magic 'PBVH', u32 version 1, u64 n_tris, u64 n_nodes, u32 built_on_device, u32 depth, i32 stack_need, u32 node_bytes,
//   f32 grid_origin[3], f32 grid_step[3], f32 coord_scale, u32 0
// then the DNode array, then the leaf order (u32 per triangle: leaf position -> triangle index in description order).
struct BvhDumpHeader {
    uint32_t magic, version;
    uint64_t n_tris, n_nodes;
    uint32_t built_on_device, depth;
    int32_t stack_need;
    uint32_t node_bytes;
    float grid_origin[3], grid_step[3], coord_scale;
    uint32_t zero;
};
static_assert(sizeof(BvhDumpHeader) == 72, "dump header layout");

static int dump_bvh(const char* path, const PrtScene* s, const DNode* nodes, size_t n_nodes, const uint32_t* order,
                    int stack_need) {
    BvhDumpHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = 0x48564250u; // "PBVH"
    h.version = 1;
    h.n_tris = s->tris.size();
    h.n_nodes = n_nodes;
    h.built_on_device = s->bvh_info.built_on_device;
    h.depth = s->bvh_info.depth;
    h.stack_need = stack_need;
    h.node_bytes = sizeof(DNode);
    for (int a = 0; a < 3; ++a) {
        h.grid_origin[a] = s->bvh.grid_origin[a];
        h.grid_step[a] = s->bvh.grid_step[a];
    }
    h.coord_scale = s->bvh.coord_scale;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(PRT_E_INVALID, std::string("PRT_TEST_DUMP_BVH: cannot open ") + path);
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1;
    ok = ok && std::fwrite(nodes, sizeof(DNode), n_nodes, f) == n_nodes;
    ok = ok && std::fwrite(order, sizeof(uint32_t), s->tris.size(), f) == s->tris.size();
    ok = (std::fclose(f) == 0) && ok;
    return ok ? PRT_OK : fail(PRT_E_INVALID, std::string("PRT_TEST_DUMP_BVH: cannot write ") + path);
}

template <typename T, typename U>
static void conv_arr(T* o, const U* a, int n) {
    for (int i = 0; i < n; ++i) o[i] = (T)a[i];
}

// How much of the material table, the light triangles and the light tree a render kernel stages in LDS, given the
// bytes a block may spend on them (record sizes differ between the fp64 and the fp32 kernels).
static void size_tables(const PrtScene* s, int budget, size_t mat_bytes, size_t ltri_bytes, size_t lnode_bytes, int* mat, int* ltri, int* light) {
    *mat = *ltri = *light = 0;
    const bool off = dev_env("PRT_TUNE_NO_LDS") && std::atoi(dev_env("PRT_TUNE_NO_LDS"));
    if (off || s->mats.empty() || s->mats.size() * mat_bytes > 8192 || (int)(s->mats.size() * mat_bytes) > budget) return;
    *mat = (int)s->mats.size();
    budget -= *mat * (int)mat_bytes;
    if (!s->lights.tris.empty() && s->lights.tris.size() <= 32 && (int)(s->lights.tris.size() * ltri_bytes) <= budget) {
        *ltri = (int)s->lights.tris.size();
        budget -= *ltri * (int)ltri_bytes;
    }
    *light = (int)std::min<size_t>(s->lights.nodes.size(), (size_t)(std::max(budget, 0) / (int)lnode_bytes));
    if (const char* e = dev_env("PRT_TUNE_LIGHT_LDS")) *light = std::min(*light, std::max(0, std::atoi(e)));
    if (const char* e = dev_env("PRT_TUNE_LTRI_LDS")) if (!std::atoi(e)) *ltri = 0;
}

// Whether a K3 launch of the scene's kernels of precision R with these launch values uses the PLAIN form (k_render): the
// launchers' render_plain decides, here for the occupancy query and for the launch alike.  PRT_TUNE_GENERIC=1 (developer): every
// launch keeps its generic kernel.
template <typename R>
static bool frame_plain(const PrtScene* s, const KernelConfig<R>& k, bool count, bool rays, int jitter, int scramble, int sample_lights) {
    const auto plain = std::is_same<R, double>::value ? prt::render_plain : prt32::render_plain;
    return plain(s->feat, count, rays, k.d.n_lights, k.ltri_lds, jitter, scramble, sample_lights);
}
static bool generic_forced() {
    const char* e = dev_env("PRT_TUNE_GENERIC");
    return e && std::atoi(e);
}
// ... and whether that PLAIN launch uses its DIFFUSE form: the launchers' render_diffuse decides, from the same values and the
// flag of the scene's material table (PrtScene::all_diffuse).  fp64 only.  PRT_TUNE_NO_DIFFUSE=1 (developer): a qualifying
// launch keeps the plain PLAIN kernel; PRT_TUNE_GENERIC=1 wins over both.
template <typename R>
static bool frame_diffuse(const PrtScene* s, const KernelConfig<R>& k, bool count, bool rays, int jitter, int scramble, int sample_lights) {
    return std::is_same<R, double>::value &&
           prt::render_diffuse(s->feat, count, rays, k.d.n_lights, k.ltri_lds, jitter, scramble, sample_lights, s->all_diffuse);
}
static bool diffuse_off() {
    const char* e = dev_env("PRT_TUNE_NO_DIFFUSE");
    return e && std::atoi(e);
}

// LDS tables and resident blocks per CU of the render kernels of one precision, for stacks of k.stack_depth entries.
// drop_tables: render without the tables when they would cost the production kernel a resident block (the budget is an
// estimate; the occupancy query is the truth).  Returns the blocks per CU without the tables (with drop_tables; else
// blocks_per_cu[0]).
template <typename R>
static int size_kernels(const PrtScene* s, KernelConfig<R>& k, bool drop_tables) {
    constexpr bool f64 = std::is_same<R, double>::value;
    const auto lds_budget = f64 ? prt::render_lds_budget : prt32::render_lds_budget;
    const auto table_bytes = f64 ? prt::render_table_bytes : prt32::render_table_bytes;
    const auto blocks_per_cu = f64 ? prt::render_blocks_per_cu : prt32::render_blocks_per_cu;
    size_tables(s, lds_budget(s->feat, k.stack_depth), sizeof(DMaterialT<R>), sizeof(DLightTriT<R>), sizeof(DLightNodeT<R>),
                &k.mat_lds, &k.ltri_lds, &k.light_lds);
    const bool pad = k.d.tri_stride == PRT_TRI_PAD_STRIDE(R) && sizeof(DTriT<R>) != PRT_TRI_PAD_STRIDE(R);
    const bool extra = !s->lights.tab.empty() || k.d.tex_compact != 0;
    auto blocks = [&](bool count, size_t tables, bool plain = false, bool diffuse = false) {
        return blocks_per_cu(count, s->feat, tables, k.stack_depth, pad, extra, false, plain, diffuse);
    };
    const size_t tables = table_bytes(k.light_lds, k.mat_lds, k.ltri_lds);
    k.blocks_per_cu[0] = blocks(false, tables);
    // a frame with default settings launches the PLAIN form where the scene has one: a function of its own, asked about on its own
    k.blocks_per_cu[2] = frame_plain(s, k, false, false, 0, 0, 1) ? blocks(false, tables, true) : 0;
    k.blocks_per_cu[3] = frame_diffuse(s, k, false, false, 0, 0, 1) ? blocks(false, tables, true, true) : 0; // ... and so is its DIFFUSE form
    const int wanted = drop_tables && tables != 0 ? blocks(false, 0) : k.blocks_per_cu[0];
    if (k.blocks_per_cu[0] < wanted || (k.blocks_per_cu[2] && k.blocks_per_cu[2] < wanted) ||
        (k.blocks_per_cu[3] && k.blocks_per_cu[3] < wanted)) { // a block per CU is worth far more than the tables
        k.mat_lds = k.ltri_lds = k.light_lds = 0;
        k.blocks_per_cu[0] = wanted;
        k.blocks_per_cu[2] = k.blocks_per_cu[3] = 0; // (no light triangles in LDS: no PLAIN form)
    }
    k.blocks_per_cu[1] = blocks(true, table_bytes(k.light_lds, k.mat_lds, k.ltri_lds));
    if (dev_env("PRT_TUNE_VERBOSE")) {
        if (f64)
            std::fprintf(stderr, "[prt] fp64 render kernels: %d blocks per CU, LDS tables: %d materials, %d light triangles, %d light nodes\n",
                         k.blocks_per_cu[0], k.mat_lds, k.ltri_lds, k.light_lds);
        else
            std::fprintf(stderr, "[prt] fp32 render kernels: %d blocks per CU, stacks %d, LDS tables: %d materials, %d light triangles, %d light nodes\n",
                         k.blocks_per_cu[0], k.stack_depth, k.mat_lds, k.ltri_lds, k.light_lds);
    }
    return wanted;
}

// Both precisions' kernels sized again, as at upload and in ensure_f32, for a resident scene whose tree or light tables
// changed (the ray-batch kernel's blocks per CU are asked for again by its next call).
static void size_kernels_again(PrtScene* s) {
    s->k64.blocks_per_cu_rays = 0;
    s->blocks_wanted = size_kernels(s, s->k64, true);
    if (s->f32_ready) {
        s->k32.blocks_per_cu_rays = 0;
        size_kernels(s, s->k32, false);
    }
}

// Resident blocks per CU of the ray-batch kernel of a scene (the production kernels' are queried at upload; this one by the
// first prt_ray_color call of its precision): same tables, stacks and record stride as the production kernel.
template <typename R>
static int rays_blocks_per_cu(const PrtScene* s, KernelConfig<R>& k) {
    if (!k.blocks_per_cu_rays) {
        constexpr bool f64 = std::is_same<R, double>::value;
        const size_t tables = (f64 ? prt::render_table_bytes : prt32::render_table_bytes)(k.light_lds, k.mat_lds, k.ltri_lds);
        const bool pad = k.d.tri_stride == PRT_TRI_PAD_STRIDE(R) && sizeof(DTriT<R>) != PRT_TRI_PAD_STRIDE(R);
        k.blocks_per_cu_rays = (f64 ? prt::render_blocks_per_cu : prt32::render_blocks_per_cu)(false, s->feat, tables, k.stack_depth, pad, true, true, false, false);
    }
    return k.blocks_per_cu_rays;
}

// The PRT_VARIANT_* byte of the production K3 instantiation a render in precision R launches: the choice launch_render makes,
// from the same fields.
template <typename R>
static uint32_t render_variant(const PrtScene* s, const KernelConfig<R>& k) {
    const bool llds = k.mat_lds != 0 || k.ltri_lds != 0 || k.light_lds != 0;
    const bool pad = k.d.tri_stride == PRT_TRI_PAD_STRIDE(R) && sizeof(DTriT<R>) != PRT_TRI_PAD_STRIDE(R);
    const bool extra = k.d.light_tab != nullptr || k.d.tex_compact != 0;
    return PRT_VARIANT_VALID | ((uint32_t)s->feat & PRT_VARIANT_PERM_MASK) | (llds ? PRT_VARIANT_LLDS : 0u) |
           (pad ? PRT_VARIANT_PAD : 0u) | (extra ? PRT_VARIANT_EXTRA : 0u);
}

// The host's tile layout of a frame (the device has its own copy: tile_pixel in prt_device.h).  tile_size 0 means 32, and
// the tile is rounded up to a multiple of 8 (at least 8); tiles are dealt round-robin over the ranks in row-major order,
// and tile row ty is rotated by 3 * ty.
struct TileLayout {
    int width, height, tile, tiles_x, tiles_y, n_tiles, rank, nranks, owned_tiles;
    uint64_t items_per_chunk; // owned_tiles * tile * tile
    TileLayout(const PrtCamera& c, const PrtRenderParams& p) : width(c.width), height(c.height), rank(p.rank), nranks(p.nranks) {
        tile = p.tile_size > 0 ? p.tile_size : 32;
        tile = std::max(8, (tile + 7) / 8 * 8);
        tiles_x = (width + tile - 1) / tile;
        tiles_y = (height + tile - 1) / tile;
        n_tiles = tiles_x * tiles_y;
        owned_tiles = n_tiles > rank ? (n_tiles - rank + nranks - 1) / nranks : 0;
        items_per_chunk = (uint64_t)owned_tiles * tile * tile;
    }
    // Pixel (x, y) lies in one of this rank's tiles.
    bool owns(int x, int y) const {
        const int tx = x / tile, ty = y / tile;
        const int kx = ((tx - 3 * ty) % tiles_x + tiles_x) % tiles_x;
        return (ty * tiles_x + kx) % nranks == rank;
    }
    // The pixels of this rank's tiles that lie inside the image.
    uint64_t owned_pixels() const {
        uint64_t px = 0;
        for (int k = rank; k < n_tiles; k += nranks) {
            const int ty = k / tiles_x, tx = (k - ty * tiles_x + 3 * ty) % tiles_x;
            px += (uint64_t)std::max(0, std::min(tile, width - tx * tile)) * (uint64_t)std::max(0, std::min(tile, height - ty * tile));
        }
        return px;
    }
    void set(DRenderParams& P) const {
        P.tile = tile; P.tiles_x = tiles_x; P.tiles_y = tiles_y; P.n_tiles = n_tiles;
        P.rank = rank; P.nranks = nranks; P.owned_tiles = owned_tiles; P.items_per_chunk = items_per_chunk;
    }
};

// What every K3 launch of the scene shares (render_impl, prt_render_samples); the callers set the samples, tiles, items
// and chunks of their launch.
// K3's one-pass vertex (prt_kernels.hip): lanes back from a shadow ray start their continuation ray between traversal
// rounds once this many of a wave's lanes wait for it; 65 = never, the next pass starts them.
#ifndef PRT_CHAIN_MIN_DEFAULT
#define PRT_CHAIN_MIN_DEFAULT 8
#endif
static DRenderParams base_params(const PrtScene* s, const PrtRenderParams* p) {
    DRenderParams P;
    std::memset(&P, 0, sizeof(P));
    P.max_depth = p->max_depth;
    P.sample_lights = p->sample_lights ? 1 : 0;
    P.rr = p->russian_roulette;
    P.inv_rr = 1.0 / p->russian_roulette;
    // wave scheduling thresholds: measured optima at the BASELINE spp with 4-wide nodes (flat within 2 %): lean 28 / 48 / 20,
    // others 20 / 40 / 12; the Phong permutations at three waves: leaf batch 32 (round 4, two sweeps and a four-fold A/B on
    // veach-mis: -0.75 %)
    P.keep = s->feat == 0 ? 28 : 20;
    P.leaf_batch = s->feat == 0 ? 48 : (s->feat & 2) ? 32 : 40; // (2 = Phong, as in s->feat above)
    P.inner_min = s->feat == 0 ? 20 : 12;
    P.chain_min = PRT_CHAIN_MIN_DEFAULT;
    for (int c = 0; c < 3; ++c) P.background[c] = p->background[c];
    P.seed_key = prt::seed_key(p->seed); // the seed is hashed on its own, once per launch (prt_device.h, Rng)
    P.jitter = p->pixel_jitter ? 1 : 0;
    P.light_lds = s->k64.light_lds;
    P.mat_lds = s->k64.mat_lds;
    P.ltri_lds = s->k64.ltri_lds;
    P.stack_depth = PRT_STACK_DEPTH;
    return P;
}

// The same launch for the fp32 kernels: reals rounded from the fp64 values, the fp32 kernels' own LDS tables and stacks.
static DRenderParamsT<float> to_f32(const DRenderParams& P, const KernelConfig<float>& k) {
    static_assert(sizeof(DRenderParamsT<float>) == 400, "DRenderParamsT changed: convert its new fields here");
    DRenderParamsT<float> o;
    std::memset(&o, 0, sizeof(o));
    o.spp = P.spp; o.max_depth = P.max_depth; o.sample_lights = P.sample_lights; o.chunks = P.chunks;
    o.rr = (float)P.rr; o.inv_rr = (float)P.inv_rr;
    conv_arr(o.background, P.background, 3);
    o.seed_key = P.seed_key;
    o.tile = P.tile; o.tiles_x = P.tiles_x; o.tiles_y = P.tiles_y; o.n_tiles = P.n_tiles;
    o.rank = P.rank; o.nranks = P.nranks; o.owned_tiles = P.owned_tiles; o.jitter = P.jitter;
    o.keep = P.keep; o.leaf_batch = P.leaf_batch; o.inner_min = P.inner_min; o.scramble = P.scramble; o.cached_min = P.cached_min; o.chain_min = P.chain_min;
    o.light_lds = k.light_lds; o.mat_lds = k.mat_lds; o.ltri_lds = k.ltri_lds;
    o.stack_depth = k.stack_depth;
    o.items_per_chunk = P.items_per_chunk; o.n_items = P.n_items;
    std::memcpy(o.chunk_begin, P.chunk_begin, sizeof(P.chunk_begin));
    return o;
}
static DCameraT<float> to_f32(const DCamera& C) {
    DCameraT<float> o;
    conv_arr(o.center, C.center, 3); conv_arr(o.pixel00, C.pixel00, 3);
    conv_arr(o.du, C.du, 3); conv_arr(o.dv, C.dv, 3);
    o.width = C.width; o.height = C.height;
    return o;
}

extern "C" {

int prt_abi_version(void) { return PRT_ABI_VERSION; }
const char* prt_last_error(void) { return g_err.c_str(); }

int prt_device_count(int* n) {
    if (!n) return fail(PRT_E_INVALID, "prt_device_count: null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(PRT_E_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *n = c;
    return PRT_OK;
}

int prt_scene_create(const PrtSceneDesc* desc, PrtScene** out) {
    if (!desc || !out) return fail(PRT_E_INVALID, "prt_scene_create: null argument");
    *out = nullptr;
    if (desc->n_tris && !desc->vertices) return fail(PRT_E_INVALID, "prt_scene_create: vertices is null");
    if (desc->n_meshes && (!desc->mesh_first_tri || !desc->mesh_material))
        return fail(PRT_E_INVALID, "prt_scene_create: mesh arrays are null");
    if (desc->n_materials && !desc->materials) return fail(PRT_E_INVALID, "prt_scene_create: materials is null");
    if (desc->n_textures && !desc->textures) return fail(PRT_E_INVALID, "prt_scene_create: textures is null");
    if (desc->n_meshes) {
        if (desc->mesh_first_tri[0] != 0 || desc->mesh_first_tri[desc->n_meshes] != desc->n_tris)
            return fail(PRT_E_INVALID, "prt_scene_create: mesh_first_tri must start at 0 and end at n_tris");
        for (uint32_t m = 0; m < desc->n_meshes; ++m) {
            if (desc->mesh_first_tri[m] > desc->mesh_first_tri[m + 1])
                return fail(PRT_E_INVALID, "prt_scene_create: mesh_first_tri must be ascending");
            if (desc->mesh_material[m] < 0 || (uint32_t)desc->mesh_material[m] >= desc->n_materials)
                return fail(PRT_E_INVALID, "prt_scene_create: mesh_material out of range");
        }
    } else if (desc->n_tris) {
        return fail(PRT_E_INVALID, "prt_scene_create: triangles without meshes");
    }
    if (desc->n_light_meshes && !desc->light_meshes) return fail(PRT_E_INVALID, "prt_scene_create: light_meshes is null");
    for (uint32_t i = 0; i < (desc->light_meshes ? desc->n_light_meshes : 0u); ++i)
        if (desc->light_meshes[i] < 0 || (uint32_t)desc->light_meshes[i] >= desc->n_meshes)
            return fail(PRT_E_INVALID, "prt_scene_create: light_meshes entry out of range");
    for (uint32_t i = 0; i < desc->n_materials; ++i) {
        const PrtMaterial& m = desc->materials[i];
        if (m.type < PRT_MAT_LAMBERTIAN || m.type > PRT_MAT_EMPTY)
            return fail(PRT_E_INVALID, "prt_scene_create: unknown material type");
        if (m.texture >= (int32_t)desc->n_textures) return fail(PRT_E_INVALID, "prt_scene_create: texture index out of range");
    }
    // NaN / infinite coordinates have no place in a BVH (the builders' orderings would be inconsistent)
    for (uint64_t i = 0; i < desc->n_tris * 9; ++i)
        if (!(std::fabs(desc->vertices[i]) <= 1e18)) // also catches NaN; the fp32 box tests need headroom below FLT_MAX
            return fail(PRT_E_INVALID, "prt_scene_create: vertex coordinate is not finite (or beyond 1e18)");
    PrtScene* s = new (std::nothrow) PrtScene();
    if (!s) return fail(PRT_E_OOM, "prt_scene_create: out of host memory");
    try {
        prt::setup_triangles(*desc, s->tris);
        s->mesh_first.assign(desc->mesh_first_tri, desc->mesh_first_tri + (desc->n_meshes ? desc->n_meshes + 1 : 0));
        s->mesh_mat.assign(desc->mesh_material, desc->mesh_material + desc->n_meshes);
        s->explicit_lights = desc->light_meshes != nullptr;
        if (s->explicit_lights) s->light_meshes.assign(desc->light_meshes, desc->light_meshes + desc->n_light_meshes);
        prt::setup_materials(*desc, s->mats);
        s->texs.resize(desc->n_textures);
        for (uint32_t i = 0; i < desc->n_textures; ++i) {
            const PrtTexture& t = desc->textures[i];
            DTexture& o = s->texs[i];
            o.width = t.width;
            o.height = t.height;
            o.channels = t.channels;
            o.has_data = (t.data && t.width > 0 && t.height > 0 && t.channels > 0) ? 1 : 0;
            o.offset = s->texels_lin.size();
            if (o.has_data) {
                // ImageTexture::GetPixel: colorScale * byte, SRGBToLinear for >= 3 channels, grey replicated otherwise
                double lut[256];
                for (int b = 0; b < 256; ++b) {
                    const double c = (1.0 / 255.0) * b;
                    lut[b] = (c <= 0.04045) ? c * (1. / 12.92) : std::pow((c + 0.055) * (1. / 1.055), 2.4);
                }
                const size_t npx = (size_t)t.width * t.height;
                s->texels_lin.reserve(s->texels_lin.size() + npx * 3);
                for (size_t i = 0; i < npx; ++i) {
                    const uint8_t* px = t.data + i * t.channels;
                    if (t.channels >= 3) {
                        s->texels_lin.push_back(lut[px[0]]);
                        s->texels_lin.push_back(lut[px[1]]);
                        s->texels_lin.push_back(lut[px[2]]);
                    } else {
                        const double g = (1.0 / 255.0) * px[0];
                        s->texels_lin.insert(s->texels_lin.end(), {g, g, g});
                    }
                }
            }
        }
        prt::build_light_tree(*desc, s->tris, s->mats, s->lights);
        s->device_bvh = (desc->flags & PRT_SCENE_DEVICE_BVH) && s->tris.size() >= 2;
        if (!s->device_bvh) {
            std::string err;
            const auto t0 = std::chrono::steady_clock::now();
            if (!prt::build_bvh(s->tris, s->bvh, &err)) {
                delete s;
                return fail(PRT_E_LIMIT, "prt_scene_create: " + err);
            }
            // For the test hook only: build_bvh has just decided for the real tree (the larger of its two collapses), and a
            // tree it let through passes here as well.  PRT_TEST_CLAIM_NODES makes this the CPU-side refusal the tests can reach.
            if (const int rc = check_node_count("prt_scene_create", s->bvh.nodes.size())) {
                delete s;
                return rc;
            }
            s->bvh_info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    } catch (const std::bad_alloc&) {
        delete s;
        return fail(PRT_E_OOM, "prt_scene_create: out of host memory");
    } catch (const std::exception& e) {
        delete s;
        return fail(PRT_E_INVALID, std::string("prt_scene_create: ") + e.what());
    }
    s->last.bvh_nodes = s->bvh.nodes.size();
    s->last.bvh_depth = s->bvh.depth;
    s->bvh_info.n_nodes = s->bvh.nodes.size();
    s->bvh_info.depth = s->bvh.depth;
    if (const char* p = dev_env("PRT_TEST_DUMP_BVH"))
        if (!s->device_bvh) {
            const int rc = dump_bvh(p, s, s->bvh.nodes.data(), s->bvh.nodes.size(), s->bvh.order.data(), s->bvh.stack_need);
            if (rc != PRT_OK) {
                delete s;
                return rc;
            }
        }
    *out = s;
    return PRT_OK;
}

void prt_scene_destroy(PrtScene* s) {
    if (!s) return;
    s->release();
    delete s;
}

int prt_scene_bvh_info(const PrtScene* s, PrtBvhInfo* out) {
    if (!s || !out) return fail(PRT_E_INVALID, "prt_scene_bvh_info: null argument");
    *out = s->bvh_info;
    out->node_bytes = (uint32_t)sizeof(DNode);
    out->width = PRT_BVH_WIDTH;
    out->tri_bytes = (uint32_t)sizeof(DTri);
    out->tri_stride = s->device >= 0 ? s->k64.d.tri_stride : 0u;
    out->texture_bytes = s->device >= 0 ? (uint64_t)s->n_texel_reals * sizeof(double) : 0u;
    out->texture_footprint_bytes = s->device >= 0 ? (uint64_t)s->tex_footprint_bytes : 0u;
    out->texture_layouts = s->device >= 0 ? s->tex_layouts : 0u;
    const bool up = s->device >= 0;
    out->render_blocks_per_cu = up ? (uint32_t)s->k64.blocks_per_cu[0] : 0u;
    out->render_blocks_wanted = up ? (uint32_t)s->blocks_wanted : 0u;
    out->lds_materials = up ? (uint32_t)s->k64.mat_lds : 0u;
    out->lds_light_nodes = up ? (uint32_t)s->k64.light_lds : 0u;
    out->lds_light_tris = up ? (uint32_t)s->k64.ltri_lds : 0u;
    out->stack_need = up ? (uint32_t)s->stack_need : 0u;
    out->render_variant = up ? render_variant(s, s->k64) | (s->f32_ready ? render_variant(s, s->k32) << 8 : 0u) : 0u;
    return PRT_OK;
}

int prt_scene_light_count(const PrtScene* s, uint64_t* n) {
    if (!s || !n) return fail(PRT_E_INVALID, "prt_scene_light_count: null argument");
    *n = s->lights.tris.size();
    return PRT_OK;
}

int prt_scene_light_order(const PrtScene* s, int32_t* prims, uint64_t cap) {
    if (!s || (!prims && cap)) return fail(PRT_E_INVALID, "prt_scene_light_order: null argument");
    if (cap < s->lights.tris.size()) return fail(PRT_E_INVALID, "prt_scene_light_order: buffer too small");
    for (size_t i = 0; i < s->lights.tris.size(); ++i) prims[i] = s->lights.tris[i].prim;
    return PRT_OK;
}

static int upload_impl(PrtScene* s, int device);

// The stack entries a traversal of a device-built tree can need: the nodes come back once for the count (at most 128 MB;
// larger trees keep the builders' bound).  Synchronous; host memory for the nodes may run out (std::bad_alloc).
static hipError_t device_tree_stack_need(const DNode* d_nodes, uint32_t n_nodes, int* need) {
    *need = PRT_STACK_DEPTH;
    if (n_nodes > (1u << 21)) return hipSuccess;
    std::vector<DNode> hn(n_nodes);
    const hipError_t e = hipMemcpy(hn.data(), d_nodes, hn.size() * sizeof(DNode), hipMemcpyDeviceToHost);
    if (e == hipSuccess) *need = prt::tree_stack_need(hn.data(), hn.size());
    return e;
}

// The corner table of a scene that answers distance queries (prt_scene_set_distance_queries), from the host triangles
// through the resident leaf order: allocated if the upload has none yet, filled on the null stream, synchronous.  The
// scene is uploaded and its device is current.
static int corners_from_host(PrtScene* s, const std::string& who) {
    const size_t n = s->tris.size();
    DevBuf<> table;
    if (!s->d_corners) PRT_HIP_AS(who, dev_alloc(table, std::max<size_t>(n * sizeof(DTriCorners), 256)));
    if (n) {
        std::vector<double> v;
        try {
            v.resize(n * 9);
        } catch (const std::bad_alloc&) {
            return fail(PRT_E_OOM, who + ": out of host memory for the corner table");
        }
        for (size_t i = 0; i < n; ++i) std::memcpy(v.data() + i * 9, s->tris[i].v, 9 * sizeof(double));
        DevBuf<> staged;
        PRT_HIP_AS(who, dev_alloc(staged, v.size() * sizeof(double)));
        PRT_HIP_AS(who, hipMemcpy(staged.get(), v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
        PRT_HIP_AS(who, s->after_refit(nullptr));
        prt::launch_gather_corners(static_cast<const double*>(staged.get()), s->d_order, (uint32_t)n,
                                   s->d_corners ? s->d_corners : static_cast<DTriCorners*>(table.get()), nullptr);
        PRT_HIP_AS(who, hipGetLastError());
        PRT_HIP_AS(who, hipDeviceSynchronize());
    }
    if (table) {
        s->d_corners = static_cast<DTriCorners*>(table.get());
        s->allocs.push_back(std::move(table));
    }
    return PRT_OK;
}

// The tables of a scene that answers signed distance queries (prt_scene_set_signed_queries): the weld, ids and adjacency
// lists of the host triangles (mesh_topology.cpp: a host pass), uploaded, and the pseudonormals from the resident corner
// table, on the null stream, synchronous.  The scene is uploaded, its device is current, it has its corner table and no
// signed tables.  All or nothing: a failure keeps none of them.
static int signed_from_host(PrtScene* s, const std::string& who) {
    const size_t n = s->tris.size();
    prt::MeshTopology topo;
    std::vector<uint32_t> slot;
    try {
        prt::build_topology(n ? &s->tris[0].v[0][0] : nullptr, sizeof(prt::HostTri) / sizeof(double), n, topo);
        const uint32_t ne = (uint32_t)topo.info.n_edges;
        slot.resize(n * 6);
        for (size_t t = 0; t < n; ++t)
            for (int k = 0; k < 3; ++k) {
                slot[t * 6 + k] = topo.eid[t * 3 + k]; // (kNoTopoId is the kernels' "no slot")
                slot[t * 6 + 3 + k] = ne + topo.vid[t * 3 + k];
            }
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, who + ": out of host memory for the mesh topology");
    }
    static_assert(sizeof(prt::HostTri) % sizeof(double) == 0, "HostTri is addressed in doubles");
    const size_t nv = topo.info.n_vertices, ne = topo.info.n_edges;
    const std::vector<uint32_t>* src[5] = {&slot, &topo.v_start, &topo.v_list, &topo.e_start, &topo.e_list};
    const size_t reals[2] = {n * 6, (nv + ne) * 3};
    DevBuf<> buf[7];
    size_t bytes = 0;
    for (int i = 0; i < 7; ++i) {
        const size_t b = i < 5 ? src[i]->size() * sizeof(uint32_t) : reals[i - 5] * sizeof(double);
        PRT_HIP_AS(who, dev_alloc(buf[i], std::max<size_t>(b, 256)));
        if (i < 5 && b) PRT_HIP_AS(who, hipMemcpy(buf[i].get(), src[i]->data(), b, hipMemcpyHostToDevice));
        if (i >= 5) PRT_HIP_AS(who, hipMemset(buf[i].get(), 0, std::max<size_t>(b, 256)));
        bytes += b;
    }
    prt::DSignedTables T;
    T.slot = static_cast<const uint32_t*>(buf[0].get());
    T.v_start = static_cast<const uint32_t*>(buf[1].get());
    T.v_list = static_cast<const uint32_t*>(buf[2].get());
    T.e_start = static_cast<const uint32_t*>(buf[3].get());
    T.e_list = static_cast<const uint32_t*>(buf[4].get());
    T.face = static_cast<double*>(buf[5].get());
    T.normal = static_cast<double*>(buf[6].get());
    T.n_tris = (uint32_t)n, T.n_vertices = (uint32_t)nv, T.n_edges = (uint32_t)ne;
    PRT_HIP_AS(who, s->after_refit(nullptr));
    prt::launch_pseudonormals(s->d_corners, T, nullptr);
    PRT_HIP_AS(who, hipGetLastError());
    PRT_HIP_AS(who, hipDeviceSynchronize());
    try {
        s->allocs.reserve(s->allocs.size() + 7);
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, who + ": out of host memory");
    }
    for (DevBuf<>& b : buf) s->allocs.push_back(std::move(b));
    s->sq = T;
    s->signed_bytes = bytes;
    return PRT_OK;
}

// The signed tables go (after the work that may still read or write them): switch-off.
static void signed_free(PrtScene* s) {
    const void* owned[7] = {s->sq.slot, s->sq.v_start, s->sq.v_list, s->sq.e_start, s->sq.e_list, s->sq.face, s->sq.normal};
    for (const void* p : owned) s->take(p).reset();
    s->sq = prt::DSignedTables();
    s->signed_bytes = 0;
}

// The moments table of a scene that answers winding-number queries (prt_scene_set_winding_queries), from the resident tree
// and corner table, on the null stream, synchronous.  The scene is uploaded, its device is current, it has its corner table
// and no moments table.  The refit's parent array and counters exist only after a first refit: this pass makes its own and
// frees them when it returns.  All or nothing.
static int winding_from_resident(PrtScene* s, const std::string& who) {
    const DScene& d = s->k64.d;
    const size_t nn = d.n_nodes;
    DevBuf<> table, parent, cnt;
    PRT_HIP_AS(who, dev_alloc(table, std::max<size_t>(nn * 4 * sizeof(prt::DWindingMoment), 256)));
    PRT_HIP_AS(who, dev_alloc(parent, std::max<size_t>(nn * sizeof(uint32_t), 256)));
    PRT_HIP_AS(who, dev_alloc(cnt, std::max<size_t>((nn * sizeof(uint32_t) + 15) & ~(size_t)15, 256)));
    PRT_HIP_AS(who, s->after_refit(nullptr));
    if (nn) prt::launch_refit_parents(d.nodes, d.n_nodes, static_cast<uint32_t*>(parent.get()), nullptr);
    PRT_HIP_AS(who, prt::launch_winding_moments(d.nodes, d.n_nodes, static_cast<const uint32_t*>(parent.get()), static_cast<uint32_t*>(cnt.get()),
                                                s->d_corners, d.n_tris, static_cast<prt::DWindingMoment*>(table.get()), nullptr));
    PRT_HIP_AS(who, hipGetLastError());
    PRT_HIP_AS(who, hipDeviceSynchronize());
    try {
        s->allocs.reserve(s->allocs.size() + 1);
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, who + ": out of host memory");
    }
    s->d_moments = static_cast<prt::DWindingMoment*>(table.get());
    s->allocs.push_back(std::move(table));
    return PRT_OK;
}

// Either the whole scene is resident afterwards, or nothing is: a failure anywhere (allocation, copy, device build)
// releases what was uploaded so far and leaves the scene in the not-uploaded state (device = -1), so that no later
// call can launch a kernel on a half-filled DScene.
int prt_scene_upload(PrtScene* s, int device) {
    if (!s) return fail(PRT_E_INVALID, "prt_scene_upload: null scene");
    if (s->host_stale)
        return fail(PRT_E_INVALID, "prt_scene_upload: the host geometry is stale (prt_scene_refit_device moved the resident geometry; "
                                   "pass every position to prt_scene_update_vertices or prt_scene_refit first)");
    const int rc = upload_impl(s, device);
    if (rc != PRT_OK) {
        KeepError keep;
        s->release();
    }
    return rc;
}

static int upload_impl(PrtScene* s, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PRT_E_NO_DEVICE, "prt_scene_upload: no HIP device");
    if (device < 0 || device >= ndev) return fail(PRT_E_INVALID, "prt_scene_upload: device index out of range");
    s->release();
    PRT_HIP(hipSetDevice(device));
    s->device = device;
    s->n_uploads = 0;
    s->fail_upload_at = dev_env("PRT_TEST_FAIL_UPLOAD") ? std::atoi(dev_env("PRT_TEST_FAIL_UPLOAD")) : -1;
    hipDeviceProp_t prop;
    PRT_HIP(hipGetDeviceProperties(&prop, device));
    s->n_cu = prop.multiProcessorCount;

    // triangles in BVH leaf order
    const size_t n = s->tris.size();
    std::vector<DTri> dt(n);
    std::vector<DTriShade> ds(n);
    for (size_t i = 0; i < n; ++i) {
        const prt::HostTri& T = s->tris[s->device_bvh ? i : s->bvh.order[i]]; // device build: permuted on the GPU below
        DTri& a = dt[i];
        std::memcpy(a.n, T.normal, 24);
        a.D = T.D;
        a.A[0] = T.e1[1] * T.w[2] - T.w[1] * T.e1[2]; // e1 x w
        a.A[1] = T.e1[2] * T.w[0] - T.w[2] * T.e1[0];
        a.A[2] = T.e1[0] * T.w[1] - T.w[0] * T.e1[1];
        a.B[0] = T.w[1] * T.e0[2] - T.e0[1] * T.w[2]; // w x e0
        a.B[1] = T.w[2] * T.e0[0] - T.e0[2] * T.w[0];
        a.B[2] = T.w[0] * T.e0[1] - T.e0[0] * T.w[1];
        a.a0 = T.v[0][0] * a.A[0] + T.v[0][1] * a.A[1] + T.v[0][2] * a.A[2];
        a.b0 = T.v[0][0] * a.B[0] + T.v[0][1] * a.B[1] + T.v[0][2] * a.B[2];
        DTriShade& b = ds[i];
        std::memset(&b, 0, sizeof(b));
        std::memcpy(b.tangent, T.tangent, 24);
        std::memcpy(b.uv0, T.uv[0], 16);
        std::memcpy(b.uv1, T.uv[1], 16);
        std::memcpy(b.uv2, T.uv[2], 16);
        b.material = T.material;
        b.prim = T.prim;
    }
    DScene& d = s->k64.d;
    int rc;
    // packed records for scenes the caches hold, one record per 128-byte line for scenes that stream from HBM
    uint32_t stride = (uint64_t)n * sizeof(DTri) > PRT_TRI_PADDED_ABOVE ? 128u : (uint32_t)sizeof(DTri);
    if (const char* e = dev_env("PRT_TUNE_TRI_STRIDE")) stride = std::atoi(e) == 128 ? 128u : (uint32_t)sizeof(DTri);
    if (sizeof(DTri) > 96) stride = (uint32_t)sizeof(DTri);
    d.tri_stride = stride;
    auto up_tris = [&](const DTri** out) -> int { // host records (packed) -> device records `stride` bytes apart
        if (stride == sizeof(DTri)) return s->up(dt, out);
        void* p = nullptr;
        if (int rc = s->alloc(n * (size_t)stride, &p)) return rc;
        if (n) {
            // the padded array is laid out on the host and goes up in one copy (a 2-D copy of millions of 96-byte rows
            // from pageable memory is served row by row)
            std::vector<char> padded;
            try {
                padded.assign(n * (size_t)stride, 0);
            } catch (const std::bad_alloc&) {
                return fail(PRT_E_OOM, "prt_scene_upload: out of host memory for the padded triangle records");
            }
            for (size_t i = 0; i < n; ++i) std::memcpy(padded.data() + i * (size_t)stride, &dt[i], sizeof(DTri));
            PRT_HIP(hipMemcpy(p, padded.data(), padded.size(), hipMemcpyHostToDevice));
        }
        *out = static_cast<const DTri*>(p);
        return PRT_OK;
    };
    const char* dump_path = s->device_bvh ? dev_env("PRT_TEST_DUMP_BVH") : nullptr; // (host trees are dumped where they are built)
    std::vector<DNode> dump_nodes;
    std::vector<uint32_t> dump_order;
    if (s->device_bvh) {
        std::vector<prt::PrimBox> pb;
        float box_origin[3];
        prt::prim_boxes(s->tris, pb, box_origin);
        prt::DeviceBVH db;
        std::string err;
        if (!prt::build_bvh_device(pb.data(), box_origin, n, db, &err)) return fail(PRT_E_HIP, "prt_scene_upload: " + err);
        s->allocs.emplace_back(db.d_nodes);
        s->allocs.emplace_back(db.d_order); // the leaf order: the gather below, and prt_scene_refit later
        if ((rc = check_node_count("prt_scene_upload", db.n_nodes))) return rc;
        if (dev_env("PRT_VALIDATE_BVH")) { // tests: check the device-built tree on the host before any ray visits it
            std::vector<DNode> hn(db.n_nodes);
            PRT_HIP(hipMemcpy(hn.data(), db.d_nodes, (size_t)db.n_nodes * sizeof(DNode), hipMemcpyDeviceToHost));
            if (!prt::validate_nodes(hn.data(), hn.size(), n, &err))
                return fail(PRT_E_LIMIT, "prt_scene_upload: device-built BVH is malformed: " + err);
        }
        if (dump_path) { // PRT_TEST_DUMP_BVH: nodes and leaf order come back here, the file is written once the stack need is known
            dump_nodes.resize(db.n_nodes);
            dump_order.resize(n);
            PRT_HIP_AS("prt_scene_upload: PRT_TEST_DUMP_BVH",
                       hipMemcpy(dump_nodes.data(), db.d_nodes, (size_t)db.n_nodes * sizeof(DNode), hipMemcpyDeviceToHost));
            PRT_HIP_AS("prt_scene_upload: PRT_TEST_DUMP_BVH", hipMemcpy(dump_order.data(), db.d_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        // records go up in description order (staging copies, freed at the end of this block) and are permuted into BVH
        // leaf order in HBM
        DevBuf<> t_in, s_in;
        void *t_out = nullptr, *s_out = nullptr;
        if ((rc = s->put(dt.data(), n * sizeof(DTri), t_in)) || (rc = s->put(ds.data(), n * sizeof(DTriShade), s_in)) ||
            (rc = s->alloc(n * (size_t)stride, &t_out)) || (rc = s->alloc(n * sizeof(DTriShade), &s_out)))
            return rc;
        prt::launch_gather_tris(static_cast<const DTri*>(t_in.get()), static_cast<const DTriShade*>(s_in.get()), db.d_order,
                                (uint32_t)n, t_out, stride, static_cast<DTriShade*>(s_out), nullptr);
        PRT_HIP_AS("prt_scene_upload", hipGetLastError());
        PRT_HIP_AS("prt_scene_upload", hipDeviceSynchronize());
        d.tris = static_cast<const DTri*>(t_out);
        d.shade = static_cast<const DTriShade*>(s_out);
        s->set_grid(db.grid_origin, db.grid_step, db.coord_scale);
        s->adopt_device_tree(db);
    } else {
        if ((rc = s->up(s->bvh.nodes, &d.nodes))) return rc;
        d.n_nodes = (uint32_t)s->bvh.nodes.size();
        if ((rc = up_tris(&d.tris))) return rc;
        if ((rc = s->up(ds, &d.shade))) return rc;
        if ((rc = s->up(s->bvh.order, &s->d_order, false))) return rc; // (for prt_scene_refit; not one of the counted table uploads)
        s->set_grid(s->bvh.grid_origin, s->bvh.grid_step, s->bvh.coord_scale); // (the host tree's own)
    }
    if ((rc = s->up(s->mats, &d.materials))) return rc;
    {
        // Device layout of the texels, per SCENE (DScene::tex_compact): BILINEAR FOOTPRINTS — per texel cell the four taps
        // Value() blends, 16 reals = one 128-byte line per lookup (bathroom2 -1.8 %) at 5.3x the bytes — while all the scene's
        // footprints fit PRT_TEX_FOOTPRINT_BUDGET (256 MiB of fp64 records = the size of the Infinity Cache; the fp32 fast mode
        // adds half as much again when it is used); else the plain row-major texel arrays (3 reals per texel, a lookup touches
        // two to four lines): a 4096^2 texture is 403 MB instead of 2.1 GB.  Same doubles, same blend, either way.
        std::vector<DTexture> qt(s->texs);
        std::vector<double> quads;
        size_t budget = PRT_TEX_FOOTPRINT_BUDGET;
        if (const char* e = dev_env("PRT_TUNE_TEX_BUDGET")) budget = (size_t)std::strtoull(e, nullptr, 10);
        size_t cells_all = 0;
        for (const DTexture& t : s->texs) cells_all += t.has_data ? (size_t)t.width * t.height : 0;
        const bool compact = cells_all * 16 * sizeof(double) > budget;
        const size_t per_cell = compact ? 3 : 16;
        try {
            quads.assign(cells_all * per_cell, 0.0);
        } catch (const std::bad_alloc&) {
            return fail(PRT_E_OOM, "prt_scene_upload: out of host memory for the texel arrays");
        }
        size_t at = 0;
        for (size_t i = 0; i < s->texs.size(); ++i) {
            const DTexture& t = s->texs[i];
            qt[i].offset = at;
            if (!t.has_data) continue;
            const double* px = s->texels_lin.data() + t.offset;
            if (compact) {
                const size_t n3 = (size_t)t.width * t.height * 3;
                std::memcpy(quads.data() + at, px, n3 * sizeof(double));
                at += n3;
                continue;
            }
            for (int y0 = 0; y0 < t.height; ++y0)
                for (int x0 = 0; x0 < t.width; ++x0) {
                    const int x1 = std::min(x0 + 1, t.width - 1), y1 = std::min(y0 + 1, t.height - 1); // Texture.cpp:35-36
                    double* o = quads.data() + at;
                    const int tap[4][2] = {{x0, y0}, {x1, y0}, {x0, y1}, {x1, y1}};
                    for (int k = 0; k < 4; ++k) std::memcpy(o + 3 * k, px + ((size_t)tap[k][1] * t.width + tap[k][0]) * 3, 24);
                    at += 16;
                }
        }
        d.tex_compact = compact ? 1u : 0u;
        s->tex_footprint_bytes = compact ? 0 : cells_all * 16 * sizeof(double);
        s->tex_layouts = cells_all == 0 ? 0u : (compact ? 2u : 1u);
        s->n_texel_reals = quads.size();
        if ((rc = s->up(qt, &d.textures))) return rc;
        if ((rc = s->up(quads, &d.texels_lin))) return rc;
    }
    if ((rc = s->up(s->lights.nodes, &d.light_nodes))) return rc;
    d.light_tab = nullptr;
    if (!s->lights.tab.empty() && (rc = s->up(s->lights.tab, &d.light_tab))) return rc;
    if ((rc = s->up(s->lights.tris, &d.light_tris))) return rc;
    s->light_res.nodes = const_cast<DLightNode*>(d.light_nodes);
    s->light_res.tris = const_cast<DLightTri*>(d.light_tris);
    s->light_res.tab = const_cast<uint32_t*>(d.light_tab);
    s->light_res.cap_nodes = s->lights.nodes.size();
    s->light_res.cap_tris = s->lights.tris.size();
    s->light_res.cap_tab = s->lights.tab.size();
    d.light_root = s->lights.root;
    d.n_lights = (int32_t)s->lights.tris.size();
    d.light_area = s->lights.area;
    d.n_tris = (uint32_t)n;
    for (PrtScene::CallSlot& q : s->slots) {
        PRT_HIP_AS("hipMalloc", dev_alloc(q.d_ctr, sizeof(DCounters)));
        PRT_HIP(hipMemset(q.d_ctr.get(), 0, sizeof(DCounters)));
        PRT_HIP(make_event(q.ev0, hipEventDefault));
        PRT_HIP(make_event(q.ev1, hipEventDefault));
        PRT_HIP(make_event(q.done, hipEventDisableTiming));
    }
    s->feat = 0;
    for (const DMaterial& m : s->mats) {
        if (m.texture >= 0) s->feat |= 1;
        if (m.type == PRT_MAT_PHONG) s->feat |= 2;
        if (m.type == PRT_MAT_COOKTORRANCE) s->feat |= 4;
    }
    if (const char* e = dev_env("PRT_TUNE_FEAT")) s->feat |= std::atoi(e); // developer: force a larger permutation
    s->feat = prt::render_permutation(s->feat);
    s->all_diffuse = prt::materials_all_diffuse(s->mats); // (the table just uploaded; nothing changes it afterwards)
    // Small read-only tables of the shading code live in LDS (LLDS kernels): every read of them is otherwise a
    // texture-addresser instruction, and the light tree's descent is a chain of dependent reads.  In order of
    // value per byte: the material table (must fit, <= 8 KB), all light triangles if there are at most 32, then
    // as many top levels of the light tree (breadth-first numbering) as the remaining budget holds.
    // Measured: materials cornell +2.5 %, bathroom2 +3 %, veach-mis +2 %; light tree veach-mis +5 %.
    // LDS traversal stacks of K3 are sized from what THIS tree can need (tree_stack_need), not from the builders' bound
    {
        int need = s->bvh.stack_need;
        if (s->bvh_info.built_on_device) // (the text is the one this failure has had since the copy stood here)
            PRT_HIP_AS("hipMemcpy(hn.data(), d.nodes, (size_t)d.n_nodes * sizeof(DNode), hipMemcpyDeviceToHost)",
                       device_tree_stack_need(d.nodes, d.n_nodes, &need));
        if (dump_path && (rc = dump_bvh(dump_path, s, dump_nodes.data(), dump_nodes.size(), dump_order.data(), need))) return rc;
        s->set_stack_need(need);
        s->d_nodes_shallow = nullptr;
        s->n_nodes_shallow = 0;
        // The fp64 render kernels keep STATIC stacks of PRT_STACK_DEPTH entries per lane (they are register-limited to three
        // blocks per CU; a run-time depth cost them 1.2 %), so a shallower collapse of the tree frees them no LDS: they
        // always traverse the full tree, and their table budget is what those static stacks leave.  (The fp32 kernels size
        // their stacks per launch and do take the 32-entry collapse of a deep host-built tree: ensure_f32.)
        if (dev_env("PRT_TUNE_VERBOSE")) std::fprintf(stderr, "[prt] tree needs %d stack entries\n", s->stack_need);
    }
    static_assert(sizeof(DLightNode) == 16 && sizeof(DLightTri) % 16 == 0, "LDS staging copies 16-byte pieces");
    // the fp64 kernels render without their LDS tables when the tables would cost a resident block (the fp32 ones do not)
    s->blocks_wanted = size_kernels(s, s->k64, true);
    if (s->distance_queries && (rc = corners_from_host(s, "prt_scene_upload"))) return rc;
    if (s->signed_queries && (rc = signed_from_host(s, "prt_scene_upload"))) return rc;
    if (s->winding_queries && (rc = winding_from_resident(s, "prt_scene_upload"))) return rc;
    return PRT_OK;
}

// The part of a scene description build_light_tree reads, from what the scene kept of it.
static void light_desc(const PrtScene* s, PrtSceneDesc& d) {
    std::memset(&d, 0, sizeof(d));
    d.n_tris = s->tris.size();
    d.n_meshes = (uint32_t)s->mesh_mat.size();
    d.mesh_first_tri = s->mesh_first.data();
    d.mesh_material = s->mesh_mat.data();
    static const int32_t none = 0;
    d.light_meshes = s->explicit_lights ? (s->light_meshes.empty() ? &none : s->light_meshes.data()) : nullptr;
    d.n_light_meshes = (uint32_t)s->light_meshes.size();
}

int prt_scene_update_vertices(PrtScene* s, const double* vertices, const double* normals) {
    if (!s || (!vertices && !s->tris.empty())) return fail(PRT_E_INVALID, "prt_scene_update_vertices: null argument");
    for (size_t i = 0; i < s->tris.size() * 9; ++i)
        if (!(std::fabs(vertices[i]) <= 1e18)) return fail(PRT_E_INVALID, "prt_scene_update_vertices: vertex coordinate is not finite (or beyond 1e18)");
    ++s->generation; // the geometry changes from here on, even if the update fails half way
    try {
        prt::update_triangles(vertices, normals, s->tris);
        s->host_stale = false; // every host position has been replaced
        PrtSceneDesc d;
        light_desc(s, d);
        s->lights = prt::LightTree();
        prt::build_light_tree(d, s->tris, s->mats, s->lights); // light areas and the CDF order follow the geometry
        if (s->device >= 0 && s->tris.size() >= 2) {
            // moving geometry: the tree is rebuilt on the GPU (milliseconds; no refit needed, no quality decay)
            s->device_bvh = true;
        } else if (!s->device_bvh) {
            std::string err;
            const auto t0 = std::chrono::steady_clock::now();
            if (!prt::build_bvh(s->tris, s->bvh, &err)) return fail(PRT_E_LIMIT, "prt_scene_update_vertices: " + err);
            s->bvh_info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            s->last.bvh_nodes = s->bvh_info.n_nodes = s->bvh.nodes.size();
            s->last.bvh_depth = s->bvh_info.depth = s->bvh.depth;
            if (const char* p = dev_env("PRT_TEST_DUMP_BVH")) {
                const int rc = dump_bvh(p, s, s->bvh.nodes.data(), s->bvh.nodes.size(), s->bvh.order.data(), s->bvh.stack_need);
                if (rc != PRT_OK) return rc;
            }
        }
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, "prt_scene_update_vertices: out of host memory");
    }
    if (s->device >= 0) return prt_scene_upload(s, s->device);
    return PRT_OK;
}

// fp32 fast mode: the float tables are derived from the resident fp64 ones the first time they are asked for
// (synchronous; the scene then holds both).  Triangle and shading records and texels are converted on the device —
// they already are in BVH leaf order there, whichever builder made the tree — the small tables on the host.
static int ensure_f32_impl(PrtScene* s);
// Stack entries per lane of the fp32 kernels for a tree that needs `need`.
static int f32_stack_depth(int need) {
    int depth = need <= PRT_STACK_SHALLOW ? PRT_STACK_SHALLOW : PRT_STACK_DEPTH;
    if (const char* e = dev_env("PRT_TUNE_STACK32")) depth = std::max(need, std::min(PRT_STACK_DEPTH, std::atoi(e))); // developer: smaller stacks when the tree allows
    return depth;
}
// The float copies of the light tree's nodes and of the light triangles (the small light tables are converted on the host).
static void light_tables_f32(const prt::LightTree& lights, std::vector<DLightNodeT<float>>& ln, std::vector<DLightTriT<float>>& lt) {
    ln.resize(lights.nodes.size());
    for (size_t i = 0; i < ln.size(); ++i) {
        std::memset(&ln[i], 0, sizeof(ln[i]));
        ln[i].left_area = (float)lights.nodes[i].left_area;
        ln[i].left = lights.nodes[i].left;
        ln[i].right = lights.nodes[i].right;
    }
    lt.resize(lights.tris.size());
    for (size_t i = 0; i < lt.size(); ++i) {
        const DLightTri& a = lights.tris[i];
        DLightTriT<float>& o = lt[i];
        std::memset(&o, 0, sizeof(o));
        conv_arr(o.v0, a.v0, 3); conv_arr(o.v1, a.v1, 3); conv_arr(o.v2, a.v2, 3); conv_arr(o.n, a.n, 3);
        o.area = (float)a.area; o.material = a.material; o.prim = a.prim; o.pdf = (float)a.pdf;
    }
}
// All or nothing, like the upload: a failure frees what this call allocated and leaves the scene without fp32 tables.
static int ensure_f32(PrtScene* s) {
    if (s->f32_ready) return PRT_OK;
    const size_t mark = s->allocs.size();
    const int rc = ensure_f32_impl(s);
    if (rc != PRT_OK) {
        KeepError keep;
        s->allocs.resize(mark);
        s->k32 = KernelConfig<float>();
        s->light_res.nodes32 = s->light_res.tris32 = nullptr;
        s->light_res.cap_nodes32 = s->light_res.cap_tris32 = 0;
    }
    return rc;
}
static int ensure_f32_impl(PrtScene* s) {
    const DScene& d = s->k64.d;
    KernelConfig<float>& k = s->k32;
    DSceneT<float>& f = k.d;
    const size_t n = d.n_tris;
    const uint32_t stride = d.tri_stride == sizeof(DTriT<double>) ? (uint32_t)sizeof(DTriT<float>) : PRT_TRI_PAD_STRIDE(float);
    void *t = nullptr, *sh = nullptr, *tx = nullptr;
    int rc;
    if ((rc = s->alloc(n * (size_t)stride, &t)) || (rc = s->alloc(n * sizeof(DTriShadeT<float>), &sh)) ||
        (rc = s->alloc(s->n_texel_reals * sizeof(float), &tx)))
        return rc;
    // the conversions read the records a refit on another (non-blocking) stream may still be writing
    PRT_HIP(s->after_refit(nullptr));
    prt32::launch_convert_tris(d.tris, d.tri_stride, (uint32_t)n, t, stride, nullptr);
    prt32::launch_convert_shade(d.shade, (uint32_t)n, static_cast<DTriShadeT<float>*>(sh), nullptr);
    prt32::launch_convert_reals(d.texels_lin, s->n_texel_reals, static_cast<float*>(tx), nullptr);
    PRT_HIP(hipGetLastError());
    std::vector<DMaterialT<float>> mats(s->mats.size());
    for (size_t i = 0; i < mats.size(); ++i) {
        const DMaterial& a = s->mats[i];
        DMaterialT<float>& o = mats[i];
        std::memset(&o, 0, sizeof(o));
        o.type = a.type; o.texture = a.texture;
        conv_arr(o.kd, a.kd, 3); conv_arr(o.ks, a.ks, 3); conv_arr(o.emission, a.emission, 3);
        conv_arr(o.eta, a.eta, 3); conv_arr(o.k, a.k, 3);
        o.ns = (float)a.ns; o.pkd = (float)a.pkd; o.pks = (float)a.pks;
        o.alpha_x = (float)a.alpha_x; o.alpha_y = (float)a.alpha_y;
        o.has_emission = a.has_emission; o.skip_light_sampling = a.skip_light_sampling;
        o.inv_ns1 = (float)a.inv_ns1; o.spec_scale = (float)a.spec_scale;
    }
    std::vector<DLightNodeT<float>> ln;
    std::vector<DLightTriT<float>> lt;
    light_tables_f32(s->lights, ln, lt);
    // (these uploads do not count for PRT_TEST_FAIL_UPLOAD, which injects failures into prt_scene_upload)
    if ((rc = s->up(mats, &f.materials, false)) || (rc = s->up(ln, &f.light_nodes, false)) || (rc = s->up(lt, &f.light_tris, false)))
        return rc;
    s->light_res.nodes32 = const_cast<DLightNodeT<float>*>(f.light_nodes);
    s->light_res.tris32 = const_cast<DLightTriT<float>*>(f.light_tris);
    s->light_res.cap_nodes32 = ln.size();
    s->light_res.cap_tris32 = lt.size();
    PRT_HIP(hipDeviceSynchronize());
    f.tris = static_cast<const DTriT<float>*>(t);
    f.shade = static_cast<const DTriShadeT<float>*>(sh);
    f.texels_lin = static_cast<const float*>(tx);
    f.tri_stride = stride;
    // The fp32 kernels have the registers for a fourth wave per SIMD; whether the LDS has room for a fourth block per CU
    // is decided by the traversal stacks: 32 entries per lane (32 KB per block) leave it, the builders' bound of
    // PRT_STACK_DEPTH does not.  Most trees need far fewer entries than that bound (tree_stack_need).
    {
        int need = s->stack_need; // of the tree the fp64 K3 traverses
        // the same binary tree collapsed for 32 entries: the fp32 kernels have the registers for a fourth block per CU,
        // which 32-entry stacks leave the LDS for
        if ((rc = s->shallow_resident())) return rc;
        if (s->d_nodes_shallow) need = std::min(need, PRT_STACK_SHALLOW);
        s->share_with_f32(); // (the collapse, where there is one, is the tree k32 traverses)
        k.stack_depth = f32_stack_depth(need);
        if (dev_env("PRT_TUNE_VERBOSE")) std::fprintf(stderr, "[prt] fp32 tables: tree needs %d stack entries, using %d\n", need, k.stack_depth);
    }
    size_kernels(s, k, false); // the fp32 kernels keep their LDS tables whatever they cost in occupancy
    s->f32_ready = true;
    return PRT_OK;
}

static int require_uploaded(PrtScene* s, const char* who) {
    if (!s) return fail(PRT_E_INVALID, std::string(who) + ": null scene");
    if (s->device < 0) return fail(PRT_E_NO_DEVICE, std::string(who) + ": scene is not uploaded to a HIP device (no CPU path exists)");
    PRT_HIP(hipSetDevice(s->device));
    return PRT_OK;
}

// ---- prt_scene_refit: new positions for a resident scene, the records and the tree's boxes follow on the GPU (bvh_refit.hip)
namespace {
float f32_round_down(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
    return f;
}
float f32_round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}
size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
} // namespace

// The refit state of the resident tree's topology, on `st`: the parents of every node, and the SAH cost that sah_ratio is
// measured against from now on.  The copy's status comes back; the launches report through hipGetLastError.
static hipError_t refit_baseline(PrtScene* s, hipStream_t st) {
    const PrtScene::Refit& R = s->refit;
    const DScene& d = s->k64.d;
    prt::launch_refit_parents(d.nodes, d.n_nodes, R.d_parent, st);
    prt::launch_refit_sah(d.nodes, d.n_nodes, d.grid_origin, d.grid_step, R.d_scratch, R.d_sah, st);
    return hipMemcpyAsync(R.d_sah + 1, R.d_sah, sizeof(double), hipMemcpyDeviceToDevice, st);
}

// What the first refit after an upload adds to the resident scene: its working arrays and events, the 32-entry collapse
// of a deep host-built tree (so that every resident node array is refitted from the first time on), the parents of
// every node, and the SAH cost of the tree as built.
static int refit_prepare(PrtScene* s, hipStream_t st) {
    PrtScene::Refit& R = s->refit;
    const DScene& d = s->k64.d;
    int rc;
    if (!R.d_check) {
        void *tbox, *parent, *cnt, *scratch, *check, *sah;
        if ((rc = s->alloc((size_t)d.n_tris * 6 * sizeof(float), &tbox)) || (rc = s->alloc((size_t)d.n_nodes * sizeof(uint32_t), &parent)) ||
            (rc = s->alloc(round16((size_t)d.n_nodes * sizeof(uint32_t)), &cnt)) || (rc = s->alloc(prt::refit_scratch_bytes(), &scratch)) ||
            (rc = s->alloc(2 * sizeof(double), &sah)) || (rc = s->alloc(sizeof(prt::RefitCheck), &check)))
            return rc;
        PRT_HIP(make_event(R.ev0, hipEventDefault));
        PRT_HIP(make_event(R.ev1, hipEventDefault));
        PRT_HIP(make_event(R.ev2, hipEventDefault));
        PRT_HIP(make_event(R.done, hipEventDisableTiming));
        if ((rc = s->shallow_resident())) return rc; // (ensure_f32 then finds it resident)
        R.d_tbox = static_cast<float*>(tbox);
        R.d_parent = static_cast<uint32_t*>(parent);
        R.d_cnt = static_cast<uint32_t*>(cnt);
        R.d_scratch = scratch;
        R.d_sah = static_cast<double*>(sah);
        // (the text is the one a failure of the copy has had since the copy stood here)
        PRT_HIP_AS("hipMemcpyAsync(R.d_sah + 1, R.d_sah, sizeof(double), hipMemcpyDeviceToDevice, st)", refit_baseline(s, st));
        PRT_HIP(hipGetLastError());
        R.d_check = static_cast<prt::RefitCheck*>(check);
    }
    if (s->d_nodes_shallow && !R.d_parent_sh) {
        void *parent, *cnt;
        if ((rc = s->alloc((size_t)s->n_nodes_shallow * sizeof(uint32_t), &parent)) ||
            (rc = s->alloc(round16((size_t)s->n_nodes_shallow * sizeof(uint32_t)), &cnt)))
            return rc;
        prt::launch_refit_parents(s->d_nodes_shallow, s->n_nodes_shallow, static_cast<uint32_t*>(parent), st);
        PRT_HIP(hipGetLastError());
        R.d_cnt_sh = static_cast<uint32_t*>(cnt);
        R.d_parent_sh = static_cast<uint32_t*>(parent);
    }
    return PRT_OK;
}

// The numbers of prim_boxes and quant_grid for a set of new positions, from the bounds of the first phase.
struct RefitGridHost {
    float origin[3], step[3], root_hi[3]; // the fp32 grid origin; the grid's steps and the root box's upper corner relative to it
    double origin_d[3], delta;            // the origin widened; prim_boxes' margin
    bool lights_moved = false;            // ... and whether light_stage has work (see refit_begin)
};

// What a refit and a rebuild share up to the decision.  after_refit, the working arrays (refit_prepare; a failure frees what
// this call made), then phase 1, read-only: vertex range, scene bounds, emitters in place; the one read-back; the grid.
// g.lights_moved: an emitter vertex differs and the scene accepts that (prt_scene_set_dynamic_lights): the gathered new
// vertices (and vertex normals, with d_normals) of the light triangles are in s->lu.h_gather.
static int refit_begin(PrtScene* s, const std::string& who, const double* d_verts, const double* d_normals, hipStream_t st,
                       RefitGridHost& g) {
    DScene& d = s->k64.d;
    const uint32_t n = d.n_tris;
    PrtScene::Refit& R = s->refit;
    if (!d_verts) return fail(PRT_E_INVALID, who + ": null vertices");
    PRT_HIP_AS(who, s->after_refit(st)); // one refit at a time: they share the working arrays
    {
        const size_t mark = s->allocs.size();
        const bool fresh = !R.d_check;
        const DNode* const shallow_before = s->d_nodes_shallow; // (ensure_f32 may have made it resident: k32 traverses it)
        const uint32_t n_shallow_before = s->n_nodes_shallow;
        const int rc = refit_prepare(s, st);
        if (rc != PRT_OK) { // (nothing resident has been written)
            KeepError keep;
            if (fresh) {
                (void)hipDeviceSynchronize();
                s->allocs.resize(mark);
                R = PrtScene::Refit();
                s->d_nodes_shallow = shallow_before; // only what this call uploaded went with `mark`
                s->n_nodes_shallow = n_shallow_before;
            }
            return rc;
        }
    }
    PrtScene::LightUpdate& U = s->lu;
    const size_t nl = (size_t)d.n_lights;
    const bool gather = s->dynamic_lights && nl > 0;
    if (gather && !U.d_gather) { // (72 bytes per light triangle for the vertices and as much for the normals, kept for the upload's life)
        PRT_HIP_AS(who, make_event(U.g0, hipEventDefault));
        PRT_HIP_AS(who, make_event(U.g1, hipEventDefault));
        PRT_HIP_AS(who, make_event(U.t0, hipEventDefault));
        PRT_HIP_AS(who, make_event(U.t1, hipEventDefault));
        void* p = nullptr;
        if (const int rc = s->alloc(nl * 18 * sizeof(double), &p)) return rc;
        U.d_gather = static_cast<double*>(p);
    }
    if (gather) {
        try {
            U.h_gather.resize(nl * 18);
        } catch (const std::bad_alloc&) {
            return fail(PRT_E_OOM, who + ": out of host memory");
        }
        PRT_HIP_AS(who, hipEventRecord(U.g0.get(), st));
    }
    prt::launch_refit_check(d_verts, n, d.light_tris, (uint32_t)d.n_lights, R.d_scratch, R.d_check, st, d_normals,
                            gather ? U.d_gather : nullptr, gather ? U.d_gather + nl * 9 : nullptr);
    PRT_HIP_AS(who, hipGetLastError());
    prt::RefitCheck c;
    PRT_HIP_AS(who, hipMemcpyAsync(&c, R.d_check, sizeof(c), hipMemcpyDeviceToHost, st));
    if (gather) { // the same read-back brings the emitters' new vertices: it scales with the emitter triangles, not the scene's
        PRT_HIP_AS(who, hipMemcpyAsync(U.h_gather.data(), U.d_gather, nl * (d_normals ? 18 : 9) * sizeof(double), hipMemcpyDeviceToHost, st));
        PRT_HIP_AS(who, hipEventRecord(U.g1.get(), st));
    }
    PRT_HIP_AS(who, hipEventRecord(R.done.get(), st)); // (the working arrays are in use until here, whatever the verdict)
    R.pending = true;
    PRT_HIP_AS(who, hipStreamSynchronize(st));
    if (c.flags & 1u) return fail(PRT_E_INVALID, who + ": vertex coordinate is not finite (or beyond 1e18)");
    if ((c.flags & 2u) && !s->dynamic_lights)
        return fail(PRT_E_INVALID, who + ": a vertex of a light mesh moved; emitters stay in place under a refit (the light tree is not "
                                         "rebuilt) - use prt_scene_update_vertices");
    g.lights_moved = (c.flags & 2u) != 0;
    // the quantisation grid of the new bounds: prim_boxes' origin and margin, quant_grid's steps.  The root box of the
    // builders is the union of the triangles' fp32 boxes; rounding and the subtraction are monotone, so its upper corner
    // is the box rule applied to the upper corner of the bounds.
    const double extent = std::max(1.0, std::max(c.hi[0] - c.lo[0], std::max(c.hi[1] - c.lo[1], c.hi[2] - c.lo[2])));
    g.delta = 1e-9 * extent + 256.0 * std::numeric_limits<double>::epsilon() * c.scale;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = f32_round_down(c.lo[a] - 2.0 * g.delta);
        g.origin_d[a] = (double)g.origin[a];
        g.root_hi[a] = f32_round_up((c.hi[a] + g.delta) - g.origin_d[a]);
    }
    const float zero[3] = {0.f, 0.f, 0.f};
    float rel0[3];
    prt::quant_grid(zero, g.root_hi, false, rel0, g.step);
    return PRT_OK;
}

// ---- a moved emitter (prt_scene_set_dynamic_lights): the light tree of the new positions, built into the spare arrays
// One array of the spare copy with room for `need` elements (a larger one replaces it: hipFree waits for the device).
static int light_grow(PrtScene* s, void*& p, size_t& cap, size_t need, size_t elem) {
    if (p && cap >= need) return PRT_OK;
    if (s->lu.n_allocs++ == s->lu.fail_alloc_at) return fail(PRT_E_OOM, "light update: injected allocation failure (PRT_TEST_FAIL_LIGHT_STAGE)");
    (void)s->take(p); // (freed here)
    p = nullptr;
    cap = 0;
    if (const int rc = s->alloc(need * elem, &p)) return rc;
    cap = need;
    return PRT_OK;
}

// Puts the emitter triangles' host records back (a refusal or a failure between light_stage and light_commit).
static void light_unstage(PrtScene* s) {
    PrtScene::LightUpdate& U = s->lu;
    if (!U.staged) return;
    for (size_t l = U.prims.size(); l-- > 0;) s->tris[(size_t)U.prims[l]] = U.saved[l];
    U.staged = false;
}

// Between the decision and the writing phase.  Host: the Triangle precompute of the emitter triangles from the gathered
// vertices, the reference's sort replay and flattening (build_light_tree), the plan of the tables.  Device, on `st`: the
// new nodes, records and table headers go into the SPARE arrays, light_tables.hip fills and verifies the tables there, and
// the flag comes back with the filled words (the call's second and last host synchronisation; none without tables).
// Nothing resident is written: a failure leaves the scene as it was.  On success the spare holds what a fresh scene of
// the new vertices has, and light_commit swaps it in.
static int light_stage(PrtScene* s, const std::string& who, bool normals, hipStream_t st) {
    PrtScene::LightUpdate& U = s->lu;
    const size_t nl = s->lights.tris.size();
    const auto t0 = std::chrono::steady_clock::now();
    bool tables = false;
    try {
        U.prims.resize(nl);
        U.saved.resize(nl);
        for (size_t l = 0; l < nl; ++l) {
            U.prims[l] = s->lights.tris[l].prim;
            U.saved[l] = s->tris[(size_t)U.prims[l]];
        }
        U.staged = true; // (from here on a failure puts the host records back)
        prt::update_triangles_listed(U.prims.data(), nl, U.h_gather.data(), normals ? U.h_gather.data() + nl * 9 : nullptr, s->tris);
        PrtSceneDesc ld;
        light_desc(s, ld);
        U.next = prt::LightTree();
        prt::build_light_tree(ld, s->tris, s->mats, U.next, false);
        tables = prt::plan_light_tables(U.next, U.plan);
        if (tables) U.words.assign(U.plan.tab.size(), 0u);
    } catch (const std::bad_alloc&) {
        light_unstage(s);
        return fail(PRT_E_OOM, who + ": out of host memory");
    }
    U.staged_host_tree_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    U.n_allocs = 0;
    U.fail_alloc_at = dev_env("PRT_TEST_FAIL_LIGHT_STAGE") ? std::atoi(dev_env("PRT_TEST_FAIL_LIGHT_STAGE")) : -1;
    {
        float ms = 0.f; // (the first phase has completed: the decision's read-back waited for it)
        U.staged_gather_ms = hipEventElapsedTime(&ms, U.g0.get(), U.g1.get()) == hipSuccess ? ms : 0.0;
    }
    auto failed = [&](int rc) {
        KeepError keep;
        light_unstage(s);
        return rc;
    };
    if (U.next.tris.size() != nl) return failed(fail(PRT_E_INVALID, who + ": the set of light triangles changed"));
    PrtScene::LightArrays& A = s->light_spare;
    const size_t n_full = U.next.full_nodes.size(), n_words = tables ? U.plan.tab.size() : 0, n_tab = tables ? U.plan.node.size() : 0;
    int rc;
    // (the node array has room for the full tree: what the scene descends if the verification fails)
    if ((rc = light_grow(s, A.nodes, A.cap_nodes, n_full, sizeof(DLightNode))) || (rc = light_grow(s, A.tris, A.cap_tris, nl, sizeof(DLightTri))) ||
        (n_words && (rc = light_grow(s, A.tab, A.cap_tab, n_words, sizeof(uint32_t)))))
        return failed(rc);
    if (s->f32_ready && ((rc = light_grow(s, A.nodes32, A.cap_nodes32, n_full, sizeof(DLightNodeT<float>))) ||
                         (rc = light_grow(s, A.tris32, A.cap_tris32, nl, sizeof(DLightTriT<float>)))))
        return failed(rc);
    const size_t off_full = 16, off_area = off_full + n_full * sizeof(DLightNode), off_node = off_area + n_tab * sizeof(double);
    auto hip = [&](hipError_t e) { return e == hipSuccess ? PRT_OK : failed(hip_fail(who, e)); };
    if ((rc = hip(U.tmp.reserve(off_node + n_tab * sizeof(int32_t), st)))) return rc;
    char* const tmp = U.tmp.get<char>();
    auto put = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
    const std::vector<DLightNode>& top = tables ? U.plan.top : U.next.full_nodes;
    if ((rc = hip(put(A.nodes, top.data(), top.size() * sizeof(DLightNode)))) || (rc = hip(put(A.tris, U.next.tris.data(), nl * sizeof(DLightTri)))))
        return rc;
    bool dropped = false;
    U.tables_timed = false;
    if (tables) {
        if ((rc = hip(put(tmp + off_full, U.next.full_nodes.data(), n_full * sizeof(DLightNode)))) ||
            (rc = hip(put(tmp + off_area, U.plan.area.data(), n_tab * sizeof(double)))) ||
            (rc = hip(put(tmp + off_node, U.plan.node.data(), n_tab * sizeof(int32_t)))) ||
            (rc = hip(put(A.tab, U.plan.tab.data(), n_words * sizeof(uint32_t)))))
            return rc;
        DLightTableBuild B;
        B.full = reinterpret_cast<const DLightNode*>(tmp + off_full);
        B.top = static_cast<const DLightNode*>(A.nodes);
        B.table_node = reinterpret_cast<const int32_t*>(tmp + off_node);
        B.table_area = reinterpret_cast<const double*>(tmp + off_area);
        B.tab = static_cast<uint32_t*>(A.tab);
        B.flag = reinterpret_cast<uint32_t*>(tmp);
        B.n_full = (uint32_t)n_full;
        B.n_top = (uint32_t)top.size();
        B.n_tables = (uint32_t)n_tab;
        B.n_words = (uint32_t)n_words;
        B.full_root = U.next.full_root;
        B.root = U.plan.root;
        B.total = (float)U.next.area;
        if ((rc = hip(hipEventRecord(U.t0.get(), st))) || (rc = hip(prt::launch_light_tables(B, st))) ||
            (rc = hip(hipMemcpyAsync(&U.flag, B.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st))) ||
            (rc = hip(hipMemcpyAsync(U.words.data(), A.tab, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st))) ||
            (rc = hip(hipEventRecord(U.t1.get(), st))) || (rc = hip(U.tmp.used(st))) || (rc = hip(hipStreamSynchronize(st))))
            return rc;
        U.tables_timed = true;
        // test hook (PRT_TEST_FAIL_LIGHT_VERIFY=1, dev-hooks build): the device verification reports a failure
        dropped = U.flag != 0 || (dev_env("PRT_TEST_FAIL_LIGHT_VERIFY") && std::atoi(dev_env("PRT_TEST_FAIL_LIGHT_VERIFY")));
        if (dropped) { // the scene keeps the full tree and no tables, as the host builder decides
            if ((rc = hip(put(A.nodes, U.next.full_nodes.data(), n_full * sizeof(DLightNode))))) return rc;
        } else {
            try {
                prt::apply_light_tables(U.next, U.plan, U.words);
            } catch (const std::bad_alloc&) {
                return failed(fail(PRT_E_OOM, who + ": out of host memory"));
            }
        }
    }
    if (s->f32_ready) {
        try {
            light_tables_f32(U.next, U.ln32, U.lt32);
        } catch (const std::bad_alloc&) {
            return failed(fail(PRT_E_OOM, who + ": out of host memory"));
        }
        if ((rc = hip(put(A.nodes32, U.ln32.data(), U.ln32.size() * sizeof(DLightNodeT<float>)))) ||
            (rc = hip(put(A.tris32, U.lt32.data(), U.lt32.size() * sizeof(DLightTriT<float>)))))
            return rc;
    }
    // did the layout change?  (array sizes, the root, or any table's place: then the kernels are sized again)
    const prt::LightTree& old = s->lights;
    bool relaid = old.nodes.size() != U.next.nodes.size() || old.tab.size() != U.next.tab.size() || old.root != U.next.root ||
                  old.n_tables != U.next.n_tables;
    for (size_t t = 0; !relaid && t < U.next.n_tables; ++t)
        relaid = std::memcmp(old.tab.data() + 8 * t, U.next.tab.data() + 8 * t, 5 * sizeof(uint32_t)) != 0; // first, n, thr_off, bkt_off, n_bkt
    U.staged_relaid = relaid;
    U.staged_dropped = dropped;
    U.staged_tables = tables;
    return PRT_OK;
}

// In the writing phase (the readers in flight have been waited for on the call's stream, the grid is committed): the
// spare copy becomes the resident one, on the device by exchanging pointers and on the host by taking the new tree.
static void light_commit(PrtScene* s) {
    PrtScene::LightUpdate& U = s->lu;
    if (!U.staged) return;
    U.staged = false;
    std::swap(s->light_res, s->light_spare);
    const PrtScene::LightArrays& A = s->light_res;
    s->lights = std::move(U.next);
    U.next = prt::LightTree();
    DScene& d = s->k64.d;
    d.light_nodes = static_cast<const DLightNode*>(A.nodes);
    d.light_tris = static_cast<const DLightTri*>(A.tris);
    d.light_tab = s->lights.tab.empty() ? nullptr : static_cast<const uint32_t*>(A.tab);
    d.light_root = s->lights.root;
    d.n_lights = (int32_t)s->lights.tris.size();
    d.light_area = s->lights.area;
    if (s->f32_ready) {
        DSceneT<float>& f = s->k32.d;
        f.light_nodes = static_cast<const DLightNodeT<float>*>(A.nodes32);
        f.light_tris = static_cast<const DLightTriT<float>*>(A.tris32);
        s->share_with_f32();
    }
    ++U.count;
    U.host_tree_ms = U.staged_host_tree_ms;
    U.gather_ms = U.staged_gather_ms;
    U.relaid = U.staged_relaid ? 1u : 0u;
    U.tables_dropped = U.staged_dropped ? 1u : 0u;
    if (U.staged_relaid) size_kernels_again(s); // LDS sizing and render_variant may change (PRT_VARIANT_EXTRA depends on the tables' presence)
}

// From the decision to the writing phase: moved emitters are staged (the last thing that can refuse); the writing phase
// changes what calls in flight read, so `st` waits for both call slots and the last features call first; then the swap.
static int lights_then_readers(PrtScene* s, const std::string& who, bool lights_moved, bool normals, hipStream_t st) {
    if (lights_moved)
        if (const int rc = light_stage(s, who, normals, st)) return rc;
    hipError_t e = hipSuccess;
    for (PrtScene::CallSlot& q : s->slots)
        if (q.timed && e == hipSuccess) e = hipStreamWaitEvent(st, q.done.get(), 0);
    if (s->feat_pending && e == hipSuccess) e = hipStreamWaitEvent(st, s->feat_done.get(), 0);
    if (e != hipSuccess) {
        light_unstage(s);
        return hip_fail(who, e);
    }
    light_commit(s);
    return PRT_OK;
}

// The geometry changes from here on, even if a launch afterwards fails half way (as in prt_scene_update_vertices): the
// generation and the grid, in every copy (the host tree's, both DScenes), go first, so that a scene whose records were
// partly rewritten never passes for the old one.
static void refit_commit_grid(PrtScene* s, const float origin[3], const float step[3], float coord_scale) {
    s->set_grid(origin, step, coord_scale);
    ++s->generation;
}

// PRT_TEST_DUMP_BVH: the resident tree (refitted or rebuilt), as the kernels now get it (synchronous)
static int dump_resident_bvh(PrtScene* s, const std::string& who, hipStream_t st) {
    const char* path = dev_env("PRT_TEST_DUMP_BVH");
    if (!path) return PRT_OK;
    const DScene& d = s->k64.d;
    std::vector<DNode> hn(d.n_nodes);
    std::vector<uint32_t> ho(d.n_tris);
    PRT_HIP_AS(who, hipStreamSynchronize(st));
    PRT_HIP_AS(who, hipMemcpy(hn.data(), d.nodes, hn.size() * sizeof(DNode), hipMemcpyDeviceToHost));
    PRT_HIP_AS(who, hipMemcpy(ho.data(), s->d_order, ho.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return dump_bvh(path, s, hn.data(), hn.size(), ho.data(), s->stack_need);
}

// Everything resident that follows new positions, on `st`: the fp64 records and the triangles' boxes (R.d_tbox), then what
// is derived from them.  A resident table that follows the geometry is added HERE, for the refit and the rebuild alike.
static void launch_position_followers(PrtScene* s, const double* d_verts, const double* d_normals, const RefitGridHost& g, hipStream_t st) {
    const DScene& d = s->k64.d;
    const uint32_t n = d.n_tris;
    prt::launch_refit_tris(d_verts, d_normals, s->d_order, n, const_cast<DTri*>(d.tris), d.tri_stride, const_cast<DTriShade*>(d.shade),
                           s->refit.d_tbox, g.origin_d, g.delta, st);
    if (s->d_corners) prt::launch_gather_corners(d_verts, s->d_order, n, s->d_corners, st); // distance queries: the corners follow
    if (s->d_corners && s->sq.slot) prt::launch_pseudonormals(s->d_corners, s->sq, st);      // signed queries: the pseudonormals too
    if (s->f32_ready) { // the float records follow the fp64 ones (same leaf order)
        const DSceneT<float>& f = s->k32.d;
        prt32::launch_convert_tris(d.tris, d.tri_stride, n, const_cast<DTriT<float>*>(f.tris), f.tri_stride, st);
        prt32::launch_convert_shade(d.shade, n, const_cast<DTriShadeT<float>*>(f.shade), st);
    }
}

// What follows the TREE as well as the positions, on `st` behind the corner gather, the boxes and the parents of the resident
// topology: the moments of the winding-number queries, with the refit's parent array and counters.  For the refit and the
// rebuild alike.
static hipError_t launch_tree_followers(PrtScene* s, hipStream_t st) {
    const DScene& d = s->k64.d;
    if (!s->d_moments || !s->d_corners) return hipSuccess;
    return prt::launch_winding_moments(d.nodes, d.n_nodes, s->refit.d_parent, s->refit.d_cnt, s->d_corners, d.n_tris, s->d_moments, st);
}

// d_verts / d_normals: device arrays [n_tris][3][xyz].  The scene is uploaded and its device is current.
static int refit_impl(PrtScene* s, const std::string& who, const double* d_verts, const double* d_normals, hipStream_t st) {
    DScene& d = s->k64.d;
    const uint32_t n = d.n_tris;
    if (n == 0) return PRT_OK; // nothing to move (the empty scene's root is never traversed)
    PrtScene::Refit& R = s->refit;
    RefitGridHost g;
    if (const int rc = refit_begin(s, who, d_verts, d_normals, st, g)) return rc;
    const float *origin = g.origin, *step = g.step;
    if (const int rc = lights_then_readers(s, who, g.lights_moved, d_normals != nullptr, st)) return rc;
    {
        float cs = std::max(g.root_hi[0], std::max(g.root_hi[1], g.root_hi[2]));
        if (s->bvh_info.built_on_device) // (the device builder also covers the grid's far corner)
            for (int a = 0; a < 3; ++a) cs = std::max(cs, (float)(65535.0 * (double)step[a]));
        refit_commit_grid(s, origin, step, std::nextafter(cs, std::numeric_limits<float>::infinity()));
    }
    PRT_HIP_AS(who, hipEventRecord(R.ev0.get(), st));
    launch_position_followers(s, d_verts, d_normals, g, st);
    PRT_HIP_AS(who, hipGetLastError());
    PRT_HIP_AS(who, hipEventRecord(R.ev1.get(), st)); // (records_ms includes the fp32 re-derivation)
    PRT_HIP_AS(who, prt::launch_refit_boxes(const_cast<DNode*>(d.nodes), d.n_nodes, R.d_parent, R.d_cnt, R.d_tbox, n, step, st));
    if (s->d_nodes_shallow)
        PRT_HIP_AS(who, prt::launch_refit_boxes(const_cast<DNode*>(s->d_nodes_shallow), s->n_nodes_shallow, R.d_parent_sh, R.d_cnt_sh,
                                                R.d_tbox, n, step, st));
    PRT_HIP_AS(who, launch_tree_followers(s, st)); // (boxes_ms includes them)
    prt::launch_refit_sah(d.nodes, d.n_nodes, origin, step, R.d_scratch, R.d_sah + 1, st);
    PRT_HIP_AS(who, hipGetLastError());
    PRT_HIP_AS(who, hipEventRecord(R.ev2.get(), st));
    PRT_HIP_AS(who, hipEventRecord(R.done.get(), st));
    ++R.count;
    return dump_resident_bvh(s, who, st);
}

// ---- prt_scene_rebuild: new positions for a resident scene and a NEW tree of them from the device builder; textures,
// materials and light tables stay resident (kernels in bvh_refit.hip, the builder in bvh_build_gpu.hip)
static int rebuild_impl(PrtScene* s, const std::string& who, const double* d_verts, const double* d_normals, hipStream_t st) {
    DScene& d = s->k64.d;
    const uint32_t n = d.n_tris;
    if (n < 2) return refit_impl(s, who, d_verts, d_normals, st); // the builder needs two triangles: one triangle's tree has one shape
    PrtScene::Refit& R = s->refit;
    RefitGridHost g;
    if (const int rc = refit_begin(s, who, d_verts, d_normals, st, g)) return rc;
    // Everything the new tree needs is made before anything resident is written: a failure up to the commit below frees
    // what this call made (the owners are locals) and leaves the scene as it was.
    // test hook (PRT_TEST_FAIL_REBUILD=k): the k-th allocation of the rebuild, the builder run counting as one, reports out-of-memory
    const int fail_at = dev_env("PRT_TEST_FAIL_REBUILD") ? std::atoi(dev_env("PRT_TEST_FAIL_REBUILD")) : -1;
    int n_allocs = 0;
    auto injected = [&]() { return n_allocs++ == fail_at; };
    auto alloc = [&](size_t bytes, DevBuf<>& out) -> int {
        if (injected()) return fail(PRT_E_OOM, who + ": injected allocation failure (PRT_TEST_FAIL_REBUILD)");
        PRT_HIP_AS(who, dev_alloc(out, std::max<size_t>(bytes, 256)));
        return PRT_OK;
    };
    DevBuf<> boxes, nodes, order, shade, inv, parent, cnt, moments;
    int rc;
    if ((rc = alloc((size_t)n * sizeof(prt::PrimBox), boxes))) return rc;
    prt::launch_prim_boxes(d_verts, n, static_cast<float*>(boxes.get()), g.origin_d, g.delta, st);
    PRT_HIP_AS(who, hipGetLastError());
    prt::DeviceBVH db;
    {
        if (injected()) return fail(PRT_E_OOM, who + ": injected allocation failure (PRT_TEST_FAIL_REBUILD)");
        std::string err;
        if (!prt::build_bvh_device_boxes(static_cast<const prt::PrimBox*>(boxes.get()), g.origin, n, db, &err, st))
            return fail(PRT_E_HIP, who + ": " + err);
        nodes.reset(db.d_nodes);
        order.reset(db.d_order);
    }
    if ((rc = check_node_count(who, db.n_nodes))) return rc;
    if ((rc = alloc((size_t)n * sizeof(DTriShade), shade)) || (rc = alloc((size_t)n * sizeof(uint32_t), inv)) ||
        (rc = alloc((size_t)db.n_nodes * sizeof(uint32_t), parent)) || (rc = alloc(round16((size_t)db.n_nodes * sizeof(uint32_t)), cnt)))
        return rc;
    if (s->d_moments && (rc = alloc((size_t)db.n_nodes * 4 * sizeof(prt::DWindingMoment), moments))) return rc; // winding queries: the new tree's table
    int need = PRT_STACK_DEPTH; // as at upload
    try {
        PRT_HIP_AS(who, device_tree_stack_need(db.d_nodes, db.n_nodes, &need));
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, who + ": out of host memory");
    }
    if ((rc = lights_then_readers(s, who, g.lights_moved, d_normals != nullptr, st))) return rc; // (before the kernels are sized below)

    // Commit.  From here on the refit's wording applies: the generation and the grid are the new ones.  The scene takes
    // the new arrays at once; the ones they replace stay alive in `old` until this call returns (freeing waits for the device).
    refit_commit_grid(s, db.grid_origin, db.grid_step, db.coord_scale);
    const DTriShade* const shade_old = d.shade;
    const uint32_t* const order_old = s->d_order;
    DevBuf<> old[9] = {s->take(d.nodes),  s->take(s->d_order),        s->take(d.shade),      s->take(R.d_parent),
                       s->take(R.d_cnt),  s->take(s->d_nodes_shallow), s->take(R.d_parent_sh), s->take(R.d_cnt_sh),
                       s->take(moments ? s->d_moments : nullptr)};
    s->adopt_device_tree(db); // (nodes and order)
    d.shade = static_cast<const DTriShade*>(shade.get());
    R.d_parent = static_cast<uint32_t*>(parent.get());
    R.d_cnt = static_cast<uint32_t*>(cnt.get());
    R.d_parent_sh = R.d_cnt_sh = nullptr; // a device-built tree has no 32-entry collapse
    s->d_nodes_shallow = nullptr;
    s->n_nodes_shallow = 0;
    if (moments) s->d_moments = static_cast<prt::DWindingMoment*>(moments.get());
    for (DevBuf<>* b : {&nodes, &order, &shade, &parent, &cnt, &moments})
        if (*b) s->allocs.push_back(std::move(*b)); // (room for more than `old` took out)
    s->device_bvh = true; // a later upload builds on the device as well: the host tree is not this one
    s->set_stack_need(need);
    if (s->f32_ready) {
        s->share_with_f32(); // (the new nodes: no collapse is left)
        s->k32.stack_depth = f32_stack_depth(s->stack_need);
    }
    size_kernels_again(s);
    // (a rebuild is no refit: none of the refit's timing events is recorded, and refit.count stays)
    prt::launch_permute_shade(shade_old, order_old, s->d_order, n, static_cast<uint32_t*>(inv.get()), const_cast<DTriShade*>(d.shade), st);
    launch_position_followers(s, d_verts, d_normals, g, st);
    // the refit state of the new topology
    PRT_HIP_AS(who, refit_baseline(s, st));
    PRT_HIP_AS(who, launch_tree_followers(s, st));
    PRT_HIP_AS(who, hipGetLastError());
    PRT_HIP_AS(who, hipEventRecord(R.done.get(), st));
    PRT_HIP_AS(who, hipStreamSynchronize(st)); // synchronous: the new tree is resident, what it replaced can go
    return dump_resident_bvh(s, who, st);
}

// The host-pointer forms of the refit and the rebuild: the caller's arrays go to the device, the host triangles follow.
static int host_positions(PrtScene* s, const char* name, const double* vertices, const double* normals, bool rebuild) {
    const std::string who = name;
    int rc = require_uploaded(s, name);
    if (rc) return rc;
    const size_t n = s->tris.size(), bytes = n * 9 * sizeof(double);
    if (n == 0) return PRT_OK;
    if (!vertices) return fail(PRT_E_INVALID, who + ": null vertices");
    // device copies of the caller's arrays, in a buffer the scene keeps (a previous refit may still be reading it)
    PRT_HIP_AS(who, s->refit_in.reserve(bytes * (normals ? 2 : 1), nullptr));
    double* dv = s->refit_in.get<double>();
    double* dn = normals ? dv + n * 9 : nullptr;
    PRT_HIP(hipMemcpyAsync(dv, vertices, bytes, hipMemcpyHostToDevice, nullptr));
    if (normals) PRT_HIP(hipMemcpyAsync(dn, normals, bytes, hipMemcpyHostToDevice, nullptr));
    rc = (rebuild ? rebuild_impl : refit_impl)(s, who, dv, dn, nullptr);
    PRT_HIP_AS(who, s->refit_in.used(nullptr));
    if (rc != PRT_OK) {
        KeepError keep;
        (void)hipStreamSynchronize(nullptr); // the caller's arrays are free again on every way out
        return rc;
    }
    // the host triangles follow, so that a later upload or update sees this geometry; the host tree does not (the boxes
    // were refitted, or the tree rebuilt, on the device only): that upload builds a fresh tree, on the GPU where there are
    // two triangles to split
    try {
        prt::update_triangles(vertices, normals, s->tris);
        s->host_stale = false;
        if (!s->device_bvh) {
            if (n >= 2) s->device_bvh = true;
            else {
                std::string err;
                if (!prt::build_bvh(s->tris, s->bvh, &err)) return fail(PRT_E_LIMIT, who + ": " + err);
            }
        }
    } catch (const std::bad_alloc&) {
        s->host_stale = true; // the device holds the new geometry, the host triangles may not
        return fail(PRT_E_OOM, who + ": out of host memory (the resident scene holds the new geometry)");
    }
    return PRT_OK;
}

int prt_scene_refit(PrtScene* s, const double* vertices, const double* normals) {
    return host_positions(s, "prt_scene_refit", vertices, normals, false);
}

int prt_scene_rebuild(PrtScene* s, const double* vertices, const double* normals) {
    return host_positions(s, "prt_scene_rebuild", vertices, normals, true);
}

// The device-pointer forms: the caller's device arrays as they are, on the caller's stream.
static int device_positions(PrtScene* s, const char* name, const void* d_vertices, const void* d_normals, void* stream, bool rebuild) {
    int rc = require_uploaded(s, name);
    if (rc) return rc;
    rc = (rebuild ? rebuild_impl : refit_impl)(s, name, static_cast<const double*>(d_vertices), static_cast<const double*>(d_normals),
                                               reinterpret_cast<hipStream_t>(stream));
    if (rc == PRT_OK && !s->tris.empty()) s->host_stale = true; // the host triangles still hold the old positions
    return rc;
}

int prt_scene_refit_device(PrtScene* s, const void* d_vertices, const void* d_normals, void* stream) {
    return device_positions(s, "prt_scene_refit_device", d_vertices, d_normals, stream, false);
}

int prt_scene_rebuild_device(PrtScene* s, const void* d_vertices, const void* d_normals, void* stream) {
    return device_positions(s, "prt_scene_rebuild_device", d_vertices, d_normals, stream, true);
}

int prt_scene_refit_info(const PrtScene* s, PrtRefitInfo* out) {
    if (!s || !out) return fail(PRT_E_INVALID, "prt_scene_refit_info: null argument");
    std::memset(out, 0, sizeof(*out));
    const PrtScene::Refit& R = s->refit;
    out->refits = R.count;
    out->sah_ratio = 1.0;
    out->host_stale = s->host_stale ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        out->grid_origin[a] = s->bvh.grid_origin[a];
        out->grid_step[a] = s->bvh.grid_step[a];
    }
    out->slab_scale = s->device >= 0 ? s->k64.d.slab_scale : 0.f;
    if (s->device >= 0 && R.count) {
        PRT_HIP(hipSetDevice(s->device));
        PRT_HIP(hipEventSynchronize(R.ev2.get()));
        float ms = 0.f;
        PRT_HIP(hipEventElapsedTime(&ms, R.ev0.get(), R.ev1.get()));
        out->records_ms = ms;
        PRT_HIP(hipEventElapsedTime(&ms, R.ev1.get(), R.ev2.get()));
        out->boxes_ms = ms;
        double sah[2] = {0, 0};
        PRT_HIP(hipMemcpy(sah, R.d_sah, sizeof(sah), hipMemcpyDeviceToHost));
        out->sah_ratio = sah[0] > 0.0 ? sah[1] / sah[0] : 1.0;
    }
    return PRT_OK;
}

int prt_scene_set_dynamic_lights(PrtScene* s, int on) {
    if (!s) return fail(PRT_E_INVALID, "prt_scene_set_dynamic_lights: null scene");
    s->dynamic_lights = on != 0;
    return PRT_OK;
}

int prt_scene_get_dynamic_lights(const PrtScene* s, int* on) {
    if (!s || !on) return fail(PRT_E_INVALID, "prt_scene_get_dynamic_lights: null argument");
    *on = s->dynamic_lights ? 1 : 0;
    return PRT_OK;
}

// Before a query switch (`what`: its name in the text) changes the tables of an uploaded scene.  On: they are made from the
// host triangles, which must be current.  Off: the queries in flight, and a refit that may still be writing the tables, end.
static int query_switch_ready(PrtScene* s, const char* who, bool want, const char* what) {
    PRT_HIP(hipSetDevice(s->device));
    if (want) {
        if (s->host_stale)
            return fail(PRT_E_INVALID, std::string(who) + ": the host geometry is stale (prt_scene_refit_device / prt_scene_rebuild_device moved the "
                                                          "resident geometry past it): switch " + what + " on before moving geometry, or call "
                                                          "prt_scene_refit or prt_scene_update_vertices first");
        return PRT_OK;
    }
    for (PrtScene::CallSlot& q : s->slots)
        if (q.timed) PRT_HIP_AS(who, hipEventSynchronize(q.done.get()));
    if (s->refit.pending) PRT_HIP_AS(who, hipEventSynchronize(s->refit.done.get()));
    return PRT_OK;
}

int prt_scene_set_distance_queries(PrtScene* s, int on) {
    const char* who = "prt_scene_set_distance_queries";
    if (!s) return fail(PRT_E_INVALID, std::string(who) + ": null scene");
    const bool want = on != 0;
    if (want == s->distance_queries) return PRT_OK;
    if (!want && s->signed_queries)
        return fail(PRT_E_INVALID, std::string(who) + ": signed distance queries are on and need the corner table "
                                                      "(call prt_scene_set_signed_queries(scene, 0) first)");
    if (!want && s->winding_queries)
        return fail(PRT_E_INVALID, std::string(who) + ": winding-number queries are on and need the corner table "
                                                      "(call prt_scene_set_winding_queries(scene, 0) first)");
    if (s->device < 0) { // not uploaded: the next upload makes the table
        s->distance_queries = want;
        return PRT_OK;
    }
    if (const int rc = query_switch_ready(s, who, want, "distance queries")) return rc;
    if (want) {
        if (const int rc = corners_from_host(s, who)) return rc; // (nothing is kept on a failure: the switch stays off)
        s->distance_queries = true;
        return PRT_OK;
    }
    s->take(s->d_corners).reset();
    s->d_corners = nullptr;
    s->distance_queries = false;
    return PRT_OK;
}

int prt_scene_get_distance_queries(const PrtScene* s, int* on) {
    if (!s || !on) return fail(PRT_E_INVALID, "prt_scene_get_distance_queries: null argument");
    *on = s->distance_queries ? 1 : 0;
    return PRT_OK;
}

// A switch whose tables need the corner table goes on for an uploaded scene: the corners first, where distance queries
// are off, then `make` (signed_from_host, winding_from_resident); a failure leaves the corner table as it was.
static int tables_beside_corners(PrtScene* s, const char* who, int (*make)(PrtScene*, const std::string&)) {
    const bool had_corners = s->distance_queries;
    if (!had_corners)
        if (const int rc = corners_from_host(s, who)) return rc;
    if (const int rc = make(s, who)) {
        if (!had_corners) { // both switches as they were
            s->take(s->d_corners).reset();
            s->d_corners = nullptr;
        }
        return rc;
    }
    s->distance_queries = true;
    return PRT_OK;
}

int prt_scene_set_signed_queries(PrtScene* s, int on) {
    const char* who = "prt_scene_set_signed_queries";
    if (!s) return fail(PRT_E_INVALID, std::string(who) + ": null scene");
    const bool want = on != 0;
    if (want == s->signed_queries) return PRT_OK;
    if (s->device < 0) { // not uploaded: the next upload makes the tables
        s->signed_queries = want;
        if (want) s->distance_queries = true;
        return PRT_OK;
    }
    if (const int rc = query_switch_ready(s, who, want, "signed queries")) return rc;
    if (want) {
        if (const int rc = tables_beside_corners(s, who, signed_from_host)) return rc;
        s->signed_queries = true;
        return PRT_OK;
    }
    signed_free(s);
    s->signed_queries = false;
    return PRT_OK;
}

int prt_scene_set_winding_queries(PrtScene* s, int on) {
    const char* who = "prt_scene_set_winding_queries";
    if (!s) return fail(PRT_E_INVALID, std::string(who) + ": null scene");
    const bool want = on != 0;
    if (want == s->winding_queries) return PRT_OK;
    if (s->device < 0) { // not uploaded: the next upload makes the table
        s->winding_queries = want;
        if (want) s->distance_queries = true;
        return PRT_OK;
    }
    if (const int rc = query_switch_ready(s, who, want, "winding queries")) return rc;
    if (want) {
        if (const int rc = tables_beside_corners(s, who, winding_from_resident)) return rc;
        s->winding_queries = true;
        return PRT_OK;
    }
    s->take(s->d_moments).reset(); // (distance queries stay on)
    s->d_moments = nullptr;
    s->winding_queries = false;
    return PRT_OK;
}

int prt_scene_get_winding_queries(const PrtScene* s, int* on) {
    if (!s || !on) return fail(PRT_E_INVALID, "prt_scene_get_winding_queries: null argument");
    *on = s->winding_queries ? 1 : 0;
    return PRT_OK;
}

int prt_scene_winding_moments(PrtScene* s, double* out, uint64_t cap_nodes, uint64_t* n) {
    static_assert(sizeof(prt::DWindingMoment) == 8 * sizeof(double), "the hook copies the records as they are");
    const char* who = "prt_scene_winding_moments";
    if (!s || !n || (!out && cap_nodes)) return fail(PRT_E_INVALID, std::string(who) + ": null argument");
    if (!s->winding_queries)
        return fail(PRT_E_INVALID, std::string(who) + ": winding-number queries are off for this scene (prt_scene_set_winding_queries)");
    if (const int rc = require_uploaded(s, who)) return rc;
    *n = s->k64.d.n_nodes;
    const size_t m = (size_t)std::min<uint64_t>(*n, cap_nodes);
    if (m == 0 || !s->d_moments) return PRT_OK;
    PRT_HIP_AS(who, hipDeviceSynchronize()); // a refit on any stream has written its moments
    PRT_HIP_AS(who, hipMemcpy(out, s->d_moments, m * 4 * sizeof(prt::DWindingMoment), hipMemcpyDeviceToHost));
    return PRT_OK;
}

int prt_scene_get_signed_queries(const PrtScene* s, int* on) {
    if (!s || !on) return fail(PRT_E_INVALID, "prt_scene_get_signed_queries: null argument");
    *on = s->signed_queries ? 1 : 0;
    return PRT_OK;
}

int prt_scene_topology_info(const PrtScene* s, PrtTopologyInfo* out) {
    if (!s || !out) return fail(PRT_E_INVALID, "prt_scene_topology_info: null argument");
    std::memset(out, 0, sizeof(*out));
    if (s->host_stale)
        return fail(PRT_E_INVALID, "prt_scene_topology_info: the host geometry is stale (prt_scene_refit_device / prt_scene_rebuild_device "
                                   "moved the resident geometry past it; call prt_scene_refit or prt_scene_update_vertices first)");
    try {
        prt::MeshTopology topo;
        const size_t n = s->tris.size();
        prt::build_topology(n ? &s->tris[0].v[0][0] : nullptr, sizeof(prt::HostTri) / sizeof(double), n, topo, false);
        *out = topo.info;
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, "prt_scene_topology_info: out of host memory");
    }
    out->table_bytes = s->signed_bytes;
    return PRT_OK;
}

int prt_scene_pseudonormals(PrtScene* s, double* out, uint64_t cap_tris, uint64_t* n) {
    const char* who = "prt_scene_pseudonormals";
    if (!s || !n || (!out && cap_tris)) return fail(PRT_E_INVALID, std::string(who) + ": null argument");
    if (!s->signed_queries)
        return fail(PRT_E_INVALID, std::string(who) + ": signed distance queries are off for this scene (prt_scene_set_signed_queries)");
    if (const int rc = require_uploaded(s, who)) return rc;
    const prt::DSignedTables& T = s->sq;
    *n = T.n_tris;
    const size_t m = (size_t)std::min<uint64_t>(T.n_tris, cap_tris), nn = (size_t)T.n_edges + T.n_vertices;
    if (m == 0) return PRT_OK;
    try {
        std::vector<uint32_t> slot(m * 6);
        std::vector<double> nrm(nn * 3);
        PRT_HIP_AS(who, hipDeviceSynchronize()); // a refit on any stream has written its pseudonormals
        PRT_HIP_AS(who, hipMemcpy(slot.data(), T.slot, slot.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        PRT_HIP_AS(who, hipMemcpy(nrm.data(), T.normal, nrm.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m * 6; ++i)
            for (int a = 0; a < 3; ++a) out[i * 3 + a] = slot[i] < nn ? nrm[(size_t)slot[i] * 3 + a] : 0.0;
    } catch (const std::bad_alloc&) {
        return fail(PRT_E_OOM, std::string(who) + ": out of host memory");
    }
    return PRT_OK;
}

// ---- the batched queries against the resident BVH (K1, K6, K7): one call frame for the device forms, one for the host forms
// The device frame: a call slot, K4's order when the call sorts, the entry point's launch, the slot's end.  `refuse(w)` holds
// the entry point's argument checks (w = `who`, the prefix of every text; it returns PRT_OK or what fail() returned) and
// `launch(f32, d_ctr, count, d_perm, st)` its kernel launch (a hipError_t); `who` names the public function in every
// message, a HIP runtime failure included ("<who>: <hip error string>").  d_rays is read only by the sort.
extern "C++" { // (templates: this part of the file is inside extern "C")
template <typename Refuse, typename Launch>
static int batch_device(PrtScene* s, const char* who, const void* d_rays, size_t n, int count_work, int precision, void* stream,
                        bool sorted, Refuse refuse, Launch launch) {
    int rc = require_uploaded(s, who);
    if (rc || (rc = refuse(std::string(who)))) return rc;
    const bool f32 = precision == PRT_PRECISION_F32;
    if (f32 && (rc = ensure_f32(s))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t we;
    PrtScene::CallSlot& q = *s->next_slot(st, &we);
    PRT_HIP_AS(who, we);
    const bool sort = sorted && n > 1;
    std::string err;
    if (sort) {
        const size_t need = prt::ray_sort_scratch_bytes(n, &err);
        if (!need) return fail(PRT_E_HIP, err);
        PRT_HIP_AS(who, s->sort.reserve(need, st));
    }
    PRT_HIP_AS(who, q.start(st)); // (the sort is inside the timed region: kernel_ms is keys + sort + trace)
    const uint32_t* d_perm = nullptr;
    if (sort) {
        d_perm = prt::ray_sort(static_cast<const PrtRay*>(d_rays), n, s->k64.d.grid_origin, s->k64.d.grid_step, s->sort.get<void>(),
                               s->sort.cap, st, &err);
        if (!d_perm) return fail(PRT_E_HIP, err);
    }
    const bool count = count_work != 0;
    PRT_HIP_AS(who, launch(f32, q.d_ctr.get(), count, d_perm, st));
    PRT_HIP_AS(who, q.stop(st));
    PRT_HIP_AS(who, q.finish(st, count, 0));
    if (d_perm) PRT_HIP_AS(who, s->sort.used(st));
    return PRT_OK;
}
// The checks the ray-batch entry points share, in the order that decides which message a doubly-wrong call gets.
// `aligned32`: the kernel stores a record 32 bytes at a time.
static int refuse_ray_batch(const std::string& w, bool sorted, size_t n, const void* d_rays, const void* d_out, int precision,
                            bool aligned32) {
    if (sorted && n > 0xffffffffull) return fail(PRT_E_INVALID, w + ": more than 2^32 - 1 rays in one batch");
    if (n && (!d_rays || !d_out)) return fail(PRT_E_INVALID, w + ": null buffer");
    if (precision != PRT_PRECISION_F64 && precision != PRT_PRECISION_F32) return fail(PRT_E_INVALID, w + ": unsupported precision");
    if (aligned32 && (reinterpret_cast<uintptr_t>(d_out) & 31u)) return fail(PRT_E_INVALID, w + ": output buffer is not 32-byte aligned");
    return PRT_OK;
}
// The host frame, behind the entry point's own checks (n > 0): device copies of the inputs (in1 may be null), room for the
// output, `device(d_in0, d_in1, d_out)` = the entry point's device form on the null stream, and the output back.
template <typename Device>
static int batch_host(const char* who, const void* in0, size_t in0_bytes, const void* in1, size_t in1_bytes, void* out,
                      size_t out_bytes, Device device) {
    Staging b;
    void* d_in0 = b.in(in0, in0_bytes);
    void* d_in1 = b.in(in1, in1_bytes);
    void* d_out = b.out(out_bytes);
    int rc;
    if ((rc = b.status(who)) || (rc = device(d_in0, d_in1, d_out))) return rc;
    b.sync();
    b.down(out, d_out, out_bytes);
    return b.status(who);
}
} // extern "C++"

int prt_closest_point_device(PrtScene* s, const void* d_q, size_t n, void* d_out, int count_work, void* stream) {
    return batch_device(
        s, "prt_closest_point_device", nullptr, n, count_work, PRT_PRECISION_F64, stream, false,
        [&](const std::string& w) {
            if (!s->distance_queries || !s->d_corners)
                return fail(PRT_E_INVALID, w + ": distance queries are off for this scene (prt_scene_set_distance_queries)");
            if (n && (!d_q || !d_out)) return fail(PRT_E_INVALID, w + ": null buffer");
            if (n > 0xffffffffull) return fail(PRT_E_INVALID, w + ": more than 2^32 - 1 queries in one batch");
            if (reinterpret_cast<uintptr_t>(d_out) & 31u) // the kernel stores a record 32 bytes at a time
                return fail(PRT_E_INVALID, w + ": output buffer is not 32-byte aligned");
            return PRT_OK;
        },
        [&](bool, DCounters* d_ctr, bool count, const uint32_t*, hipStream_t st) {
            return prt::launch_closest_point(s->k64.d, s->d_corners, static_cast<const PrtPointQuery*>(d_q), n,
                                             static_cast<PrtClosestPoint*>(d_out), d_ctr, count, s->stack_need, s->n_cu,
                                             dev_env("PRT_TUNE_CLOSEST_PLAIN") != nullptr, st); // (developer: the plain schedule, for A/B runs)
        });
}

int prt_closest_point(PrtScene* s, const PrtPointQuery* qs, size_t n, PrtClosestPoint* out, int count_work) {
    static_assert(sizeof(PrtPointQuery) == 32 && sizeof(PrtClosestPoint) == 64, "PrtPointQuery is 32 bytes, PrtClosestPoint 64");
    const char* who = "prt_closest_point";
    if (!s) return fail(PRT_E_INVALID, "prt_closest_point: null scene");
    if (n && (!qs || !out)) return fail(PRT_E_INVALID, "prt_closest_point: null buffer");
    if (n > 0xffffffffull) return fail(PRT_E_INVALID, "prt_closest_point: more than 2^32 - 1 queries in one batch");
    for (size_t i = 0; i < n; ++i) { // the batch is checked before anything else: a bad query is refused with or without a device
        const PrtPointQuery& q = qs[i];
        if (!(std::isfinite(q.p[0]) && std::isfinite(q.p[1]) && std::isfinite(q.p[2])))
            return fail(PRT_E_INVALID, "prt_closest_point: query " + std::to_string(i) + " has a non-finite point");
        if (!(q.max_dist >= 0.0)) return fail(PRT_E_INVALID, "prt_closest_point: query " + std::to_string(i) + " has a negative or NaN max_dist");
    }
    if (const int rc = require_uploaded(s, who)) return rc;
    if (!s->distance_queries || !s->d_corners)
        return fail(PRT_E_INVALID, "prt_closest_point: distance queries are off for this scene (prt_scene_set_distance_queries)");
    if (n == 0) return PRT_OK;
    return batch_host(who, qs, n * sizeof(PrtPointQuery), nullptr, 0, out, n * sizeof(PrtClosestPoint),
                      [&](void* dq, void*, void* dout) { return prt_closest_point_device(s, dq, n, dout, count_work, nullptr); });
}

static int refuse_unsigned(const PrtScene* s, const std::string& w) {
    if (!s->signed_queries || (s->device >= 0 && (!s->d_corners || !s->sq.slot)))
        return fail(PRT_E_INVALID, w + ": signed distance queries are off for this scene (prt_scene_set_signed_queries)");
    return PRT_OK;
}

int prt_signed_distance_device(PrtScene* s, const void* d_q, size_t n, void* d_out, int count_work, void* stream) {
    if (!s) return fail(PRT_E_INVALID, "prt_signed_distance_device: null scene");
    if (const int rc = refuse_unsigned(s, "prt_signed_distance_device")) return rc; // (before the missing device: contract 5)
    return batch_device(
        s, "prt_signed_distance_device", nullptr, n, count_work, PRT_PRECISION_F64, stream, false,
        [&](const std::string& w) {
            if (n && (!d_q || !d_out)) return fail(PRT_E_INVALID, w + ": null buffer");
            if (n > 0xffffffffull) return fail(PRT_E_INVALID, w + ": more than 2^32 - 1 queries in one batch");
            if (reinterpret_cast<uintptr_t>(d_out) & 31u) // the kernel stores a record 32 bytes at a time
                return fail(PRT_E_INVALID, w + ": output buffer is not 32-byte aligned");
            return PRT_OK;
        },
        [&](bool, DCounters* d_ctr, bool count, const uint32_t*, hipStream_t st) {
            return prt::launch_signed_distance(s->k64.d, s->d_corners, s->sq, static_cast<const PrtPointQuery*>(d_q), n,
                                               static_cast<PrtSignedDistance*>(d_out), d_ctr, count, s->stack_need, s->n_cu, st);
        });
}

int prt_signed_distance(PrtScene* s, const PrtPointQuery* qs, size_t n, PrtSignedDistance* out, int count_work) {
    static_assert(sizeof(PrtSignedDistance) == 64, "PrtSignedDistance is 64 bytes");
    const char* who = "prt_signed_distance";
    if (!s) return fail(PRT_E_INVALID, "prt_signed_distance: null scene");
    if (n && (!qs || !out)) return fail(PRT_E_INVALID, "prt_signed_distance: null buffer");
    if (n > 0xffffffffull) return fail(PRT_E_INVALID, "prt_signed_distance: more than 2^32 - 1 queries in one batch");
    for (size_t i = 0; i < n; ++i) { // the batch is checked before anything else, as prt_closest_point checks it
        const PrtPointQuery& q = qs[i];
        if (!(std::isfinite(q.p[0]) && std::isfinite(q.p[1]) && std::isfinite(q.p[2])))
            return fail(PRT_E_INVALID, "prt_signed_distance: query " + std::to_string(i) + " has a non-finite point");
        if (!(q.max_dist >= 0.0)) return fail(PRT_E_INVALID, "prt_signed_distance: query " + std::to_string(i) + " has a negative or NaN max_dist");
    }
    if (const int rc = refuse_unsigned(s, who)) return rc;
    if (const int rc = require_uploaded(s, who)) return rc;
    if (n == 0) return PRT_OK;
    return batch_host(who, qs, n * sizeof(PrtPointQuery), nullptr, 0, out, n * sizeof(PrtSignedDistance),
                      [&](void* dq, void*, void* dout) { return prt_signed_distance_device(s, dq, n, dout, count_work, nullptr); });
}

static int refuse_winding(const PrtScene* s, const std::string& w, double beta) {
    if (!s->winding_queries || (s->device >= 0 && (!s->d_corners || !s->d_moments)))
        return fail(PRT_E_INVALID, w + ": winding-number queries are off for this scene (prt_scene_set_winding_queries)");
    if (!(beta > 1.0)) return fail(PRT_E_INVALID, w + ": beta must be greater than 1 (PRT_WINDING_BETA_DEFAULT is 2; +inf sums every triangle)");
    return PRT_OK;
}

int prt_winding_number_device(PrtScene* s, const void* d_q, size_t n, double beta, void* d_out, int count_work, void* stream) {
    if (!s) return fail(PRT_E_INVALID, "prt_winding_number_device: null scene");
    if (const int rc = refuse_winding(s, "prt_winding_number_device", beta)) return rc; // (before the missing device)
    return batch_device(
        s, "prt_winding_number_device", nullptr, n, count_work, PRT_PRECISION_F64, stream, false,
        [&](const std::string& w) {
            if (n && (!d_q || !d_out)) return fail(PRT_E_INVALID, w + ": null buffer");
            if (n > 0xffffffffull) return fail(PRT_E_INVALID, w + ": more than 2^32 - 1 queries in one batch");
            if (reinterpret_cast<uintptr_t>(d_out) & 7u) // the kernel stores one double per query
                return fail(PRT_E_INVALID, w + ": output buffer is not 8-byte aligned");
            return PRT_OK;
        },
        [&](bool, DCounters* d_ctr, bool count, const uint32_t*, hipStream_t st) {
            return prt::launch_winding_number(s->k64.d, s->d_corners, s->d_moments, static_cast<const PrtPointQuery*>(d_q), n, beta,
                                              static_cast<double*>(d_out), d_ctr, count, s->stack_need, s->n_cu, st);
        });
}

int prt_winding_number(PrtScene* s, const PrtPointQuery* qs, size_t n, double beta, double* out, int count_work) {
    const char* who = "prt_winding_number";
    if (!s) return fail(PRT_E_INVALID, "prt_winding_number: null scene");
    if (const int rc = refuse_winding(s, who, beta)) return rc;
    if (n && (!qs || !out)) return fail(PRT_E_INVALID, "prt_winding_number: null buffer");
    if (n > 0xffffffffull) return fail(PRT_E_INVALID, "prt_winding_number: more than 2^32 - 1 queries in one batch");
    for (size_t i = 0; i < n; ++i) { // (max_dist is not read)
        const PrtPointQuery& q = qs[i];
        if (!(std::isfinite(q.p[0]) && std::isfinite(q.p[1]) && std::isfinite(q.p[2])))
            return fail(PRT_E_INVALID, "prt_winding_number: query " + std::to_string(i) + " has a non-finite point");
    }
    if (const int rc = require_uploaded(s, who)) return rc;
    if (n == 0) return PRT_OK;
    return batch_host(who, qs, n * sizeof(PrtPointQuery), nullptr, 0, out, n * sizeof(double),
                      [&](void* dq, void*, void* dout) { return prt_winding_number_device(s, dq, n, beta, dout, count_work, nullptr); });
}

int prt_scene_light_update_info(const PrtScene* s, PrtLightUpdateInfo* out) {
    if (!s || !out) return fail(PRT_E_INVALID, "prt_scene_light_update_info: null argument");
    std::memset(out, 0, sizeof(*out));
    const PrtScene::LightUpdate& U = s->lu;
    out->updates = U.count;
    out->host_tree_ms = U.host_tree_ms;
    out->gather_ms = U.gather_ms;
    out->n_tables = s->lights.n_tables;
    out->table_words = (uint32_t)s->lights.tab.size();
    out->tables_dropped = U.tables_dropped;
    out->relaid = U.relaid;
    if (s->device >= 0 && U.count) {
        PRT_HIP(hipSetDevice(s->device));
        float ms = 0.f;
        if (U.tables_timed) {
            PRT_HIP(hipEventSynchronize(U.t1.get()));
            PRT_HIP(hipEventElapsedTime(&ms, U.t0.get(), U.t1.get()));
            out->tables_ms = ms;
        }
    }
    return PRT_OK;
}

int prt_scene_light_table_words(PrtScene* s, uint32_t* words, uint64_t cap, uint64_t* n) {
    if (int rc = require_uploaded(s, "prt_scene_light_table_words")) return rc;
    if (!n || (!words && cap)) return fail(PRT_E_INVALID, "prt_scene_light_table_words: null argument");
    const DScene& d = s->k64.d;
    *n = d.light_tab ? s->lights.tab.size() : 0;
    const size_t k = (size_t)std::min<uint64_t>(*n, cap);
    if (k) {
        PRT_HIP(s->after_refit(nullptr)); // a light update on another stream may still be filling them
        PRT_HIP(hipMemcpy(words, d.light_tab, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return PRT_OK;
}

int prt_trace_closest_device(PrtScene* s, const void* d_rays, size_t n, void* d_hits, int count_work, void* stream) {
    return prt_trace_closest_device_prec(s, d_rays, n, d_hits, count_work, PRT_PRECISION_F64, stream);
}

// The six device calls of K1: `mode` (PRT_TRACE_*) picks what K1 writes per ray — a PrtHit, the any-hit byte (any-hit
// traversal) or a PrtSurface; `who` names the public function in error messages.
static int trace_batch_device(PrtScene* s, const void* d_rays, size_t n, void* d_out, int count_work, int precision, void* stream,
                              bool sorted, int mode, const char* who) {
    return batch_device(
        s, who, d_rays, n, count_work, precision, stream, sorted,
        [&](const std::string& w) { return refuse_ray_batch(w, sorted, n, d_rays, d_out, precision, mode == PRT_TRACE_SURFACE); },
        [&](bool f32, DCounters* d_ctr, bool count, const uint32_t* d_perm, hipStream_t st) {
            const PrtRay* rays = static_cast<const PrtRay*>(d_rays);
            return f32 ? prt32::launch_trace(s->k32.d, rays, n, d_out, d_ctr, count, mode, s->n_cu, st, d_perm)
                       : prt::launch_trace(s->k64.d, rays, n, d_out, d_ctr, count, mode, s->n_cu, st, d_perm);
        });
}
int prt_trace_closest_device_prec(PrtScene* s, const void* d_rays, size_t n, void* d_hits, int count_work, int precision,
                                  void* stream) {
    return trace_batch_device(s, d_rays, n, d_hits, count_work, precision, stream, false, PRT_TRACE_CLOSEST, "prt_trace_closest_device");
}
int prt_trace_closest_sorted_device(PrtScene* s, const void* d_rays, size_t n, void* d_hits, int count_work, int precision,
                                    void* stream) {
    return trace_batch_device(s, d_rays, n, d_hits, count_work, precision, stream, true, PRT_TRACE_CLOSEST,
                              "prt_trace_closest_sorted_device");
}
int prt_trace_occluded_device(PrtScene* s, const void* d_rays, size_t n, void* d_occluded, int count_work, int precision,
                              void* stream) {
    return trace_batch_device(s, d_rays, n, d_occluded, count_work, precision, stream, false, PRT_TRACE_ANY, "prt_trace_occluded_device");
}
int prt_trace_occluded_sorted_device(PrtScene* s, const void* d_rays, size_t n, void* d_occluded, int count_work, int precision,
                                     void* stream) {
    return trace_batch_device(s, d_rays, n, d_occluded, count_work, precision, stream, true, PRT_TRACE_ANY,
                              "prt_trace_occluded_sorted_device");
}
int prt_trace_surface_device(PrtScene* s, const void* d_rays, size_t n, void* d_out, int count_work, int precision, void* stream) {
    return trace_batch_device(s, d_rays, n, d_out, count_work, precision, stream, false, PRT_TRACE_SURFACE, "prt_trace_surface_device");
}
int prt_trace_surface_sorted_device(PrtScene* s, const void* d_rays, size_t n, void* d_out, int count_work, int precision,
                                    void* stream) {
    return trace_batch_device(s, d_rays, n, d_out, count_work, precision, stream, true, PRT_TRACE_SURFACE,
                              "prt_trace_surface_sorted_device");
}

// The three host-buffer calls of K1 (fp64, unsorted): `elem` = bytes per ray of the output (a PrtHit, the any-hit byte, or
// a PrtSurface); `who` names the public function in error messages, and its device call (`who`_device) does the work.
static int trace_batch_host(PrtScene* s, const PrtRay* rays, size_t n, void* out, size_t elem, int count_work, int mode,
                            const char* who) {
    if (const int rc = require_uploaded(s, who)) return rc;
    if (n == 0) return PRT_OK;
    if (!rays || !out) return fail(PRT_E_INVALID, std::string(who) + ": null buffer");
    const std::string dev = std::string(who) + "_device";
    return batch_host(who, rays, n * sizeof(PrtRay), nullptr, 0, out, n * elem, [&](void* dr, void*, void* dh) {
        return trace_batch_device(s, dr, n, dh, count_work, PRT_PRECISION_F64, nullptr, false, mode, dev.c_str());
    });
}
int prt_trace_closest(PrtScene* s, const PrtRay* rays, size_t n, PrtHit* hits, int count_work) {
    return trace_batch_host(s, rays, n, hits, sizeof(PrtHit), count_work, PRT_TRACE_CLOSEST, "prt_trace_closest");
}
int prt_trace_occluded(PrtScene* s, const PrtRay* rays, size_t n, uint8_t* occluded, int count_work) {
    return trace_batch_host(s, rays, n, occluded, 1, count_work, PRT_TRACE_ANY, "prt_trace_occluded");
}
int prt_trace_surface(PrtScene* s, const PrtRay* rays, size_t n, PrtSurface* out, int count_work) {
    static_assert(sizeof(PrtSurface) == 192, "PrtSurface is 192 bytes");
    return trace_batch_host(s, rays, n, out, sizeof(PrtSurface), count_work, PRT_TRACE_SURFACE, "prt_trace_surface");
}

// The two device multi-hit calls (K7, multi_hit.hip): K1's frame with the cursors and k records per ray.
static int multi_batch_device(PrtScene* s, const void* d_rays, const void* d_after, size_t n, int32_t k, void* d_hits, int count_work,
                              int precision, void* stream, bool sorted, const char* who) {
    return batch_device(
        s, who, d_rays, n, count_work, precision, stream, sorted,
        [&](const std::string& w) {
            if (k < 1 || k > PRT_MULTI_HIT_MAX) return fail(PRT_E_INVALID, w + ": k must be 1.." + std::to_string(PRT_MULTI_HIT_MAX));
            return refuse_ray_batch(w, sorted, n, d_rays, d_hits, precision, true);
        },
        [&](bool f32, DCounters* d_ctr, bool count, const uint32_t* d_perm, hipStream_t st) {
            const PrtRay* rays = static_cast<const PrtRay*>(d_rays);
            const PrtHitCursor* after = static_cast<const PrtHitCursor*>(d_after);
            PrtHit* hits = static_cast<PrtHit*>(d_hits);
            return f32 ? prt32::launch_multi_hit(s->k32.d, rays, after, n, k, hits, d_ctr, count, s->n_cu, st, d_perm)
                       : prt::launch_multi_hit(s->k64.d, rays, after, n, k, hits, d_ctr, count, s->n_cu, st, d_perm);
        });
}
int prt_trace_multi_device(PrtScene* s, const void* d_rays, const void* d_after, size_t n, int32_t k, void* d_hits, int count_work,
                           int precision, void* stream) {
    return multi_batch_device(s, d_rays, d_after, n, k, d_hits, count_work, precision, stream, false, "prt_trace_multi_device");
}
int prt_trace_multi_sorted_device(PrtScene* s, const void* d_rays, const void* d_after, size_t n, int32_t k, void* d_hits, int count_work,
                                  int precision, void* stream) {
    return multi_batch_device(s, d_rays, d_after, n, k, d_hits, count_work, precision, stream, true, "prt_trace_multi_sorted_device");
}
int prt_trace_multi(PrtScene* s, const PrtRay* rays, const PrtHitCursor* after, size_t n, int32_t k, PrtHit* hits, int count_work) {
    static_assert(sizeof(PrtHitCursor) == 16, "PrtHitCursor is 16 bytes");
    const char* who = "prt_trace_multi";
    if (!s) return fail(PRT_E_INVALID, std::string(who) + ": null scene");
    if (k < 1 || k > PRT_MULTI_HIT_MAX) return fail(PRT_E_INVALID, std::string(who) + ": k must be 1.." + std::to_string(PRT_MULTI_HIT_MAX));
    if (n && (!rays || !hits)) return fail(PRT_E_INVALID, std::string(who) + ": null buffer");
    if (after) // the cursors are checked before anything else: a bad one is refused with or without a device
        for (size_t i = 0; i < n; ++i) {
            if (after[i].t != after[i].t) return fail(PRT_E_INVALID, std::string(who) + ": cursor " + std::to_string(i) + " has a NaN t");
            if (after[i].reserved != 0) return fail(PRT_E_INVALID, std::string(who) + ": cursor " + std::to_string(i) + " has a nonzero reserved field");
        }
    if (const int rc = require_uploaded(s, who)) return rc;
    if (n == 0) return PRT_OK;
    return batch_host(who, rays, n * sizeof(PrtRay), after, n * sizeof(PrtHitCursor), hits, n * (size_t)k * sizeof(PrtHit),
                      [&](void* dr, void* da, void* dh) {
                          return multi_batch_device(s, dr, da, n, k, dh, count_work, PRT_PRECISION_F64, nullptr, false, "prt_trace_multi_device");
                      });
}

int prt_sample_lights(PrtScene* s, const double* origins, size_t n, uint64_t seed, PrtLightSample* out) {
    int rc = require_uploaded(s, "prt_sample_lights");
    if (rc) return rc;
    if (n == 0) return PRT_OK;
    if (!origins || !out) return fail(PRT_E_INVALID, "prt_sample_lights: null buffer");
    if (s->k64.d.n_lights == 0) return fail(PRT_E_INVALID, "prt_sample_lights: scene has no emissive mesh");
    Staging b;
    const double* dorg = static_cast<const double*>(b.in(origins, n * 3 * sizeof(double)));
    PrtLightSample* dout = static_cast<PrtLightSample*>(b.out(n * sizeof(PrtLightSample)));
    if ((rc = b.status("prt_sample_lights"))) return rc;
    PRT_HIP(s->after_refit(nullptr));
    prt::launch_sample_lights(s->k64.d, dorg, n, seed, dout, nullptr);
    b.sync();
    b.down(out, dout, n * sizeof(PrtLightSample));
    return b.status("prt_sample_lights");
}

int prt_material_eval(PrtScene* s, int32_t material, size_t n, const double* wi, const double* wo, const double* uv,
                      uint64_t seed, double* f) {
    int rc = require_uploaded(s, "prt_material_eval");
    if (rc) return rc;
    if (material < 0 || (size_t)material >= s->mats.size()) return fail(PRT_E_INVALID, "prt_material_eval: material index out of range");
    if (n == 0) return PRT_OK;
    if (!wi || !wo || !f) return fail(PRT_E_INVALID, "prt_material_eval: null buffer");
    Staging b;
    const double *dwi = static_cast<const double*>(b.in(wi, n * 24)), *dwo = static_cast<const double*>(b.in(wo, n * 24));
    const double* duv = static_cast<const double*>(b.in(uv, n * 16));
    double* df = static_cast<double*>(b.out(n * 24));
    if ((rc = b.status("prt_material_eval"))) return rc;
    prt::launch_material_eval(s->k64.d, material, dwi, dwo, duv, n, seed, df, nullptr);
    b.sync();
    b.down(f, df, n * 24);
    return b.status("prt_material_eval");
}

int prt_material_scatter(PrtScene* s, int32_t material, size_t n, const double* rd, const double* normal, const double* tangent,
                         const double* uv, uint64_t seed, double* wi_world, double* attenuation, int32_t* ok) {
    int rc = require_uploaded(s, "prt_material_scatter");
    if (rc) return rc;
    if (material < 0 || (size_t)material >= s->mats.size()) return fail(PRT_E_INVALID, "prt_material_scatter: material index out of range");
    if (n == 0) return PRT_OK;
    if (!rd || !normal || !tangent || !wi_world || !attenuation || !ok) return fail(PRT_E_INVALID, "prt_material_scatter: null buffer");
    Staging b;
    const double* drd = static_cast<const double*>(b.in(rd, n * 24));
    const double* duv = static_cast<const double*>(b.in(uv, n * 16));
    double *dwi = static_cast<double*>(b.out(n * 24)), *datt = static_cast<double*>(b.out(n * 24));
    int32_t* dok = static_cast<int32_t*>(b.out(n * 4));
    if ((rc = b.status("prt_material_scatter"))) return rc;
    prt::launch_material_scatter(s->k64.d, material, drd, normal, tangent, duv, n, seed, dwi, datt, dok, nullptr);
    b.sync();
    b.down(wi_world, dwi, n * 24);
    b.down(attenuation, datt, n * 24);
    b.down(ok, dok, n * 4);
    return b.status("prt_material_scatter");
}

int prt_texture_value(PrtScene* s, int32_t texture, size_t n, const double* uv, double* rgb) {
    int rc = require_uploaded(s, "prt_texture_value");
    if (rc) return rc;
    if (texture < 0 || (size_t)texture >= s->texs.size()) return fail(PRT_E_INVALID, "prt_texture_value: texture index out of range");
    if (n == 0) return PRT_OK;
    if (!uv || !rgb) return fail(PRT_E_INVALID, "prt_texture_value: null buffer");
    Staging b;
    const double* duv = static_cast<const double*>(b.in(uv, n * 16));
    double* d = static_cast<double*>(b.out(n * 24));
    if ((rc = b.status("prt_texture_value"))) return rc;
    prt::launch_texture_value(s->k64.d, texture, duv, n, d, nullptr);
    b.sync();
    b.down(rgb, d, n * 24);
    return b.status("prt_texture_value");
}

// What one K3 launch renders and where its item sums go.  prt_render_device: samples [0, spp) of a frame, scaled by 1/spp
// (Camera.cpp:83) and written by K5 into cleared framebuffers.  prt_accum_render: samples [first, first + spp), unscaled
// (the launch runs with spp = 1, so an item's partial sum is the raw sum of its samples' RayColor), added by k_accumulate
// into an accumulator's running sums; the chunks of the launch are sized for `spp` samples either way.
// prt_accum_render_adaptive sets d_list: K3 renders the list_n listed pixels (j*W+i, device memory) in chunks of
// exactly `batch` samples (spp / batch <= PRT_MAX_CHUNKS of them), and k_accumulate_list adds sums, moments and counts.
// prt_ray_color_device sets `rays`: no camera and no tiles — item oi of a chunk is ray d_rays[oi] of the caller's batch, keyed
// d_keys[oi] (or oi), samples [first, first + spp) scaled by 1/spp, and k_finalize_rays writes one triple per ray.
struct RenderPass {
    int spp;
    int32_t first = 0;
    double* d_sum = nullptr;
    const int32_t* d_list = nullptr;
    uint32_t list_n = 0;
    int batch = 0;
    double* d_moment = nullptr;
    uint32_t* d_count = nullptr;
    bool rays = false;
    const void* d_rays = nullptr;
    const void* d_keys = nullptr;
    uint64_t n_rays = 0;
};

static int render_impl(PrtScene* s, const char* who, const PrtCamera* cam, const PrtRenderParams* p, const RenderPass& pass,
                       void* d_rgb_f64, void* d_rgb_f32, int count_work, hipStream_t st);

int prt_ray_color_device(PrtScene* s, const void* d_rays, const void* d_keys, size_t n, const PrtRenderParams* p, int32_t sample_begin,
                         void* d_rgb_f64, void* d_rgb_f32, void* stream) {
    const char* who = "prt_ray_color_device";
    int rc = require_uploaded(s, who);
    if (rc) return rc;
    const std::string w(who);
    if (!p) return fail(PRT_E_INVALID, w + ": null argument");
    if (n && !d_rays) return fail(PRT_E_INVALID, w + ": null ray buffer");
    if (!d_rgb_f64 && !d_rgb_f32) return fail(PRT_E_INVALID, w + ": both outputs are null");
    if (p->spp < 1) return fail(PRT_E_INVALID, w + ": spp must be >= 1");
    if (sample_begin < 0 || (int64_t)sample_begin + p->spp > (int64_t)INT32_MAX) return fail(PRT_E_INVALID, w + ": bad sample range");
    if (p->pixel_jitter || p->reserved) return fail(PRT_E_INVALID, w + ": pixel_jitter and reserved must be 0 (a ray has no pixel to jitter)");
    if (n >= 0xffffffffULL) return fail(PRT_E_LIMIT, w + ": more than 2^32 work items (rays x sample chunks) in one launch");
    RenderPass pass;
    pass.spp = p->spp;
    pass.first = sample_begin;
    pass.rays = true;
    pass.d_rays = d_rays;
    pass.d_keys = d_keys;
    pass.n_rays = n;
    return render_impl(s, who, nullptr, p, pass, d_rgb_f64, d_rgb_f32, 0, reinterpret_cast<hipStream_t>(stream));
}

int prt_ray_color(PrtScene* s, const PrtRay* rays, const uint32_t* keys, size_t n, const PrtRenderParams* p, int32_t sample_begin,
                  double* rgb_f64, float* rgb_f32) {
    const char* who = "prt_ray_color";
    int rc = require_uploaded(s, who);
    if (rc) return rc;
    if (n && !rays) return fail(PRT_E_INVALID, "prt_ray_color: null ray buffer");
    if (n >= 0xffffffffULL) return fail(PRT_E_LIMIT, "prt_ray_color: more than 2^32 work items (rays x sample chunks) in one launch");
    for (size_t i = 0; i < n; ++i) {
        const PrtRay& r = rays[i];
        bool ok = r.d[0] != 0.0 || r.d[1] != 0.0 || r.d[2] != 0.0;
        for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(r.o[a]) && std::isfinite(r.d[a]);
        if (!ok) return fail(PRT_E_INVALID, "prt_ray_color: ray " + std::to_string(i) + " has a non-finite origin or direction, or a zero direction");
    }
    Staging b;
    void* dr = b.in(rays, n * sizeof(PrtRay));
    void* dk = b.in(keys, n * sizeof(uint32_t));
    void* d64 = rgb_f64 ? b.out(n * 3 * sizeof(double)) : nullptr;
    void* d32 = rgb_f32 ? b.out(n * 3 * sizeof(float)) : nullptr;
    if ((rc = b.status(who)) || (rc = prt_ray_color_device(s, dr, dk, n, p, sample_begin, d64, d32, nullptr)))
        return rc;
    b.sync();
    if (rgb_f64) b.down(rgb_f64, d64, n * 3 * sizeof(double));
    if (rgb_f32) b.down(rgb_f32, d32, n * 3 * sizeof(float));
    return b.status(who);
}

int prt_render_device(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, void* d_rgb_f64, void* d_rgb_f32,
                      int count_work, void* stream) {
    int rc = require_uploaded(s, "prt_render_device");
    if (rc) return rc;
    if (!cam || !p) return fail(PRT_E_INVALID, "prt_render_device: null argument");
    if (cam->width < 1 || cam->height < 1) return fail(PRT_E_INVALID, "prt_render_device: bad image size");
    if (p->spp < 1) return fail(PRT_E_INVALID, "prt_render_device: spp must be >= 1");
    RenderPass pass;
    pass.spp = p->spp;
    return render_impl(s, "prt_render_device", cam, p, pass, d_rgb_f64, d_rgb_f32, count_work, reinterpret_cast<hipStream_t>(stream));
}

static int render_impl(PrtScene* s, const char* who, const PrtCamera* cam, const PrtRenderParams* p, const RenderPass& pass,
                       void* d_rgb_f64, void* d_rgb_f32, int count_work, hipStream_t st) {
    int rc = PRT_OK;
    const std::string w(who);
    if (p->precision != PRT_PRECISION_F64 && p->precision != PRT_PRECISION_F32) return fail(PRT_E_INVALID, w + ": unsupported precision");
    const bool f32 = p->precision == PRT_PRECISION_F32;
    if (f32 && (rc = ensure_f32(s))) return rc;
    if (!pass.rays && (p->nranks < 1 || p->rank < 0 || p->rank >= p->nranks)) return fail(PRT_E_INVALID, w + ": bad rank/nranks");

    DCamera C;
    if (pass.rays) std::memset(&C, 0, sizeof(C)); // (the ray-batch kernels have no camera)
    else prt::setup_camera(*cam, C);
    DRenderParams P = base_params(s, p);
    P.spp = pass.d_sum ? 1 : pass.spp;
    P.cached_min = 24; // measured: veach-mis -1 %, the others flat
    // (developer overrides of the wave scheduling thresholds through the environment, for sweeps)
    if (const char* e = dev_env("PRT_TUNE_CACHED_MIN")) P.cached_min = std::max(1, std::atoi(e)); // (0 would keep a wave passing for ever)
    if (const char* e = dev_env("PRT_TUNE_CHAIN_MIN")) P.chain_min = std::min(65, std::max(1, std::atoi(e))); // (65: never between rounds; 0 would let a wave take chain steps that chain nothing, for ever)
    if (const char* e = dev_env("PRT_TUNE_KEEP")) P.keep = std::min(64, std::max(0, std::atoi(e))); // (< 0 would keep a wave traversing once every lane is idle)
    if (const char* e = dev_env("PRT_TUNE_LEAF_BATCH")) P.leaf_batch = std::min(64, std::max(1, std::atoi(e))); // (a batch is 1 to 64 lanes of a wave)
    if (const char* e = dev_env("PRT_TUNE_INNER_MIN")) P.inner_min = std::min(64, std::max(0, std::atoi(e))); // (< 0 would never test the leaves of a wave whose lanes are all parked)
    if (const char* e = dev_env("PRT_TUNE_SCRAMBLE")) P.scramble = std::atoi(e) ? 1 : 0; // experiment: incoherent pixel order (PRT_ITEMS_FROM_LIST is set by adaptive rounds below and by prt_render_samples)
    uint64_t owned_pixels = pass.n_rays;
    if (pass.rays) { // one "tile" that is never mapped to pixels: the items are the rays
        P.scramble = 0;
        P.tile = 8; P.tiles_x = P.tiles_y = P.n_tiles = 1; P.rank = 0; P.nranks = 1; P.owned_tiles = 1;
        P.items_per_chunk = pass.n_rays;
    } else {
        const TileLayout L(*cam, *p);
        L.set(P);
        owned_pixels = L.owned_pixels();
    }
    if (pass.d_list) { // an adaptive round: the listed pixels (all owned by this rank) instead of the owned tiles
        P.scramble = PRT_ITEMS_FROM_LIST;
        P.items_per_chunk = pass.list_n;
    }
    const bool count = count_work != 0;
    const bool plain = !generic_forced() && (f32 ? frame_plain(s, s->k32, count, pass.rays, P.jitter, P.scramble, P.sample_lights)
                                                 : frame_plain(s, s->k64, count, pass.rays, P.jitter, P.scramble, P.sample_lights));
    const bool diffuse = plain && !diffuse_off() && !f32 && frame_diffuse(s, s->k64, count, pass.rays, P.jitter, P.scramble, P.sample_lights);
    int bpc = (f32 ? s->k32.blocks_per_cu : s->k64.blocks_per_cu)[count ? 1 : diffuse ? 3 : plain ? 2 : 0];
    if (pass.rays) bpc = f32 ? rays_blocks_per_cu(s, s->k32) : rays_blocks_per_cu(s, s->k64);
    const uint64_t lanes = (uint64_t)s->n_cu * bpc * PRT_BLOCK;
    // Work item = (pixel, chunk of samples), dealt chunk-major from PRT_ITEM_QUEUES counters (prt_types.h).
    //  * explicit sample_chunks: that many equal chunks;
    //  * auto: guided self-scheduling.  The launch ends when the LAST lane finishes, so no item may be
    //    handed out that can outlast the work still queued behind it.  Items of one chunk cover every owned
    //    pixel, pixels differ in cost by a factor `var` (a pixel looking into the box interior traces ~3x the
    //    rays of the average one), and `lanes` lanes drain the queue, so chunk j may hold at most
    //        s_j <= (pixels / lanes) / var * (samples in all later chunks)
    //    samples.  Built from the last chunk (1 sample) backwards this gives a geometric tail whose ratio
    //    depends on the share: x2.8 per chunk for a full 1024^2 frame, x1.2 for a 1/8 tile share — where
    //    a fixed halving tail left lanes finishing 32-sample items 5.8 ms after the queue ran dry (measured
    //    with per-wave timestamps: 58.3 ms launch, queue dry at 52.5 ms).  Sizes are capped at `body`
    //    samples; the per-item fetch is one wave-aggregated atomic.
    std::vector<int> sizes;
    const int spp = pass.spp;
    int want = p->sample_chunks;
    if (const char* e = dev_env("PRT_TUNE_CHUNKS")) want = std::atoi(e);
    if (pass.d_list) {
        for (int c = 0; c < spp / pass.batch; ++c) sizes.push_back(pass.batch);
    } else if (want > 0) {
        want = std::min(want, std::min(spp, PRT_MAX_CHUNKS));
        for (int c = 0; c < want; ++c) sizes.push_back((int)(((int64_t)(c + 1) * spp) / want - ((int64_t)c * spp) / want));
    } else if (P.items_per_chunk == 0) {
        sizes.push_back(spp);
    } else {
        // largest item: beyond ~100 samples the per-item costs are already amortised; a small tile share (fewer owned
        // pixels than resident lanes x 2) does 1 % better with 64 (53.1 -> 52.6 ms on a 1/8 share of the cornell frame)
        int body = P.items_per_chunk < 2 * lanes ? 64 : 128;
        if (const char* e = dev_env("PRT_TUNE_BODY")) body = std::max(1, std::atoi(e));
        body = std::max(body, (spp + PRT_MAX_CHUNKS / 2 - 1) / (PRT_MAX_CHUNKS / 2)); // very high spp: the body must fit in half the table
        double var = 4.0; // measured optimum with the multi-queue item dealing (3 before it: short items were fetch-bound)
        if (const char* e = dev_env("PRT_TUNE_VAR")) var = std::max(0.25, std::atof(e));
        double c = ((double)P.items_per_chunk / (double)lanes) / var;
        for (;;) {
            sizes.clear();
            int64_t sum = 0;
            while (sum < spp && (int)sizes.size() <= PRT_MAX_CHUNKS) {
                int64_t sz = (int64_t)std::floor(c * (double)sum);
                sz = std::max<int64_t>(1, std::min<int64_t>(sz, body));
                sz = std::min<int64_t>(sz, spp - sum);
                sizes.push_back((int)sz);
                sum += sz;
            }
            if ((int)sizes.size() <= PRT_MAX_CHUNKS) break;
            c *= 1.25; // a tiny share would need more chunks than the partial-sum table holds: steepen the tail
            if (c > 1e9) body *= 2; // (cannot happen with the body bound above; keeps the loop finite regardless)
        }
        std::reverse(sizes.begin(), sizes.end()); // largest chunks first
    }
    sizes.erase(std::remove(sizes.begin(), sizes.end(), 0), sizes.end());
    if (sizes.empty()) sizes.push_back(spp);
    int chunks = (int)sizes.size();
    P.chunk_begin[0] = pass.first;
    for (int c = 0; c < chunks; ++c) P.chunk_begin[c + 1] = P.chunk_begin[c] + sizes[c];
    P.chunks = chunks;
    P.n_items = P.items_per_chunk * (uint64_t)chunks;
    if (P.n_items >= 0xffffffffULL) return fail(PRT_E_LIMIT, w + ": more than 2^32 work items (pixels x sample chunks) in one launch");

    const size_t need = std::max<size_t>(P.n_items * 3, 3);
    hipError_t we;
    PrtScene::CallSlot& q = *s->next_slot(st, &we);
    PRT_HIP(we);
    PRT_HIP(q.partial.reserve(need * sizeof(double), st));
    double* d_partial = q.partial.get<double>();
    const size_t npx = pass.rays ? (size_t)pass.n_rays * 3 : (size_t)C.width * C.height * 3;
    DevBuf<> dump_buf;
    unsigned long long dump_cap = 0;
    std::string dump_path;
    if (d_rgb_f64 && npx) PRT_HIP(hipMemsetAsync(d_rgb_f64, 0, npx * sizeof(double), st));
    if (d_rgb_f32 && npx) PRT_HIP(hipMemsetAsync(d_rgb_f32, 0, npx * sizeof(float), st));
    PRT_HIP(q.start(st));
    // maxDepth < 0: RayColor returns 0 before it traces anything (Camera.cpp:121) — the cleared framebuffer is the frame
    if (P.max_depth < 0) P.n_items = 0;
    if (P.n_items) {
        const uint64_t want = (P.n_items + PRT_BLOCK - 1) / PRT_BLOCK;
        const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)s->n_cu * bpc));
        PRT_HIP(q.set_pointers(st, pass.d_list, nullptr));
        if (pass.rays) PRT_HIP(q.set_rays(st, pass.d_rays, pass.d_keys));
        if (const char* e = dev_env("PRT_TUNE_DUMP_RAYS")) { // "<max rays>,<file>" (counting launches only)
            const std::string v(e);
            const size_t comma = v.find(',');
            if (count && comma != std::string::npos) {
                dump_cap = std::strtoull(v.substr(0, comma).c_str(), nullptr, 10);
                dump_path = v.substr(comma + 1);
                PRT_HIP(dev_alloc(dump_buf, (size_t)dump_cap * sizeof(PrtRay)));
                const unsigned long long vals[3] = {(unsigned long long)(uintptr_t)dump_buf.get(), dump_cap, 0ULL};
                PRT_HIP(hipMemcpyAsync(reinterpret_cast<char*>(q.d_ctr.get()) + offsetof(DCounters, ray_dump), vals, sizeof(vals), hipMemcpyHostToDevice, st));
            }
        }
        // fp32: the same camera and parameters rounded to float (K5 below works from the fp64 originals: it only maps pixels)
        if (f32) prt32::launch_render(s->k32.d, to_f32(C), to_f32(P, s->k32), d_partial, q.d_ctr.get(), count, s->feat, grid, st, pass.rays, plain, false);
        else prt::launch_render(s->k64.d, C, P, d_partial, q.d_ctr.get(), count, s->feat, grid, st, pass.rays, plain, diffuse);
        note_render_form(plain, diffuse);
        PRT_HIP(hipGetLastError());
    }
    PRT_HIP(q.stop(st));
    if (dump_buf) { // developer experiment: write K3's ray stream to the file (synchronous)
        PRT_HIP(hipStreamSynchronize(st));
        DCounters h;
        PRT_HIP(hipMemcpy(&h, q.d_ctr.get(), sizeof(h), hipMemcpyDeviceToHost));
        const size_t nd = (size_t)std::min<unsigned long long>(h.ray_dump_n, dump_cap);
        std::vector<PrtRay> rays(nd);
        PRT_HIP(hipMemcpy(rays.data(), dump_buf.get(), nd * sizeof(PrtRay), hipMemcpyDeviceToHost));
        dump_buf.reset();
        if (FILE* f = std::fopen(dump_path.c_str(), "wb")) {
            std::fwrite(rays.data(), sizeof(PrtRay), nd, f);
            std::fclose(f);
        }
        std::fprintf(stderr, "[prt] dumped %zu of %llu rays to %s\n", nd, h.ray_dump_n, dump_path.c_str());
    }
    if (pass.d_list) {
        // maxDepth < 0: no item ran, and every sample is 0; the counts still grow
        if (!P.n_items) PRT_HIP(hipMemsetAsync(d_partial, 0, need * sizeof(double), st));
        prt::launch_accumulate_list(P, d_partial, pass.d_list, (uint32_t)pass.batch, (uint32_t)spp, pass.d_sum, pass.d_moment,
                                    pass.d_count, st);
        PRT_HIP(hipGetLastError());
    } else if (P.n_items) {
        if (pass.rays) prt::launch_finalize_rays(P, d_partial, static_cast<double*>(d_rgb_f64), static_cast<float*>(d_rgb_f32), st);
        else if (pass.d_sum) prt::launch_accumulate(C, P, d_partial, pass.d_sum, st);
        else prt::launch_finalize(C, P, d_partial, static_cast<double*>(d_rgb_f64), static_cast<float*>(d_rgb_f32), st);
        PRT_HIP(hipGetLastError());
    }
    const uint64_t samples = !P.n_items ? 0 : pass.d_list ? (uint64_t)pass.list_n * (uint64_t)spp : owned_pixels * (uint64_t)spp;
    PRT_HIP(q.finish(st, count, samples));
    return PRT_OK;
}

int prt_render(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, double* rgb_f64, float* rgb_f32) {
    int rc = require_uploaded(s, "prt_render");
    if (rc) return rc;
    if (!cam || !p) return fail(PRT_E_INVALID, "prt_render: null argument");
    if (cam->width < 1 || cam->height < 1) return fail(PRT_E_INVALID, "prt_render: bad image size");
    const size_t npx = (size_t)cam->width * cam->height * 3;
    Staging b;
    void* d64 = rgb_f64 ? b.out(npx * sizeof(double)) : nullptr;
    void* d32 = rgb_f32 ? b.out(npx * sizeof(float)) : nullptr;
    if ((rc = b.status("prt_render")) || (rc = prt_render_device(s, cam, p, d64, d32, 0, nullptr))) return rc;
    b.sync();
    if (rgb_f64) b.down(rgb_f64, d64, npx * sizeof(double));
    if (rgb_f32) b.down(rgb_f32, d32, npx * sizeof(float));
    return b.status("prt_render");
}

// Test hook (prt.h): single camera samples through K3.  One work item per (listed pixel, sample): the sample chunks of a
// launch are the samples themselves (at most PRT_MAX_CHUNKS per launch), spp = 1 so that nothing is scaled, and the item's
// partial sum IS the sample's RayColor.
int prt_render_samples(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, const int32_t* pixel_xy, size_t n_pixels,
                       int32_t sample_begin, int32_t sample_count, double* radiance, int32_t* trace) {
    const char* who = "prt_render_samples";
    int rc = require_uploaded(s, who);
    if (rc) return rc;
    if (!cam || !p || (n_pixels && (!pixel_xy || !radiance))) return fail(PRT_E_INVALID, "prt_render_samples: null argument");
    if (cam->width < 1 || cam->height < 1) return fail(PRT_E_INVALID, "prt_render_samples: bad image size");
    if (p->precision != PRT_PRECISION_F64) return fail(PRT_E_INVALID, "prt_render_samples: fp64 only");
    if (sample_begin < 0 || sample_count < 0) return fail(PRT_E_INVALID, "prt_render_samples: bad sample range");
    if (n_pixels == 0 || sample_count == 0) return PRT_OK;
    if (n_pixels * (size_t)PRT_MAX_CHUNKS >= 0xffffffffULL) return fail(PRT_E_LIMIT, "prt_render_samples: too many pixels");
    std::vector<int32_t> pix(n_pixels);
    for (size_t k = 0; k < n_pixels; ++k) {
        const int32_t i = pixel_xy[2 * k], j = pixel_xy[2 * k + 1];
        if (i < 0 || j < 0 || i >= cam->width || j >= cam->height) return fail(PRT_E_INVALID, "prt_render_samples: pixel outside the image");
        pix[k] = j * cam->width + i;
    }
    DCamera C;
    prt::setup_camera(*cam, C);
    DRenderParams P = base_params(s, p);
    P.spp = 1;
    P.scramble = PRT_ITEMS_FROM_LIST;
    P.cached_min = 65;
    P.tile = 8; P.tiles_x = P.tiles_y = P.n_tiles = 1; P.rank = 0; P.nranks = 1; P.owned_tiles = 1; // (the items come from the list)
    P.items_per_chunk = n_pixels;
    const bool count = trace != nullptr;
    const bool plain = !generic_forced() && frame_plain(s, s->k64, count, false, P.jitter, P.scramble, P.sample_lights); // (false: the items come from a list)
    const int bpc = s->k64.blocks_per_cu[count ? 1 : plain ? 2 : 0];
    const size_t per_launch = n_pixels * (size_t)std::min<int>(sample_count, PRT_MAX_CHUNKS);
    Staging b;
    const int32_t* d_pix = static_cast<const int32_t*>(b.in(pix.data(), n_pixels * sizeof(int32_t)));
    double* d_part = static_cast<double*>(b.out(per_launch * 3 * sizeof(double)));
    int32_t* d_trace = trace ? static_cast<int32_t*>(b.out(per_launch * PRT_TRACE_WORDS * sizeof(int32_t))) : nullptr;
    if ((rc = b.status(who))) return rc;
    std::vector<double> part(per_launch * 3);
    std::vector<int32_t> tr(trace ? per_launch * PRT_TRACE_WORDS : 0);
    for (int32_t s0 = 0; s0 < sample_count; s0 += PRT_MAX_CHUNKS) {
        const int chunks = std::min<int>(PRT_MAX_CHUNKS, sample_count - s0);
        for (int c = 0; c <= chunks; ++c) P.chunk_begin[c] = sample_begin + s0 + c;
        P.chunks = chunks;
        P.n_items = P.items_per_chunk * (uint64_t)chunks;
        hipError_t we;
        PrtScene::CallSlot& q = *s->next_slot(nullptr, &we);
        PRT_HIP_AS(who, we);
        const uint64_t want = (P.n_items + PRT_BLOCK - 1) / PRT_BLOCK;
        const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)s->n_cu * bpc));
        if (d_trace) PRT_HIP_AS(who, hipMemset(d_trace, 0, (size_t)P.n_items * PRT_TRACE_WORDS * sizeof(int32_t)));
        PRT_HIP_AS(who, q.start(nullptr));
        PRT_HIP_AS(who, q.set_pointers(nullptr, d_pix, d_trace));
        if (P.max_depth >= 0) {
            prt::launch_render(s->k64.d, C, P, d_part, q.d_ctr.get(), count, s->feat, grid, nullptr, false, plain, false); // (a list: never PLAIN, so never DIFFUSE)
            note_render_form(plain, false);
        } else PRT_HIP_AS(who, hipMemset(d_part, 0, (size_t)P.n_items * 3 * sizeof(double)));
        PRT_HIP_AS(who, hipGetLastError());
        PRT_HIP_AS(who, q.stop(nullptr));
        PRT_HIP_AS(who, q.finish(nullptr, count, P.max_depth >= 0 ? P.n_items : 0));
        PRT_HIP_AS(who, hipDeviceSynchronize());
        PRT_HIP_AS(who, hipMemcpy(part.data(), d_part, (size_t)P.n_items * 3 * sizeof(double), hipMemcpyDeviceToHost));
        if (trace) PRT_HIP_AS(who, hipMemcpy(tr.data(), d_trace, (size_t)P.n_items * PRT_TRACE_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int c = 0; c < chunks; ++c)
            for (size_t k = 0; k < n_pixels; ++k) { // item = chunk * n_pixels + k  ->  out[k][s0 + c]
                const size_t item = (size_t)c * n_pixels + k, o = k * (size_t)sample_count + (size_t)(s0 + c);
                std::memcpy(radiance + o * 3, part.data() + item * 3, 3 * sizeof(double));
                if (trace) std::memcpy(trace + o * PRT_TRACE_WORDS, tr.data() + item * PRT_TRACE_WORDS, PRT_TRACE_WORDS * sizeof(int32_t));
            }
    }
    return PRT_OK;
}

namespace {
// One RCCL communicator set per list of devices, created on first use and kept for the life of the process
// (ncclCommInitAll takes hundreds of milliseconds; a frame takes tens).
struct CommSet {
    std::vector<ncclComm_t> comms;
};
std::mutex g_comm_mutex;
std::map<std::vector<int>, CommSet> g_comms;
} // namespace

namespace {
// Restores the caller's current HIP device on every way out of a call that visits several devices.
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};
void drop_comms_locked(std::map<std::vector<int>, CommSet>::iterator it, bool abort) {
    for (ncclComm_t c : it->second.comms)
        if (c) (void)(abort ? ncclCommAbort(c) : ncclCommDestroy(c));
    g_comms.erase(it);
}

int render_multi_impl(PrtScene* const* scenes, int n, const PrtCamera* cam, const PrtRenderParams* p, float* rgb_f32) {
    std::vector<int> devs(n);
    for (int r = 0; r < n; ++r) {
        if (!scenes[r]) return fail(PRT_E_INVALID, "prt_render_multi: null scene");
        if (scenes[r]->device < 0) return fail(PRT_E_NO_DEVICE, "prt_render_multi: a scene is not uploaded to a HIP device (no CPU path exists)");
        for (int q = 0; q < r; ++q)
            if (scenes[q] == scenes[r]) return fail(PRT_E_INVALID, "prt_render_multi: the same scene handle twice (one handle per tile share)");
        devs[r] = scenes[r]->device;
    }
    bool all_same = true, all_distinct = true;
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < r; ++q) {
            if (devs[q] == devs[r]) all_distinct = false;
            else all_same = false;
        }
    if (n > 1 && !all_same && !all_distinct)
        return fail(PRT_E_INVALID, "prt_render_multi: scenes must sit on pairwise different devices (RCCL reduce) or all on one device");
    const size_t npx = (size_t)cam->width * cam->height * 3;
    // every share renders its tiles into its device's zeroed full-size fp32 framebuffer
    for (int r = 0; r < n; ++r) {
        PrtScene* s = scenes[r];
        PRT_HIP(hipSetDevice(s->device));
        PRT_HIP(s->multi_fb.reserve(npx * sizeof(float), nullptr));
        PrtRenderParams pr = *p;
        pr.tile_size = n > 1 ? 16 : p->tile_size;
        pr.rank = r;
        pr.nranks = n;
        const int rc = prt_render_device(s, cam, &pr, nullptr, s->multi_fb.get<void>(), 0, nullptr);
        if (rc != PRT_OK) return rc;
    }
    // test hooks (PRT_DEV_HOOKS builds only).  PRT_TEST_FORCE_RCCL: a single scene goes through the RCCL branch as well (a
    // communicator of one rank) — the most of that branch a one-GPU box can execute: library, communicator, the grouped
    // reduce on the device buffer, the stream order.  PRT_TEST_FAIL_NCCL=init|reduce: that step reports a failure.
    const bool force_rccl = n == 1 && dev_env("PRT_TEST_FORCE_RCCL") && std::atoi(dev_env("PRT_TEST_FORCE_RCCL"));
    const char* inject = dev_env("PRT_TEST_FAIL_NCCL");
    if (n > 1 && all_same) {
        // tile shares of one device (replicas; a rehearsal of the multi-GPU path on one GPU): summed where they are
        PRT_HIP(hipSetDevice(devs[0]));
        for (int r = 1; r < n; ++r) prt::launch_add_f32(scenes[0]->multi_fb.get<float>(), scenes[r]->multi_fb.get<float>(), npx, nullptr);
        PRT_HIP(hipGetLastError());
    } else if (n > 1 || force_rccl) {
        // ONE collective: reduce(sum) of the fp32 framebuffers to the first device over RCCL (xGMI between the GPUs of a
        // node).  Tiles are disjoint, so every element is x + 0 + ... + 0: the reduce is exact.  The communicator set of a
        // device list is created once and kept (prt_shutdown destroys them); the mutex is held for the whole collective,
        // so two host threads cannot interleave grouped calls on the same communicators.
        std::lock_guard<std::mutex> lock(g_comm_mutex);
        auto it = g_comms.find(devs);
        if (it == g_comms.end()) {
            CommSet fresh;
            fresh.comms.assign(n, nullptr);
            ncclResult_t nr = (inject && !std::strcmp(inject, "init")) ? ncclSystemError : ncclCommInitAll(fresh.comms.data(), n, devs.data());
            if (nr != ncclSuccess) {
                for (ncclComm_t c : fresh.comms) // whatever a failed initialisation left behind
                    if (c) (void)ncclCommAbort(c);
                return fail(PRT_E_HIP, std::string("prt_render_multi: ncclCommInitAll failed: ") + ncclGetErrorString(nr) +
                                           " (no host-side fallback exists: the frame is not assembled)");
            }
            it = g_comms.emplace(devs, std::move(fresh)).first;
        }
        CommSet& cs = it->second;
        // Every error between ncclGroupStart and ncclGroupEnd is COLLECTED: the group is always closed before the call fails.
        std::string what;
        ncclResult_t nr = ncclGroupStart();
        if (nr != ncclSuccess) return fail(PRT_E_HIP, std::string("prt_render_multi: ncclGroupStart failed: ") + ncclGetErrorString(nr));
        for (int r = 0; r < n && nr == ncclSuccess; ++r) {
            const hipError_t he = hipSetDevice(devs[r]);
            if (he != hipSuccess) {
                what = std::string("hipSetDevice: ") + hipGetErrorString(he);
                nr = ncclUnhandledCudaError;
                break;
            }
            nr = (inject && !std::strcmp(inject, "reduce")) ? ncclInternalError
                 : ncclReduce(scenes[r]->multi_fb.get<float>(), scenes[r]->multi_fb.get<float>(), npx, ncclFloat, ncclSum, 0, cs.comms[r], nullptr);
        }
        const ncclResult_t ne = ncclGroupEnd();
        if (nr == ncclSuccess) nr = ne;
        if (nr != ncclSuccess) {
            drop_comms_locked(it, true); // a communicator that failed a collective is not used again
            return fail(PRT_E_HIP, std::string("prt_render_multi: ncclReduce failed: ") + ncclGetErrorString(nr) + (what.empty() ? "" : " (" + what + ")"));
        }
        for (int r = 1; r < n; ++r) { // the root's copy below only waits for the root's stream
            PRT_HIP(hipSetDevice(devs[r]));
            PRT_HIP(hipDeviceSynchronize());
        }
    }
    PRT_HIP(hipSetDevice(devs[0]));
    PRT_HIP(hipDeviceSynchronize());
    PRT_HIP(hipMemcpy(rgb_f32, scenes[0]->multi_fb.get<float>(), npx * sizeof(float), hipMemcpyDeviceToHost));
    return PRT_OK;
}
} // namespace

// Camera::Render over several GPUs of this process (prt.h).  Single host thread: every device's launches are
// asynchronous; the reduce is one grouped RCCL call.  The caller's current device is restored on every way out.
// EXPERIMENTAL for n > 1 on different devices: that branch has only ever run with a one-rank communicator (rounds 1-4
// had one-GPU boxes); the result is an fp32 framebuffer (the reduce's element type), not the fp64 one of prt_render.
int prt_render_multi(PrtScene* const* scenes, int n, const PrtCamera* cam, const PrtRenderParams* p, float* rgb_f32) {
    if (!scenes || n < 1 || !cam || !p || !rgb_f32) return fail(PRT_E_INVALID, "prt_render_multi: null argument");
    if (cam->width < 1 || cam->height < 1) return fail(PRT_E_INVALID, "prt_render_multi: bad image size");
    DeviceGuard guard;
    return render_multi_impl(scenes, n, cam, p, rgb_f32);
}

// Releases what the library keeps for the whole process: the cached RCCL communicators of prt_render_multi.  Scenes are
// not touched (prt_scene_destroy).  Call it before the process exits when prt_render_multi ran over several devices; safe
// to call any number of times, and prt_render_multi creates communicators again when it needs them.
void prt_shutdown(void) {
    std::lock_guard<std::mutex> lock(g_comm_mutex);
    DeviceGuard guard;
    while (!g_comms.empty()) drop_comms_locked(g_comms.begin(), false);
}

int prt_get_counters(PrtScene* s, PrtCounters* out) {
    if (!s || !out) return fail(PRT_E_INVALID, "prt_get_counters: null argument");
    PrtCounters c = s->last;
    c.bvh_nodes = s->bvh_info.n_nodes; // host- and device-built trees alike (bvh.nodes is empty for the latter)
    c.bvh_depth = s->bvh_info.depth;
    PrtScene::CallSlot& q = s->slots[s->cur];
    if (s->device >= 0 && q.timed) {
        PRT_HIP(hipSetDevice(s->device));
        PRT_HIP(hipEventSynchronize(q.ev1.get()));
        float ms = 0.f;
        PRT_HIP(hipEventElapsedTime(&ms, q.ev0.get(), q.ev1.get()));
        DCounters h;
        PRT_HIP(hipMemcpy(&h, q.d_ctr.get(), sizeof(h), hipMemcpyDeviceToHost));
        c.rays_closest = h.rays_closest;
        c.rays_shadow = h.rays_shadow;
        c.node_fetches = h.node_fetches;
        c.tri_tests = h.tri_tests;
        c.samples = q.samples;
        c.inner_rounds = h.inner_rounds;
        c.leaf_rounds = h.leaf_rounds;
        c.refills = h.refills;
        c.tri_full = h.tri_full;
        c.kernel_ms = ms;
    }
    s->last = c;
    *out = c;
    return PRT_OK;
}

// ------------------------------------------------------------------ progressive rendering (PrtAccum)
} // extern "C"

// Running fp64 sums of every sample rendered so far, one per real of the full frame (pixels of other ranks' tiles stay 0).
// Camera and parameters are frozen at create time.  `done` is recorded behind the last kernel that read or wrote the sums,
// and every later use of them waits for it first: passes on different streams are ordered, not raced.
struct PrtAccum {
    PrtScene* scene = nullptr;
    PrtCamera cam{};
    PrtRenderParams params{};
    int device = -1;
    uint64_t generation = 0; // the scene geometry (PrtScene::generation) the sums were rendered from
    uint64_t samples = 0;
    uint64_t fingerprint = 0;
    size_t n = 0; // W * H * 3
    DevBuf<double> d_sum;
    Event done;
    // adaptive accumulators (prt_accum_create_adaptive): `samples` is the global count n, and per pixel a second moment and
    // a sample count; a round's active pixels are listed in d_list (d_seg: the select's per-segment counts, d_active: the
    // list's length, read back through the pinned h_active)
    bool adaptive = false;
    PrtAdaptiveParams ad{}; // with the effective batch
    DevBuf<double> d_moment;
    DevBuf<uint32_t> d_count;
    DevBuf<int32_t> d_list;
    DevBuf<uint32_t> d_seg;
    DevBuf<uint32_t> d_active;
    std::unique_ptr<uint32_t, HipHostFree> h_active;
    // prt_accum_resolve_denoised: the cached features (albedo [n], normal [n], depth [n / 3] floats) of scene generation
    // feat_gen traced with feat_spp samples, the resolved fp32 frame and the denoised one (when the caller wants only bytes)
    DevBuf<float> d_feat;
    bool feat_valid = false;
    uint64_t feat_gen = 0;
    int32_t feat_spp = 0;
    DevBuf<float> d_res32;
    DevBuf<float> d_dn32;
    DevBuf<float> d_var32; // prt_accum_resolve_denoised_guided: the variance plane (W * H floats)
};

namespace {
struct Fnv {
    uint64_t h = 1469598103934665603ULL;
    template <typename T>
    void add(const T& v) {
        unsigned char b[sizeof(T)];
        std::memcpy(b, &v, sizeof(T));
        for (unsigned char c : b) h = (h ^ c) * 1099511628211ULL;
    }
};
// Everything that changes a sample's value or a pixel's owner, plus the scene's counts (not its contents); for an adaptive
// accumulator also everything that changes when a pixel stops, under a layout tag of its own.
uint64_t accum_fingerprint(const PrtScene* s, const PrtCamera& c, const PrtRenderParams& p, const PrtAdaptiveParams* ad = nullptr) {
    Fnv f;
    f.add((uint32_t)(ad ? 0x70727462u : 0x70727461u)); // layout tag of this hash
    f.add(c.width); f.add(c.height); f.add(c.fovy);
    for (int k = 0; k < 3; ++k) { f.add(c.eye[k]); f.add(c.look_at[k]); f.add(c.up[k]); }
    f.add(p.max_depth); f.add(p.russian_roulette); f.add((int32_t)(p.sample_lights ? 1 : 0)); f.add(p.precision);
    for (int k = 0; k < 3; ++k) f.add(p.background[k]);
    f.add(p.seed);
    f.add((int32_t)TileLayout(c, p).tile); f.add(p.rank); f.add(p.nranks); f.add((int32_t)(p.pixel_jitter ? 1 : 0));
    f.add((uint64_t)s->tris.size()); f.add((uint64_t)s->mesh_mat.size()); f.add((uint64_t)s->mats.size());
    if (ad) {
        f.add(ad->min_spp); f.add(ad->max_spp); f.add(ad->batch); f.add(ad->rel_tol); f.add(ad->abs_tol);
    }
    return f.h;
}
int not_adaptive(const PrtAccum* a, const char* who, const char* instead) {
    if (a && a->adaptive)
        return fail(PRT_E_INVALID, std::string(who) + ": an adaptive accumulator has per-pixel sample counts (use " + instead + ")");
    return PRT_OK;
}
// The accumulator's scene is uploaded, to the device the sums live on.
int accum_ready(PrtAccum* a, const char* who) {
    if (!a) return fail(PRT_E_INVALID, std::string(who) + ": null accumulator");
    int rc = require_uploaded(a->scene, who);
    if (rc) return rc;
    if (a->scene->device != a->device) return fail(PRT_E_INVALID, std::string(who) + ": the scene was uploaded to another device since the accumulator was created");
    return PRT_OK;
}
// Zeroed state of an accumulator (ad: adaptive, its batch already resolved and checked).
hipError_t accum_zero(PrtAccum* a) {
    const size_t npx = a->n / 3;
    hipError_t e = hipMemsetAsync(a->d_sum.get(), 0, a->n * sizeof(double), nullptr);
    if (e == hipSuccess && a->adaptive) e = hipMemsetAsync(a->d_moment.get(), 0, npx * sizeof(double), nullptr);
    if (e == hipSuccess && a->adaptive) e = hipMemsetAsync(a->d_count.get(), 0, npx * sizeof(uint32_t), nullptr);
    if (e == hipSuccess) e = hipEventRecord(a->done.get(), nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(a->done.get());
    return e;
}

int accum_create(const char* who, PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, const PrtAdaptiveParams* ad, PrtAccum** out) {
    const std::string w(who);
    if (!out) return fail(PRT_E_INVALID, w + ": null argument");
    *out = nullptr;
    int rc = require_uploaded(s, who);
    if (rc) return rc;
    if (!cam || !p) return fail(PRT_E_INVALID, w + ": null argument");
    if (cam->width < 1 || cam->height < 1) return fail(PRT_E_INVALID, w + ": bad image size");
    if (p->reserved != 0) return fail(PRT_E_INVALID, w + ": reserved must be 0");
    if (p->precision != PRT_PRECISION_F64 && p->precision != PRT_PRECISION_F32) return fail(PRT_E_INVALID, w + ": unsupported precision");
    if (p->nranks < 1 || p->rank < 0 || p->rank >= p->nranks) return fail(PRT_E_INVALID, w + ": bad rank/nranks");
    PrtAdaptiveParams A{};
    if (ad) {
        A = *ad;
        if (A.reserved != 0) return fail(PRT_E_INVALID, w + ": adaptive reserved must be 0");
        if (A.batch == 0) A.batch = PRT_ADAPTIVE_DEFAULT_BATCH;
        if (A.batch < 1) return fail(PRT_E_INVALID, w + ": batch must be >= 1 (or 0 for the default)");
        if (A.min_spp < 2 * (int64_t)A.batch || A.min_spp % A.batch)
            return fail(PRT_E_INVALID, w + ": min_spp must be a multiple of batch and >= 2 * batch");
        if (A.max_spp < A.min_spp || A.max_spp % A.batch) return fail(PRT_E_INVALID, w + ": max_spp must be a multiple of batch and >= min_spp");
        if (!std::isfinite(A.rel_tol) || A.rel_tol < 0 || !std::isfinite(A.abs_tol) || A.abs_tol < 0)
            return fail(PRT_E_INVALID, w + ": rel_tol and abs_tol must be finite and >= 0");
    }
    if (p->precision == PRT_PRECISION_F32 && (rc = ensure_f32(s))) return rc;
    PrtAccum* a = new (std::nothrow) PrtAccum();
    if (!a) return fail(PRT_E_OOM, w + ": out of host memory");
    a->scene = s;
    a->cam = *cam;
    a->params = *p;
    a->params.spp = 0; // the pass size is prt_accum_render's argument
    a->device = s->device;
    a->generation = s->generation;
    a->adaptive = ad != nullptr;
    a->ad = A;
    a->fingerprint = accum_fingerprint(s, *cam, *p, ad ? &A : nullptr);
    a->n = (size_t)cam->width * cam->height * 3;
    const size_t npx = a->n / 3;
    hipError_t e = dev_alloc(a->d_sum, a->n * sizeof(double));
    if (e == hipSuccess) e = make_event(a->done, hipEventDisableTiming);
    if (a->adaptive) {
        const uint64_t owned = TileLayout(*cam, *p).items_per_chunk;
        const size_t items = std::max<size_t>(1, owned), segs = std::max<uint32_t>(1, prt::adapt_segments(owned));
        if (e == hipSuccess) e = dev_alloc(a->d_moment, npx * sizeof(double));
        if (e == hipSuccess) e = dev_alloc(a->d_count, npx * sizeof(uint32_t));
        if (e == hipSuccess) e = dev_alloc(a->d_list, items * sizeof(int32_t));
        if (e == hipSuccess) e = dev_alloc(a->d_seg, segs * sizeof(uint32_t));
        if (e == hipSuccess) e = dev_alloc(a->d_active, sizeof(uint32_t));
        void* h = nullptr;
        if (e == hipSuccess && (e = hipHostMalloc(&h, sizeof(uint32_t), hipHostMallocDefault)) == hipSuccess)
            a->h_active.reset(static_cast<uint32_t*>(h));
    }
    if (e == hipSuccess) e = accum_zero(a);
    if (e != hipSuccess) {
        prt_accum_destroy(a);
        return hip_fail(w, e);
    }
    *out = a;
    return PRT_OK;
}
} // namespace

extern "C" {

int prt_accum_create(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, PrtAccum** out) {
    return accum_create("prt_accum_create", s, cam, p, nullptr, out);
}

int prt_accum_create_adaptive(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, const PrtAdaptiveParams* ad, PrtAccum** out) {
    if (!ad) {
        if (out) *out = nullptr;
        return fail(PRT_E_INVALID, "prt_accum_create_adaptive: null argument");
    }
    return accum_create("prt_accum_create_adaptive", s, cam, p, ad, out);
}

void prt_accum_destroy(PrtAccum* a) {
    if (!a) return;
    if (a->device >= 0) (void)hipSetDevice(a->device);
    if (a->done) (void)hipEventSynchronize(a->done.get()); // nothing is freed under a running pass
    delete a;
}

int prt_accum_render(PrtAccum* a, int32_t n_samples, void* stream) {
    int rc = accum_ready(a, "prt_accum_render");
    if (rc || (rc = not_adaptive(a, "prt_accum_render", "prt_accum_render_adaptive"))) return rc;
    if (n_samples < 1) return fail(PRT_E_INVALID, "prt_accum_render: n_samples must be >= 1");
    if (a->samples + (uint64_t)n_samples > (uint64_t)INT32_MAX)
        return fail(PRT_E_LIMIT, "prt_accum_render: sample indices would pass INT32_MAX");
    if (a->generation != a->scene->generation)
        return fail(PRT_E_INVALID, "prt_accum_render: the scene's vertices were updated since these sums were rendered (prt_accum_reset first)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PRT_HIP(hipStreamWaitEvent(st, a->done.get(), 0));
    RenderPass pass;
    pass.spp = n_samples;
    pass.first = (int32_t)a->samples;
    pass.d_sum = a->d_sum.get();
    if ((rc = render_impl(a->scene, "prt_accum_render", &a->cam, &a->params, pass, nullptr, nullptr, 0, st))) return rc;
    PRT_HIP(hipEventRecord(a->done.get(), st));
    a->samples += (uint64_t)n_samples;
    return PRT_OK;
}

int prt_accum_samples(const PrtAccum* a, uint64_t* n) {
    if (!a || !n) return fail(PRT_E_INVALID, "prt_accum_samples: null argument");
    *n = a->samples;
    return PRT_OK;
}

int prt_accum_reset(PrtAccum* a) {
    int rc = accum_ready(a, "prt_accum_reset");
    if (rc) return rc;
    PRT_HIP(hipEventSynchronize(a->done.get()));
    PRT_HIP(accum_zero(a));
    a->samples = 0;
    a->generation = a->scene->generation;
    a->feat_valid = false; // the denoiser's features are retraced on the next use
    return PRT_OK;
}

int prt_accum_resolve(PrtAccum* a, void* d_rgb_f64, void* d_rgb_f32, void* d_rgb_u8, void* stream) {
    int rc = accum_ready(a, "prt_accum_resolve");
    if (rc) return rc;
    if (!d_rgb_f64 && !d_rgb_f32 && !d_rgb_u8) return fail(PRT_E_INVALID, "prt_accum_resolve: no output buffer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PRT_HIP(hipStreamWaitEvent(st, a->done.get(), 0));
    prt::launch_resolve(a->d_sum.get(), a->n, a->samples, a->adaptive ? a->d_count.get() : nullptr, static_cast<double*>(d_rgb_f64),
                        static_cast<float*>(d_rgb_f32), static_cast<uint8_t*>(d_rgb_u8), st);
    PRT_HIP(hipGetLastError());
    PRT_HIP(hipEventRecord(a->done.get(), st));
    return PRT_OK;
}

int prt_accum_read(PrtAccum* a, double* rgb_f64, float* rgb_f32) {
    int rc = accum_ready(a, "prt_accum_read");
    if (rc) return rc;
    if (!rgb_f64 && !rgb_f32) return fail(PRT_E_INVALID, "prt_accum_read: no output buffer");
    Staging b;
    void* d64 = rgb_f64 ? b.out(a->n * sizeof(double)) : nullptr;
    void* d32 = rgb_f32 ? b.out(a->n * sizeof(float)) : nullptr;
    if ((rc = b.status("prt_accum_read")) || (rc = prt_accum_resolve(a, d64, d32, nullptr, nullptr))) return rc;
    b.sync(a->done.get());
    if (rgb_f64) b.down(rgb_f64, d64, a->n * sizeof(double));
    if (rgb_f32) b.down(rgb_f32, d32, a->n * sizeof(float));
    return b.status("prt_accum_read");
}

int prt_accum_export(const PrtAccum* a, double* sums, uint64_t* samples, uint64_t* fingerprint) {
    if (!a || !sums || !samples || !fingerprint) return fail(PRT_E_INVALID, "prt_accum_export: null argument");
    if (int rc = not_adaptive(a, "prt_accum_export", "prt_accum_export_adaptive")) return rc;
    PRT_HIP(hipSetDevice(a->device));
    PRT_HIP(hipEventSynchronize(a->done.get()));
    PRT_HIP(hipMemcpy(sums, a->d_sum.get(), a->n * sizeof(double), hipMemcpyDeviceToHost));
    *samples = a->samples;
    *fingerprint = a->fingerprint;
    return PRT_OK;
}

int prt_accum_import(PrtAccum* a, const double* sums, uint64_t samples, uint64_t fingerprint) {
    int rc = accum_ready(a, "prt_accum_import");
    if (rc || (rc = not_adaptive(a, "prt_accum_import", "prt_accum_import_adaptive"))) return rc;
    if (!sums) return fail(PRT_E_INVALID, "prt_accum_import: null argument");
    if (fingerprint != a->fingerprint)
        return fail(PRT_E_INVALID, "prt_accum_import: fingerprint mismatch (other camera, render parameters or scene counts)");
    if (samples > (uint64_t)INT32_MAX) return fail(PRT_E_LIMIT, "prt_accum_import: more than INT32_MAX samples");
    PRT_HIP(hipEventSynchronize(a->done.get()));
    PRT_HIP(hipMemcpy(a->d_sum.get(), sums, a->n * sizeof(double), hipMemcpyHostToDevice));
    a->samples = samples;
    a->generation = a->scene->generation;
    return PRT_OK;
}

int prt_accum_render_adaptive(PrtAccum* a, int32_t n_samples, uint64_t* n_active, void* stream) {
    const char* who = "prt_accum_render_adaptive";
    int rc = accum_ready(a, who);
    if (rc) return rc;
    if (!n_active) return fail(PRT_E_INVALID, "prt_accum_render_adaptive: null argument");
    *n_active = 0;
    if (!a->adaptive) return fail(PRT_E_INVALID, "prt_accum_render_adaptive: not an adaptive accumulator (prt_accum_create_adaptive)");
    const PrtAdaptiveParams& A = a->ad;
    if (n_samples < 1 || n_samples % A.batch) return fail(PRT_E_INVALID, "prt_accum_render_adaptive: n_samples must be a positive multiple of batch");
    if (a->generation != a->scene->generation)
        return fail(PRT_E_INVALID, "prt_accum_render_adaptive: the scene's vertices were updated since these sums were rendered (prt_accum_reset first)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PRT_HIP(hipStreamWaitEvent(st, a->done.get(), 0));
    // (1) + (2): the active pixels, listed on the device; their number is the one value a round reads back
    DCamera C; // (the select maps owned item oi to its pixel as K3 does: the camera and the tile layout are what it reads)
    prt::setup_camera(a->cam, C);
    DRenderParams P;
    std::memset(&P, 0, sizeof(P));
    TileLayout(a->cam, a->params).set(P);
    DAdaptRule R;
    R.n = (uint32_t)a->samples;
    R.min_spp = (uint32_t)A.min_spp;
    R.max_spp = (uint32_t)A.max_spp;
    R.batch = (uint32_t)A.batch;
    R.rel_tol = A.rel_tol;
    R.abs_tol = A.abs_tol;
    prt::launch_adapt_select(C, P, R, a->d_sum.get(), a->d_moment.get(), a->d_count.get(), a->d_seg.get(), a->d_list.get(), a->d_active.get(), st);
    PRT_HIP(hipGetLastError());
    PRT_HIP(hipMemcpyAsync(a->h_active.get(), a->d_active.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PRT_HIP(hipStreamSynchronize(st));
    const uint32_t listed = *a->h_active;
    if (listed > P.items_per_chunk) return fail(PRT_E_HIP, "prt_accum_render_adaptive: the select listed more pixels than are owned");
    if (listed == 0) {
        PRT_HIP(hipEventRecord(a->done.get(), st));
        return PRT_OK;
    }
    // (3) + (4): samples [n, n + k) of the listed pixels, at most PRT_MAX_CHUNKS batches per launch
    const int64_t k = std::min<int64_t>(n_samples, (int64_t)A.max_spp - (int64_t)a->samples);
    const int64_t per_launch = (int64_t)PRT_MAX_CHUNKS * A.batch;
    for (int64_t s0 = 0; s0 < k; s0 += per_launch) {
        RenderPass pass;
        pass.spp = (int)std::min<int64_t>(per_launch, k - s0);
        pass.first = (int32_t)(a->samples + s0);
        pass.d_sum = a->d_sum.get();
        pass.d_list = a->d_list.get();
        pass.list_n = listed;
        pass.batch = A.batch;
        pass.d_moment = a->d_moment.get();
        pass.d_count = a->d_count.get();
        if ((rc = render_impl(a->scene, who, &a->cam, &a->params, pass, nullptr, nullptr, 0, st))) return rc;
    }
    PRT_HIP(hipEventRecord(a->done.get(), st));
    a->samples += (uint64_t)k;
    *n_active = listed;
    return PRT_OK;
}

int prt_accum_pixel_samples(PrtAccum* a, uint32_t* counts) {
    int rc = accum_ready(a, "prt_accum_pixel_samples");
    if (rc) return rc;
    if (!counts) return fail(PRT_E_INVALID, "prt_accum_pixel_samples: null argument");
    PRT_HIP(hipEventSynchronize(a->done.get()));
    if (a->adaptive) {
        PRT_HIP(hipMemcpy(counts, a->d_count.get(), a->n / 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    } else { // every owned pixel has every sample
        const TileLayout L(a->cam, a->params);
        for (int y = 0; y < L.height; ++y)
            for (int x = 0; x < L.width; ++x) counts[(size_t)y * L.width + x] = L.owns(x, y) ? (uint32_t)a->samples : 0u;
    }
    return PRT_OK;
}

int prt_accum_export_adaptive(const PrtAccum* a, double* sums, double* moments, uint32_t* counts, uint64_t* samples,
                              uint64_t* fingerprint) {
    if (!a || !sums || !moments || !counts || !samples || !fingerprint) return fail(PRT_E_INVALID, "prt_accum_export_adaptive: null argument");
    if (!a->adaptive) return fail(PRT_E_INVALID, "prt_accum_export_adaptive: not an adaptive accumulator (prt_accum_export)");
    PRT_HIP(hipSetDevice(a->device));
    PRT_HIP(hipEventSynchronize(a->done.get()));
    PRT_HIP(hipMemcpy(sums, a->d_sum.get(), a->n * sizeof(double), hipMemcpyDeviceToHost));
    PRT_HIP(hipMemcpy(moments, a->d_moment.get(), a->n / 3 * sizeof(double), hipMemcpyDeviceToHost));
    PRT_HIP(hipMemcpy(counts, a->d_count.get(), a->n / 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *samples = a->samples;
    *fingerprint = a->fingerprint;
    return PRT_OK;
}

int prt_accum_import_adaptive(PrtAccum* a, const double* sums, const double* moments, const uint32_t* counts, uint64_t samples,
                              uint64_t fingerprint) {
    int rc = accum_ready(a, "prt_accum_import_adaptive");
    if (rc) return rc;
    if (!sums || !moments || !counts) return fail(PRT_E_INVALID, "prt_accum_import_adaptive: null argument");
    if (!a->adaptive) return fail(PRT_E_INVALID, "prt_accum_import_adaptive: not an adaptive accumulator (prt_accum_import)");
    if (fingerprint != a->fingerprint)
        return fail(PRT_E_INVALID, "prt_accum_import_adaptive: fingerprint mismatch (other camera, render or adaptive parameters, or scene counts)");
    if (samples > (uint64_t)INT32_MAX) return fail(PRT_E_LIMIT, "prt_accum_import_adaptive: more than INT32_MAX samples");
    if (samples > (uint64_t)a->ad.max_spp || samples % (uint64_t)a->ad.batch)
        return fail(PRT_E_INVALID, "prt_accum_import_adaptive: samples must be a multiple of batch and <= max_spp");
    const TileLayout L(a->cam, a->params);
    for (size_t i = 0; i < a->n / 3; ++i) {
        if (counts[i] > samples || counts[i] % (uint32_t)a->ad.batch)
            return fail(PRT_E_INVALID, "prt_accum_import_adaptive: a count above samples or not a multiple of batch");
        if (counts[i] && !L.owns((int)(i % L.width), (int)(i / L.width))) return fail(PRT_E_INVALID, "prt_accum_import_adaptive: samples on a pixel this rank does not own");
        if (!std::isfinite(moments[i]) || moments[i] < 0) return fail(PRT_E_INVALID, "prt_accum_import_adaptive: a negative or non-finite moment");
    }
    PRT_HIP(hipEventSynchronize(a->done.get()));
    PRT_HIP(hipMemcpy(a->d_sum.get(), sums, a->n * sizeof(double), hipMemcpyHostToDevice));
    PRT_HIP(hipMemcpy(a->d_moment.get(), moments, a->n / 3 * sizeof(double), hipMemcpyHostToDevice));
    PRT_HIP(hipMemcpy(a->d_count.get(), counts, a->n / 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
    a->samples = samples;
    a->generation = a->scene->generation;
    return PRT_OK;
}

int prt_tonemap_srgb8(PrtScene* s, const void* d_rgb_f32, int width, int height, void* d_rgb_u8, void* stream) {
    int rc = require_uploaded(s, "prt_tonemap_srgb8");
    if (rc) return rc;
    if (!d_rgb_f32 || !d_rgb_u8 || width < 1 || height < 1) return fail(PRT_E_INVALID, "prt_tonemap_srgb8: bad argument");
    prt::launch_tonemap(static_cast<const float*>(d_rgb_f32), (size_t)width * height * 3, static_cast<uint8_t*>(d_rgb_u8),
                        reinterpret_cast<hipStream_t>(stream));
    PRT_HIP(hipGetLastError());
    return PRT_OK;
}

// ------------------------------------------------------------------------------------------- features + denoiser
void prt_denoise_defaults(PrtDenoiseParams* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    // measured: tools/denoise_timing.py, DESIGN.md §7 (the best point of its 16-spp sweep over cornell-box, veach-mis and bathroom2)
    p->iterations = 4;
    p->demodulate = 1;
    p->sigma_color = 0.5f;
    p->sigma_normal = 0.2f;
    p->sigma_depth = 0.1f;
    p->sigma_albedo = 0.1f;
    p->feature_spp = 1;
    p->reserved = 0;
}

void prt_denoise_guided_defaults(PrtDenoiseParams* p) {
    if (!p) return;
    prt_denoise_defaults(p);
    // measured: tools/denoise_guided_timing.py, DESIGN.md §7 (the best point of its sweep around SVGF's published sigma_l = 4 and
    // five levels, by mean log relMSE over cornell-box, veach-mis and bathroom2 at 16 and 64 spp)
    p->iterations = 4;
    p->sigma_color = 8.0f;
}

} // extern "C"

namespace {
int check_denoise_params(const PrtDenoiseParams* p, const std::string& w) {
    if (!p) return fail(PRT_E_INVALID, w + ": null denoise params");
    if (p->reserved != 0) return fail(PRT_E_INVALID, w + ": reserved must be 0");
    if (p->iterations < 0 || p->iterations > 10) return fail(PRT_E_INVALID, w + ": iterations must be in 0..10");
    if (p->demodulate != 0 && p->demodulate != 1) return fail(PRT_E_INVALID, w + ": demodulate must be 0 or 1");
    if (std::isnan(p->sigma_color) || std::isnan(p->sigma_normal) || std::isnan(p->sigma_depth) || std::isnan(p->sigma_albedo))
        return fail(PRT_E_INVALID, w + ": a sigma is NaN");
    if (p->feature_spp < 1) return fail(PRT_E_INVALID, w + ": feature_spp must be >= 1");
    return PRT_OK;
}

// k_features on the scene's fp64 tables (the tree K1 traverses).
int features_impl(PrtScene* s, const std::string& w, const PrtCamera* cam, const PrtRenderParams* p, int32_t feature_spp, float* albedo,
                  float* normal, float* depth, int32_t* prim, hipStream_t st) {
    if (!cam || !p) return fail(PRT_E_INVALID, w + ": null argument");
    if (cam->width < 1 || cam->height < 1) return fail(PRT_E_INVALID, w + ": bad image size");
    if ((uint64_t)cam->width * (uint64_t)cam->height >= (1ull << 31)) return fail(PRT_E_LIMIT, w + ": more than 2^31 pixels");
    if (feature_spp < 1) return fail(PRT_E_INVALID, w + ": feature_spp must be >= 1");
    if (!albedo && !normal && !depth && !prim) return fail(PRT_E_INVALID, w + ": no output buffer");
    DCamera C;
    prt::setup_camera(*cam, C);
    PRT_HIP(s->after_refit(st));
    prt::launch_features(s->k64.d, C, prt::seed_key(p->seed), p->pixel_jitter ? 1 : 0, feature_spp, albedo, normal, depth, prim, st);
    PRT_HIP(hipGetLastError());
    if (!s->feat_done) PRT_HIP(make_event(s->feat_done, hipEventDisableTiming));
    PRT_HIP(hipEventRecord(s->feat_done.get(), st)); // a refit's writing phase waits for this reader too
    s->feat_pending = true;
    return PRT_OK;
}

// What either form of the filter asks of its arguments, host or device pointers alike.  guided: the variance-guided form,
// with `variance` in and `out_variance` (may be null) out; both are null for the plain filter.
int check_denoise_args(const std::string& w, int32_t W, int32_t H, const void* rgb, const void* variance, const void* albedo,
                       const void* normal, const void* depth, const PrtDenoiseParams* p, const void* out, const void* out_variance,
                       bool guided) {
    int rc = check_denoise_params(p, w);
    if (rc) return rc;
    if (W < 1 || H < 1) return fail(PRT_E_INVALID, w + ": bad image size");
    if ((uint64_t)W * (uint64_t)H >= (1ull << 31)) return fail(PRT_E_LIMIT, w + ": more than 2^31 pixels");
    if (!rgb || !albedo || !normal || !depth || !out || (guided && !variance)) return fail(PRT_E_INVALID, w + ": null buffer");
    if (guided)
        for (const void* in : {rgb, variance, albedo, normal, depth})
            if (in == out || in == out_variance) return fail(PRT_E_INVALID, w + ": an output buffer aliases an input");
    return PRT_OK;
}

// The filter on device buffers through the scene's scratch; the arguments have passed check_denoise_args.
int denoise_run(PrtScene* s, const std::string& w, int32_t W, int32_t H, const void* rgb, const void* variance, const void* albedo,
                const void* normal, const void* depth, const PrtDenoiseParams* p, void* out, void* out_variance, bool guided,
                hipStream_t st) {
    const size_t npx = (size_t)W * H;
    if (p->iterations == 0) PRT_HIP(hipMemcpyAsync(out, rgb, npx * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (p->iterations == 0 && !guided) return PRT_OK;
    if (p->iterations > 0) PRT_HIP_AS(w, s->dn.reserve(prt::denoise_scratch_bytes(W, H), st));
    const float sigma[4] = {p->sigma_color, p->sigma_normal, p->sigma_depth, p->sigma_albedo};
    if (guided)
        prt::launch_denoise_guided(W, H, static_cast<const float*>(rgb), static_cast<const float*>(variance), static_cast<const float*>(albedo),
                                   static_cast<const float*>(normal), static_cast<const float*>(depth), p->iterations, p->demodulate, sigma,
                                   s->dn.get<void>(), static_cast<float*>(out), static_cast<float*>(out_variance), st);
    else
        prt::launch_denoise(W, H, static_cast<const float*>(rgb), static_cast<const float*>(albedo), static_cast<const float*>(normal),
                            static_cast<const float*>(depth), p->iterations, p->demodulate, sigma, s->dn.get<void>(), static_cast<float*>(out), st);
    PRT_HIP(hipGetLastError());
    if (p->iterations > 0) PRT_HIP(s->dn.used(st));
    return PRT_OK;
}

int denoise_impl(PrtScene* s, const std::string& w, int32_t W, int32_t H, const void* rgb, const void* variance, const void* albedo,
                 const void* normal, const void* depth, const PrtDenoiseParams* p, void* out, void* out_variance, bool guided,
                 hipStream_t st) {
    int rc = check_denoise_args(w, W, H, rgb, variance, albedo, normal, depth, p, out, out_variance, guided);
    return rc ? rc : denoise_run(s, w, W, H, rgb, variance, albedo, normal, depth, p, out, out_variance, guided, st);
}

// prt_denoise / prt_denoise_guided: the filter on host buffers, staged through the device.
int denoise_host(PrtScene* s, const std::string& who, int32_t w, int32_t h, const float* rgb, const float* variance, const float* albedo,
                 const float* normal, const float* depth, const PrtDenoiseParams* p, float* out, float* out_variance, bool guided) {
    int rc = require_uploaded(s, who.c_str());
    if (rc) return rc;
    if ((rc = check_denoise_args(who, w, h, rgb, variance, albedo, normal, depth, p, out, out_variance, guided))) return rc;
    const size_t npx = (size_t)w * h, b3 = npx * 3 * sizeof(float), b1 = npx * sizeof(float);
    Staging b;
    void* dc = b.in(rgb, b3);
    void* dv = guided ? b.in(variance, b1) : nullptr;
    void* da = b.in(albedo, b3);
    void* dn = b.in(normal, b3);
    void* dz = b.in(depth, b1);
    void* dout = b.out(b3);
    void* dvout = out_variance ? b.out(b1) : nullptr;
    if ((rc = b.status(who)) || (rc = denoise_run(s, who, w, h, dc, dv, da, dn, dz, p, dout, dvout, guided, nullptr))) return rc;
    b.sync();
    b.down(out, dout, b3);
    if (out_variance) b.down(out_variance, dvout, b1);
    return b.status(who);
}

// What the variance of an accumulator needs: the moments of an adaptive one, and two batches in every rendered pixel
// (min_spp >= 2 * batch, and the running pixels share the global count).
int accum_variance_ready(const PrtAccum* a, const std::string& w) {
    if (!a->adaptive) return fail(PRT_E_INVALID, w + ": a plain accumulator keeps no moments (use an adaptive one; min_spp == max_spp samples uniformly)");
    if (a->samples < 2 * (uint64_t)a->ad.batch) return fail(PRT_E_INVALID, w + ": fewer than two batches of samples so far");
    return PRT_OK;
}

// prt_accum_resolve_denoised[_guided]: the accumulator's fp32 frame (and, guided, its variance) through the filter, with
// the cached features.
int accum_resolve_denoised_impl(PrtAccum* a, const std::string& w, const PrtDenoiseParams* p, void* d_rgb_f32, void* d_rgb_u8, void* stream,
                                bool guided) {
    int rc = accum_ready(a, w.c_str());
    if (rc || (rc = check_denoise_params(p, w))) return rc;
    if (a->params.nranks > 1) return fail(PRT_E_INVALID, w + ": nranks > 1 (a tile share lacks its neighbours' pixels)");
    if (!d_rgb_f32 && !d_rgb_u8) return fail(PRT_E_INVALID, w + ": no output buffer");
    const size_t npx = a->n / 3;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (guided && (rc = accum_variance_ready(a, w))) return rc;
    PRT_HIP(hipStreamWaitEvent(st, a->done.get(), 0));
    if (guided) {
        if (!a->d_var32) PRT_HIP(dev_alloc(a->d_var32, npx * sizeof(float)));
        prt::launch_accum_variance(a->d_sum.get(), a->d_moment.get(), a->d_count.get(), npx, (uint32_t)a->ad.batch, a->d_var32.get(), st);
        PRT_HIP(hipGetLastError());
    }
    if (!a->d_feat) PRT_HIP(dev_alloc(a->d_feat, npx * 7 * sizeof(float)));
    if (!a->d_res32) PRT_HIP(dev_alloc(a->d_res32, a->n * sizeof(float)));
    if (!d_rgb_f32 && !a->d_dn32) PRT_HIP(dev_alloc(a->d_dn32, a->n * sizeof(float)));
    float* alb = a->d_feat.get();
    float* nrm = alb + a->n;
    float* dep = nrm + a->n;
    if (!a->feat_valid || a->feat_gen != a->scene->generation || a->feat_spp != p->feature_spp) {
        a->feat_valid = false;
        if ((rc = features_impl(a->scene, w, &a->cam, &a->params, p->feature_spp, alb, nrm, dep, nullptr, st))) return rc;
        a->feat_valid = true;
        a->feat_gen = a->scene->generation;
        a->feat_spp = p->feature_spp;
    }
    prt::launch_resolve(a->d_sum.get(), a->n, a->samples, a->adaptive ? a->d_count.get() : nullptr, nullptr, a->d_res32.get(), nullptr, st);
    PRT_HIP(hipGetLastError());
    float* out = d_rgb_f32 ? static_cast<float*>(d_rgb_f32) : a->d_dn32.get();
    if ((rc = denoise_impl(a->scene, w, a->cam.width, a->cam.height, a->d_res32.get(), guided ? a->d_var32.get() : nullptr, alb, nrm, dep, p,
                           out, nullptr, guided, st)))
        return rc;
    if (d_rgb_u8) {
        prt::launch_tonemap(out, a->n, static_cast<uint8_t*>(d_rgb_u8), st);
        PRT_HIP(hipGetLastError());
    }
    PRT_HIP(hipEventRecord(a->done.get(), st));
    return PRT_OK;
}

int accum_read_denoised_impl(PrtAccum* a, const std::string& w, const PrtDenoiseParams* p, float* rgb_f32, bool guided) {
    int rc = accum_ready(a, w.c_str());
    if (rc) return rc;
    if (!rgb_f32) return fail(PRT_E_INVALID, w + ": no output buffer");
    Staging b;
    void* d = b.out(a->n * sizeof(float));
    if ((rc = b.status(w)) || (rc = accum_resolve_denoised_impl(a, w, p, d, nullptr, nullptr, guided))) return rc;
    b.sync(a->done.get());
    b.down(rgb_f32, d, a->n * sizeof(float));
    return b.status(w);
}

} // namespace

extern "C" {

int prt_render_features_device(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, int32_t feature_spp, void* d_albedo,
                               void* d_normal, void* d_depth, void* d_prim, void* stream) {
    int rc = require_uploaded(s, "prt_render_features_device");
    if (rc) return rc;
    return features_impl(s, "prt_render_features_device", cam, p, feature_spp, static_cast<float*>(d_albedo), static_cast<float*>(d_normal),
                         static_cast<float*>(d_depth), static_cast<int32_t*>(d_prim), reinterpret_cast<hipStream_t>(stream));
}

int prt_render_features(PrtScene* s, const PrtCamera* cam, const PrtRenderParams* p, int32_t feature_spp, float* albedo, float* normal,
                        float* depth, int32_t* prim) {
    const std::string w = "prt_render_features";
    int rc = require_uploaded(s, w.c_str());
    if (rc) return rc;
    if (!cam || cam->width < 1 || cam->height < 1) return features_impl(s, w, cam, p, feature_spp, albedo, normal, depth, prim, nullptr);
    const size_t npx = (size_t)cam->width * cam->height;
    Staging b;
    void* da = albedo ? b.out(npx * 3 * sizeof(float)) : nullptr;
    void* dn = normal ? b.out(npx * 3 * sizeof(float)) : nullptr;
    void* dz = depth ? b.out(npx * sizeof(float)) : nullptr;
    void* dp = prim ? b.out(npx * sizeof(int32_t)) : nullptr;
    if ((rc = b.status(w)) || (rc = features_impl(s, w, cam, p, feature_spp, static_cast<float*>(da), static_cast<float*>(dn),
                                                  static_cast<float*>(dz), static_cast<int32_t*>(dp), nullptr)))
        return rc;
    b.sync();
    if (albedo) b.down(albedo, da, npx * 3 * sizeof(float));
    if (normal) b.down(normal, dn, npx * 3 * sizeof(float));
    if (depth) b.down(depth, dz, npx * sizeof(float));
    if (prim) b.down(prim, dp, npx * sizeof(int32_t));
    return b.status(w);
}

int prt_denoise_device(PrtScene* s, int32_t w, int32_t h, const void* d_rgb, const void* d_albedo, const void* d_normal,
                       const void* d_depth, const PrtDenoiseParams* p, void* d_out, void* stream) {
    int rc = require_uploaded(s, "prt_denoise_device");
    if (rc) return rc;
    return denoise_impl(s, "prt_denoise_device", w, h, d_rgb, nullptr, d_albedo, d_normal, d_depth, p, d_out, nullptr, false,
                        reinterpret_cast<hipStream_t>(stream));
}

int prt_denoise_guided_device(PrtScene* s, int32_t w, int32_t h, const void* d_rgb, const void* d_variance, const void* d_albedo,
                              const void* d_normal, const void* d_depth, const PrtDenoiseParams* p, void* d_out, void* d_out_variance,
                              void* stream) {
    int rc = require_uploaded(s, "prt_denoise_guided_device");
    if (rc) return rc;
    return denoise_impl(s, "prt_denoise_guided_device", w, h, d_rgb, d_variance, d_albedo, d_normal, d_depth, p, d_out, d_out_variance, true,
                        reinterpret_cast<hipStream_t>(stream));
}

int prt_denoise(PrtScene* s, int32_t w, int32_t h, const float* rgb, const float* albedo, const float* normal, const float* depth,
                const PrtDenoiseParams* p, float* out) {
    return denoise_host(s, "prt_denoise", w, h, rgb, nullptr, albedo, normal, depth, p, out, nullptr, false);
}

int prt_denoise_guided(PrtScene* s, int32_t w, int32_t h, const float* rgb, const float* variance, const float* albedo,
                       const float* normal, const float* depth, const PrtDenoiseParams* p, float* out, float* out_variance) {
    return denoise_host(s, "prt_denoise_guided", w, h, rgb, variance, albedo, normal, depth, p, out, out_variance, true);
}

int prt_accum_variance(PrtAccum* a, void* d_var_f32, void* stream) {
    const std::string w = "prt_accum_variance";
    int rc = accum_ready(a, w.c_str());
    if (rc) return rc;
    if ((rc = accum_variance_ready(a, w))) return rc;
    if (!d_var_f32) return fail(PRT_E_INVALID, w + ": no output buffer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PRT_HIP(hipStreamWaitEvent(st, a->done.get(), 0));
    prt::launch_accum_variance(a->d_sum.get(), a->d_moment.get(), a->d_count.get(), a->n / 3, (uint32_t)a->ad.batch,
                               static_cast<float*>(d_var_f32), st);
    PRT_HIP(hipGetLastError());
    PRT_HIP(hipEventRecord(a->done.get(), st));
    return PRT_OK;
}

int prt_accum_read_variance(PrtAccum* a, float* var_f32) {
    const std::string w = "prt_accum_read_variance";
    int rc = accum_ready(a, w.c_str());
    if (rc) return rc;
    if (!var_f32) return fail(PRT_E_INVALID, w + ": no output buffer");
    Staging b;
    void* d = b.out(a->n / 3 * sizeof(float));
    if ((rc = b.status(w)) || (rc = prt_accum_variance(a, d, nullptr))) return rc;
    b.sync(a->done.get());
    b.down(var_f32, d, a->n / 3 * sizeof(float));
    return b.status(w);
}

int prt_accum_resolve_denoised(PrtAccum* a, const PrtDenoiseParams* p, void* d_rgb_f32, void* d_rgb_u8, void* stream) {
    return accum_resolve_denoised_impl(a, "prt_accum_resolve_denoised", p, d_rgb_f32, d_rgb_u8, stream, false);
}

int prt_accum_read_denoised(PrtAccum* a, const PrtDenoiseParams* p, float* rgb_f32) {
    return accum_read_denoised_impl(a, "prt_accum_read_denoised", p, rgb_f32, false);
}

int prt_accum_resolve_denoised_guided(PrtAccum* a, const PrtDenoiseParams* p, void* d_rgb_f32, void* d_rgb_u8, void* stream) {
    return accum_resolve_denoised_impl(a, "prt_accum_resolve_denoised_guided", p, d_rgb_f32, d_rgb_u8, stream, true);
}

int prt_accum_read_denoised_guided(PrtAccum* a, const PrtDenoiseParams* p, float* rgb_f32) {
    return accum_read_denoised_impl(a, "prt_accum_read_denoised_guided", p, rgb_f32, true);
}

} // extern "C"
