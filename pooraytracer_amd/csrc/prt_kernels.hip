// prt_kernels.hip — gfx950 kernels of the path-tracing hot path and their launchers.
//
//   K1 k_trace           closest hit / any hit for a ray batch     (world.Hit, BVH.cpp:51-61)
//      k_trace_surface   closest hit with the whole HitRecord and the material's response (PrtSurface)
//   K3 k_render          persistent-wavefront path tracer          (Camera::Render/RayColor, Camera.cpp:21-204)
//   K5 k_finalize        ordered sum of per-chunk partial sums -> f64 / f32 framebuffer
//      k_finalize_rays   the same sum per ray of a batch           (prt_ray_color)
//      k_sample_lights   lights.Sample test hook                   (BVH.cpp:62-67,86-100)
//      k_tonemap         NaN scrub + sRGB + clamp -> u8            (Camera.cpp:206-221,279-301)
//
// K3 design (MI355X: 256 CUs x 4 SIMD, wave64, 160 KB LDS/CU, per-XCD L2):
//   * persistent workgroups (grid = CUs x resident blocks); every LANE owns one work item =
//     (pixel, sample chunk) and pulls the next one from one of 16 global atomic counters when it finishes, so
//     short paths (light / background pixels) never idle a wave for long — lane-level regeneration
//     instead of a per-bounce compaction pass;
//   * traversal is resumable per lane (Trav::step = one node visit or one leaf).  A wave steps all
//     its traversing lanes together and leaves the stepping loop as soon as only PRT_K3_KEEP of them
//     are still busy (ballot + popcount); the finished lanes consume their hit (shade / NEE set-up /
//     Russian roulette / Scatter / next sample / next item) and start their next ray — continuation
//     or shadow, whichever that path needs — while the others keep their stack and resume.  Lanes
//     never wait for the slowest ray of the wave, and there is a single traversal call site;
//     shadow rays are any-hit rays over [0.001, dist - 0.001] (what Camera.cpp:150-155's test amounts to);
//   * the camera ray of a pixel is traced once per work item; every sample starts from its parked hit;
//   * traversal stack in LDS, lane-strided (conflict-free), PRT_STACK_DEPTH entries per lane;
//   * results are deterministic: per-sample keyed RNG, per-item partial sums combined in a fixed
//     order by K5 (no float atomics on the framebuffer).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/prt.h"
#include "prt_device.h"
#include "prt_launch.h"

// This file is compiled twice: as it stands (fp64, the reference's arithmetic: namespace prt, every kernel) and through
// prt_kernels_f32.hip with PRT_REAL = float (the fp32 fast mode: namespace prt32, K1 and K3 only — K5, the tone map and
// the test hooks work on fp64 buffers in either mode and exist once).
#ifndef PRT_F32_TU
#define PRT_F32_TU 0
#endif
#if PRT_F32_TU
#define PRT_NS prt32
#else
#define PRT_NS prt
#endif
#define PRT_DYN_STACK PRT_F32_TU // K3's traversal stacks in dynamic LDS, sized per launch from what the scene's tree can need (DRenderParams::stack_depth): the fp32 kernels, which have the registers for a fourth block per CU; the fp64 kernels are register-limited to three and keep static PRT_STACK_DEPTH-entry stacks (a run-time depth cost them 1.2 %)

// minimum resident waves per SIMD the register allocator must leave room for in K3
#ifndef PRT_RENDER_WAVES
#define PRT_RENDER_WAVES 2
#endif
#ifndef PRT_RENDER_WAVES_LEAN
#define PRT_RENDER_WAVES_LEAN 3 // the lean material permutation fits one more wave per SIMD
#endif
#ifndef PRT_RENDER_WAVES_TEX
#define PRT_RENDER_WAVES_TEX 3  // Lambertian / mirror / light + image textures (bathroom2-class scenes)
#endif
#ifndef PRT_RENDER_WAVES_PHONG
#define PRT_RENDER_WAVES_PHONG 3 // PhoneReflectance without textures (veach-mis-class scenes): fits since round 3 (168 registers); pays since round 4 (the light tables freed the LDS the third block needs)
#endif
#ifndef PRT_F32_WAVES
#define PRT_F32_WAVES 3 // fp32 fast mode: resident waves per SIMD of every K3 permutation
#endif
constexpr int render_waves(int feat_with_extra) {
    const int feat = feat_with_extra & PRT_FEAT_ALL; // (PRT_FEAT_EXTRA and PRT_FEAT_RAYS are not material features)
    if (PRT_F32_TU) return PRT_F32_WAVES;
    return feat == 0 ? PRT_RENDER_WAVES_LEAN
         : feat == PRT_FEAT_TEX ? PRT_RENDER_WAVES_TEX
         : feat == PRT_FEAT_PHONG ? PRT_RENDER_WAVES_PHONG
         : PRT_RENDER_WAVES;
}
// The stepping loop of a wave runs while MORE than this many lanes are still traversing; below it the
// finished lanes are handed new rays (K1) / shaded and re-armed (K3).
// (PRT_K1_KEEP and PRT_K1_CHUNK: prt_wave.h)
#ifndef PRT_K3_KEEP
#define PRT_K3_KEEP 24
#endif
#ifndef PRT_K1_WAVES
#define PRT_K1_WAVES 4 // resident waves per SIMD the K1 register allocation leaves room for
#endif

namespace {

#ifndef PRT_K3_PROFILE
#define PRT_K3_PROFILE 0 // developer diagnostic (COUNT instantiation): shader-clock cycles per section of the wave loop, folded into the counters
#endif
#if PRT_K3_PROFILE
#define PROF_MARK(k) do { if (COUNT) { const unsigned long long t_ = __builtin_readcyclecounter(); prof_[k] += t_ - prof_t_; prof_t_ = t_; } } while (0)
#else
#define PROF_MARK(k) do { } while (0)
#endif
// ------------------------------------------------------------------------------------------- K1
// Persistent waves; every lane pulls its next ray from a global counter the moment its traversal
// ends.  The stepping loop is left (and the finished lanes refilled) once no more than
// PRT_K1_KEEP lanes are still traversing.
// ANY = false is the closest-hit batch (one PrtHit per ray; counter rays_closest).  ANY = true is its any-hit form (K1o):
// is some triangle accepted in the ray's [tmin, tmax]?  The traversal ends at the first accepted triangle (Trav's any-hit
// mode, K3's shadow rays) and the write-out is ONE byte per ray — no normal fetch, no barycentrics, no S.shade lookup
// (counter rays_shadow; PRT_K1O_KEEP / PRT_K1O_WAVES, K1's values unless set).  The byte equals (prim >= 0) of the
// closest-hit kernel for the same ray: a triangle is accepted by the same test against the same interval in either
// form, the box tests only ever cull what cannot be accepted, and an exact tie cannot change a boolean.
#ifndef PRT_K1O_KEEP
#define PRT_K1O_KEEP PRT_K1_KEEP
#endif
#ifndef PRT_K1O_WAVES
#define PRT_K1O_WAVES PRT_K1_WAVES
#endif
// K1s (k_trace_surface, after the shading helpers it shares with K3 and k_features): the closest-hit loop once more, with a
// third write-out — where K1 writes its PrtHit the lane also reads the hit's shading record and material and writes one
// PrtSurface.  A sibling kernel, not a third mode of k_trace: as a mode (the loop as a device function under two wrappers)
// the any-hit instantiations compiled to other multiply-add contractions than before, and their bytes left the closest-hit
// kernel's on edge-grazing rays (2 of 400,000 on the 2M-triangle soup in fp32).
// What the two kernels (and K7, K6, K8) do share is the integer scheduling code around the loop: the wave's ray pool
// (WavePool, prt_wave.h) and the counter flush (flush_trace_counts, prt_device.h).  How much of the pool can be a function was
// settled on the compiled instructions, per kernel against the text that carried the block itself ("Shared
// scheduling code of the batch kernels"):
//   - one take(idle, lane, n, counter, idx&) doing refill, index and advance: the ray set-up after it contracts differently
//     (fp64 k_trace: v_fma_f32 28 -> 30, v_pk_fma_f32 5 -> 4, v_pk_mul_f32 5 -> 4, v_add_f32 1 -> 0) - the hazard above;
//   - deal(idle, ..., set-up as a lambda): ~25 more instructions per kernel, and again another fp32 mix;
//   - open() / index() / advance() with open() refilling and returning `need != 0 && !exhausted`: fp32 mix intact, but
//     written with an early return or as nested ifs the any-hit fp64 kernels lose a v_cmp / v_cndmask pair and K6 / K8 gain
//     a v_mov_b64; with the result computed before the refill the two counting any-hit fp64 kernels still lose the pair;
//   - wants() / refill() / index() / advance(), the condition tested by the kernel: every vector opcode count of every
//     kernel is the former one, registers, scratch and occupancy too.  That is the form in use; tr.init() stays in the kernel.
#ifndef PRT_K1S_WAVES
#define PRT_K1S_WAVES PRT_K1_WAVES // the 40 KB of stacks allow four blocks per CU; the surface write-out fits their 128 registers without scratch
#endif
template <bool COUNT, bool PAD, bool ANY>
__global__ __launch_bounds__(PRT_BLOCK, ANY ? PRT_K1O_WAVES : PRT_K1_WAVES) void k_trace(DScene S, const PrtRay* __restrict__ rays, size_t n,
                                                             typename std::conditional<ANY, uint8_t, PrtHit>::type* __restrict__ out, DCounters* ctr,
                                                             const uint32_t* __restrict__ perm) { // K4's order (ray_sort.hip) or null
    __shared__ uint32_t s_stack[PRT_BLOCK / 64][PRT_STACK_DEPTH][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* stk = &s_stack[wave][0][lane];
    WorkCount wc{0, 0, 0, 0, 0};
    uint32_t nrays = 0;
    Trav<PAD> tr;
    tr.init(S, mk3(0, 0, 0), mk3(0, 0, 1), RL(0.0), RL(0.0));
    if (!ANY) tr.hit.alpha = tr.hit.beta = RL(0.0);
    tr.active = false;
    bool have = false;
    size_t my = 0;
    WavePool<PRT_K1_CHUNK> pool; // the wave's rays (prt_wave.h)
    for (;;) {
        if (!tr.active && have) {
            if constexpr (ANY) {
                out[my] = tr.hit.tri >= 0 ? 1 : 0;
            } else {
                PrtHit h;
                if (tr.hit.tri >= 0) {
                    const DTri* T = tri_at<PAD>(S, (uint32_t)tr.hit.tri);
                    const d3 nrm = mk3(T->n[0], T->n[1], T->n[2]);
                    h.t = tr.hit.t;
                    h.alpha = tr.hit.alpha;
                    h.beta = tr.hit.beta;
                    h.prim = S.shade[tr.hit.tri].prim;
                    h.front = dot(tr.d, nrm) < RL(0.) ? 1 : 0; // HitRecord::SetFaceNormal, Hittable.cpp:8-13
                } else {
                    h.t = PRT_INF;
                    h.alpha = h.beta = 0;
                    h.prim = -1;
                    h.front = 0;
                }
                out[my] = h;
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
                        tr.init(S, mk3((real)r0.x, (real)r0.y, (real)r0.z), mk3((real)r1.x, (real)r1.y, (real)r1.z), (real)r0.w, (real)r1.w); // PrtRay is fp64 at the ABI in either mode
                        my = ri;
                        have = true;
                        nrays++;
                    }
                }
                pool.advance(need);
            }
        }
        if (__ballot(tr.active || have) == 0ULL && pool.exhausted) break;
        do {
            tr.template round<COUNT>(S, stk, wc, PRT_LEAF_BATCH, PRT_INNER_MIN, tr.tmin, ANY);
        } while (wave_count(tr.active) > (ANY ? PRT_K1O_KEEP : PRT_K1_KEEP));
    }
    flush_trace_counts<COUNT>(ctr, lane, ANY ? &ctr->rays_shadow : &ctr->rays_closest, nrays, wc);
}

// ------------------------------------------------------------------------------------------- K3
#ifndef PRT_ONE_PASS_VERTEX
#define PRT_ONE_PASS_VERTEX 1 // the lean and the CookTorrance permutation shade a path vertex in one pass (k_render, ONE_PASS)
#endif
#ifndef PRT_SAMPLE_TURNOVER
#define PRT_SAMPLE_TURNOVER 1 // the one-pass permutations start the next sample in the pass that ends the previous one (k_render, TURN)
#endif
enum : int { ST_FETCH = 0, ST_NEW_SAMPLE = 1, ST_CLOSEST = 2, ST_SHADOW = 3, ST_DONE = 4, ST_PRIMARY = 5, ST_CACHED = 6 };
// The camera ray of a pixel is the same for every sample (Camera.cpp:53-57: GetRay once per pixel, no jitter): K3 traces
// it ONCE per work item (ST_PRIMARY) and parks the ray's direction and its hit — t, triangle, barycentrics — in LDS,
// lane-strided; every sample of the item starts from that hit (ST_CACHED) instead of re-tracing the identical ray.

// Shading context of a hit, rebuilt from (incoming ray, HitInfo): HitRecord of Triangle::Hit
// (Triangle.cpp:76-80,111) — position = ray(t), face-forwarded normal, tangent, uv.
struct ShadeCtx {
    Frame f;
    d2 uv;
    int32_t material;
};
// `rd` = the direction the hit was reached along, (alpha, beta, tri) = the hit (read in place: no HitInfo copy)
// The three expressions every consumer of a hit shares (K3's make_ctx, k_features, the surface write-out of K1):
// HitRecord::SetFaceNormal (Hittable.cpp:8-13) on the stored geometric normal, ...
PRT_DEV d3 face_normal(d3 rd, d3 gn) {
    const bool front = dot(rd, gn) < RL(0.);
    return front ? gn : -gn;
}
// ... the texture coordinates of Triangle.cpp:111, ...
PRT_DEV d2 hit_uv(const DTriShade* sh, real alpha, real beta) {
    const real w0 = RL(1.) - alpha - beta;
    d2 uv;
    uv.x = w0 * sh->uv0[0] + alpha * sh->uv1[0] + beta * sh->uv2[0];
    uv.y = w0 * sh->uv0[1] + alpha * sh->uv1[1] + beta * sh->uv2[1];
    return uv;
}
// ... and the albedo feature of prt_render_features (include/prt.h): what the material multiplies diffuse light by
template <int F>
PRT_DEV d3 feature_albedo(const DScene& S, const DMaterial& m, d2 uv) {
    d3 a = mk3(1, 1, 1);
    if (m.type == PRT_MAT_LAMBERTIAN || m.type == PRT_MAT_DEBUG) a = mat_kd<F>(S, m, uv);
    else if (m.type == PRT_MAT_PHONG) a = mat_kd<F>(S, m, uv) + mat_ks<F>(S, m, uv);
    return a;
}
template <int FEAT, bool PAD>
PRT_DEV ShadeCtx make_ctx(const DScene& S, d3 rd, real alpha, real beta, int32_t tri) {
    ShadeCtx c;
    const DTriShade* sh = S.shade + tri;
    const DTri* T = tri_at<PAD>(S, (uint32_t)tri);
    const d3 gn = mk3(T->n[0], T->n[1], T->n[2]);
    c.f.n = face_normal(rd, gn);
    c.f.t = ld3(sh->tangent);
    if (FEAT & PRT_FEAT_TEX) { // texture coordinates are only read by image-textured materials
        c.uv = hit_uv(sh, alpha, beta);
    } else {
        c.uv.x = c.uv.y = RL(0.0);
    }
    c.material = sh->material;
    return c;
}

// K1's surface write-out: one PrtSurface from the ray the lane still holds and its finished closest-hit traversal.  The head
// is the PrtHit k_trace writes (same expressions on the same values); the body is computed in `real` and widened at the
// store.  Twelve 16-byte stores, each value stored as soon as it is known and the albedo — the only one behind a texture
// fetch — last: the twelve taps of a footprint then share the registers with the traversal state alone, not with a record
// waiting to be written (the fp64 kernel: 13 registers spilled when the record was put together first).
template <bool PAD>
PRT_DEV void surface_record(const DScene& S, d3 o, d3 d, const HitInfo& hit, PrtSurface* __restrict__ out) {
    static_assert(sizeof(PrtSurface) == 192 && offsetof(PrtSurface, position) == 32 && offsetof(PrtSurface, material) == 168, "PrtSurface layout");
    double2* q = reinterpret_cast<double2*>(out); // (the host checks the buffer's alignment)
    if (hit.tri >= 0) {
        const DTriShade* sh = S.shade + hit.tri;
        const d3 gn = ld3(tri_at<PAD>(S, (uint32_t)hit.tri)->n);
        const int32_t front = dot(d, gn) < RL(0.) ? 1 : 0; // as k_trace's head
        const unsigned long long pf = (unsigned long long)(uint32_t)sh->prim | ((unsigned long long)(uint32_t)front << 32);
        q[0] = make_double2((double)hit.t, (double)hit.alpha);
        q[1] = make_double2((double)hit.beta, __longlong_as_double((long long)pf));
        const d3 p = o + d * hit.t; // Ray::operator()
        const d3 fn = face_normal(d, gn);
        q[2] = make_double2((double)p.x, (double)p.y);
        q[3] = make_double2((double)p.z, (double)fn.x);
        q[4] = make_double2((double)fn.y, (double)fn.z);
        __builtin_amdgcn_sched_barrier(0); // (the shading record is fetched once the head and the normal are on their way, ...
        const d3 tg = ld3(sh->tangent);
        const d2 uv = hit_uv(sh, hit.alpha, hit.beta);
        q[5] = make_double2((double)tg.x, (double)tg.y);
        q[6] = make_double2((double)tg.z, (double)uv.x);
        __builtin_amdgcn_sched_barrier(0); // ... and the material after it: fetched all at once they cost the counting kernel two spilled registers)
        const int32_t mi = sh->material;
        const DMaterial& m = S.materials[mi];
        const d3 em = ld3(m.emission);
        const unsigned long long mt = (unsigned long long)(uint32_t)mi | ((unsigned long long)(uint32_t)m.type << 32);
        q[9] = make_double2((double)em.x, (double)em.y);
        q[10] = make_double2((double)em.z, __longlong_as_double((long long)mt));
        q[11] = make_double2(0.0, 0.0);
        const d3 a = feature_albedo<PRT_FEAT_ALL | PRT_FEAT_EXTRA | PRT_FEAT_NARROW>(S, m, uv);
        q[7] = make_double2((double)uv.y, (double)a.x);
        q[8] = make_double2((double)a.y, (double)a.z);
    } else {
        const double2 z = make_double2(0.0, 0.0);
        q[0] = make_double2((double)PRT_INF, 0.0);
        q[1] = make_double2(0.0, __longlong_as_double(0x00000000ffffffffLL)); // prim -1, front 0
        for (int k = 2; k < 12; ++k) q[k] = z;
        q[10] = make_double2(0.0, __longlong_as_double(-1LL)); // material = material_type = -1
    }
}

template <bool COUNT, bool PAD>
__global__ __launch_bounds__(PRT_BLOCK, PRT_K1S_WAVES) void k_trace_surface(DScene S, const PrtRay* __restrict__ rays, size_t n,
                                                                            PrtSurface* __restrict__ out, DCounters* ctr,
                                                                            const uint32_t* __restrict__ perm) { // K4's order (ray_sort.hip) or null
    __shared__ uint32_t s_stack[PRT_BLOCK / 64][PRT_STACK_DEPTH][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* stk = &s_stack[wave][0][lane];
    WorkCount wc{0, 0, 0, 0, 0};
    uint32_t nrays = 0;
    Trav<PAD> tr;
    tr.init(S, mk3(0, 0, 0), mk3(0, 0, 1), RL(0.0), RL(0.0));
    tr.hit.alpha = tr.hit.beta = RL(0.0);
    tr.active = false;
    bool have = false;
    size_t my = 0;
    WavePool<PRT_K1_CHUNK> pool; // the wave's rays (prt_wave.h)
    for (;;) {
        if (!tr.active && have) {
            surface_record<PAD>(S, tr.o, tr.d, tr.hit, out + my);
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
                        tr.init(S, mk3((real)r0.x, (real)r0.y, (real)r0.z), mk3((real)r1.x, (real)r1.y, (real)r1.z), (real)r0.w, (real)r1.w); // PrtRay is fp64 at the ABI in either mode
                        my = ri;
                        have = true;
                        nrays++;
                    }
                }
                pool.advance(need);
            }
        }
        if (__ballot(tr.active || have) == 0ULL && pool.exhausted) break;
        do {
            tr.template round<COUNT>(S, stk, wc, PRT_LEAF_BATCH, PRT_INNER_MIN, tr.tmin, false);
        } while (wave_count(tr.active) > PRT_K1_KEEP);
    }
    flush_trace_counts<COUNT>(ctr, lane, &ctr->rays_closest, nrays, wc);
}

// A real number parked in / fetched from a lane's LDS column (`base` = the lane's slot of word 0, words PRT_BLOCK apart)
template <int PARK_STRIDE>
PRT_DEV void park_real(uint32_t* base, int word, real v) {
    if (PRT_F32) {
        base[word * PARK_STRIDE] = __float_as_uint((float)v);
    } else {
        const unsigned long long b = (unsigned long long)__double_as_longlong((double)v);
        base[word * PARK_STRIDE] = (uint32_t)b;
        base[(word + 1) * PARK_STRIDE] = (uint32_t)(b >> 32);
    }
}
template <int PARK_STRIDE>
PRT_DEV real unpark_real(const uint32_t* base, int word) {
    if (PRT_F32) return (real)__uint_as_float(base[word * PARK_STRIDE]);
    return (real)__longlong_as_double((long long)(((unsigned long long)base[(word + 1) * PARK_STRIDE] << 32) | base[word * PARK_STRIDE]));
}
#define PRT_RW ((int)(sizeof(real) / 4)) // dwords per real
// a lane's parked camera ray and primary hit: t | triangle | direction[3] | (textured permutations) alpha, beta
#define PARK_T 0
#define PARK_TRI PRT_RW
#define PARK_DIR (PRT_RW + 1)
// Textured permutations do not park the direction: their LDS is spoken for (a deep tree's 40-entry stacks plus t, triangle
// and barycentrics plus the material table fill a third of a CU), so they recompute it per sample from the camera, read on
// demand (measured on bathroom2: parked in global memory +4.5 %, parked in LDS at the price of the 32-entry tree +2.5 %).
#define PARK_DIR_GLOBAL(feat) (((feat) & PRT_FEAT_TEX) != 0)
#define PARK_AB_AT(feat) (PARK_DIR_GLOBAL(feat) ? PRT_RW + 1 : 4 * PRT_RW + 1)
#define PARK_WORDS(feat) (((feat) & PRT_FEAT_TEX) ? 3 * PRT_RW + 1 : 4 * PRT_RW + 1)

// prt_ray_color (PRT_FEAT_RAYS kernels): ray i of the caller's batch, fp64 records rounded to the kernel's real on load.  tmin and
// tmax are not read: a primary ray is traced over Interval(0.0001, inf) like a camera ray (Camera.cpp:125).
PRT_DEV void load_ray(const void* ray_list, uint32_t i, d3& o, d3& d) {
    const PrtRay* r = static_cast<const PrtRay*>(ray_list) + i;
    o = mk3((real)r->o[0], (real)r->o[1], (real)r->o[2]);
    d = mk3((real)r->d[0], (real)r->d[1], (real)r->d[2]);
}

// K3's arguments are ONE struct, so that the kernel can also reach them through the kernarg segment pointer: what the
// hot loop needs (scene tables, thresholds, roulette, seed) is used as plain arguments — the compiler loads those into
// scalar registers once — while everything only a work-item fetch or a miss needs (the camera, tile geometry, the chunk
// table, the background, the output pointer: ~50 scalar registers) is read ON DEMAND through cold_args(), a pointer to the
// same bytes that the compiler cannot see through: s_load at the point of use instead of values kept (and, beyond ~100
// of them, spilled to VGPR lanes: 116 v_readlane per pass before this) across the whole traversal loop.
template <typename R> // (the scalar type shows in the kernel's name: profiles tell the fp64 launch from the fp32 one by it)
struct RenderArgsT {
    DSceneT<R> S;
    DCameraT<R> C;
    DRenderParamsT<R> P;
    double* partial;
    DCounters* ctr;
};
typedef RenderArgsT<real> RenderArgs;
typedef const RenderArgs __attribute__((address_space(4)))* ColdRenderArgs;
PRT_DEV ColdRenderArgs cold_args() {
    ColdRenderArgs q = (ColdRenderArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q)); // opaque from here on: loads through q stay where they are written
    return q;
}

template <bool COUNT, int FEAT, bool LLDS, bool PAD>
__global__ __launch_bounds__(PRT_BLOCK, render_waves(FEAT)) void k_render(RenderArgs A) {
    const DScene& S = A.S;
    const DRenderParams& P = A.P; // hot fields only: see RenderArgs
    DCounters* const ctr = A.ctr;
    // RAYS (prt_ray_color): the work item's primary ray is ray_list[oi] of the caller's batch instead of a camera ray, and the
    // key of its random streams is key_list[oi] (or oi) instead of the pixel index.  The ray is traced once per work item
    // and its hit parked like a camera ray's; a sample re-reads the ray itself (64 bytes, L2) instead of unparking a
    // direction and taking the block's one camera centre, so the park layout and the LDS budget are the frame kernels'.
    // `px` carries oi across the item; no pixel, no jitter.
    constexpr bool RAYS = (FEAT & PRT_FEAT_RAYS) != 0;
    // PLAIN (PRT_FEAT_PLAIN; render_plain() on the host decides, from the same values): the launch renders a frame with default
    // settings — no pixel jitter, items from the tiles, light sampling on, a scene with emitters whose light triangles are all
    // staged in LDS.  What the generic kernel tests per pass as launch-uniform values are constants here, so the branches
    // such a frame never takes (and the scalar registers that keep their conditions across the pass) are not compiled.
    // Only the conditions differ: every expression, every draw and the order of terms into acc are the generic kernel's.
    constexpr bool PLAIN = (FEAT & PRT_FEAT_PLAIN) != 0;
    static_assert(!PLAIN || (!COUNT && !RAYS && LLDS), "PLAIN: production frame kernels with LDS tables only");
#define JITTER (!PLAIN && P.jitter)                                // a camera ray of its own per sample
#define FROM_LIST (!PLAIN && P.scramble == PRT_ITEMS_FROM_LIST)    // prt_render_samples, adaptive rounds
#define SAMPLE_LIGHTS (PLAIN || P.sample_lights)                   // bSampleLights
#define HAS_LIGHTS (PLAIN || S.n_lights > 0)
#define LTRI_LDS (PLAIN ? 1 : P.ltri_lds)                          // > 0: the light triangles are read from LDS (all or none are staged)
    // DIFFUSE (PRT_FEAT_DIFFUSE on top of PLAIN, lean fp64 permutation only; render_diffuse() on the host decides, from a flag of
    // the scene's material table): every material that is not an emitter is an untextured Lambertian and none skips light
    // sampling.  Eval and Scatter are their Lambertian case without a test of m.type (mat_eval, mat_scatter), no vertex skips
    // its light pick, and prev_skip is never set, so it is not carried.  Again only conditions differ: has_emission stays a
    // per-lane test, the redraw loop of Scatter stays, every expression and draw is the generic kernel's.
    constexpr bool DIFFUSE = (FEAT & PRT_FEAT_DIFFUSE) != 0;
    static_assert(!DIFFUSE || (PLAIN && !(FEAT & PRT_FEAT_ALL) && !PRT_F32), "DIFFUSE: the lean fp64 PLAIN kernels only");
#define SKIPS_LIGHTS(m) (!DIFFUSE && (m).skip_light_sampling != 0) // SkipLightSampling of the vertex's material
    __shared__ uint32_t s_qoff[PRT_BLOCK / 64];
    __shared__ unsigned long long s_rays[PRT_BLOCK / 64];
    __shared__ real s_center[4]; // Camera::center, the origin of every camera ray
    constexpr int NPARK = PRT_BLOCK;
    __shared__ uint32_t s_park[PARK_WORDS(FEAT)][NPARK]; // per lane: the work item's camera ray and its hit (ST_PRIMARY), read once per sample
#define park (&s_park[0][threadIdx.x])
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Dynamic LDS, sized by the host: the four waves' traversal stacks (P.stack_depth entries per lane, lane-strided),
    // then the shading tables.  The depth is a launch parameter: what the scene's tree can need, not the builders' bound of
    // PRT_STACK_DEPTH — LDS left over decides how many blocks a CU holds (the fp32 kernels have the registers for a fourth
    // block when a tree needs at most 32 entries) and leaves room for the parked camera rays.
    extern __shared__ __align__(16) unsigned char s_dyn_all[];
#if PRT_DYN_STACK
    uint32_t* stk = reinterpret_cast<uint32_t*>(s_dyn_all) + (size_t)(wave * P.stack_depth) * 64 + lane;
    unsigned char* s_dyn = s_dyn_all + (size_t)(PRT_BLOCK / 64) * P.stack_depth * 64 * sizeof(uint32_t);
#else
    __shared__ uint32_t s_stack[PRT_BLOCK / 64][PRT_STACK_DEPTH][64];
    uint32_t* stk = &s_stack[wave][0][lane];
    unsigned char* s_dyn = s_dyn_all;
#endif
    if (lane == 0) {
        s_qoff[wave] = 0;
        s_rays[wave] = 0ULL;
    }
    if (threadIdx.x < 3) s_center[threadIdx.x] = A.C.center[threadIdx.x];
    if (!LLDS) __syncthreads(); // (the LLDS kernels synchronise below, after staging their tables)
    // light tree in LDS (see sample_lights)
    const DLightNode* lds_lights = reinterpret_cast<const DLightNode*>(s_dyn);
    // ... followed by the whole material table (the host only selects LLDS when it fits): its fields are read
    // several times per path vertex, and every one of those reads is otherwise a texture-addresser instruction
    const DMaterial* lds_mats = reinterpret_cast<const DMaterial*>(s_dyn + (size_t)P.light_lds * sizeof(DLightNode));
    const DLightTri* lds_ltris = reinterpret_cast<const DLightTri*>(s_dyn + (size_t)P.light_lds * sizeof(DLightNode) + (size_t)P.mat_lds * sizeof(DMaterial));
    if (LLDS) { // every thread of the block gets here before any divergence
        uint4* dst = reinterpret_cast<uint4*>(s_dyn);
        const uint4* src = reinterpret_cast<const uint4*>(S.light_nodes);
        for (int i = threadIdx.x; i < P.light_lds; i += PRT_BLOCK) dst[i] = src[i];
        dst += P.light_lds;
        src = reinterpret_cast<const uint4*>(S.materials);
        const int nm = P.mat_lds * (int)(sizeof(DMaterial) / 16);
        for (int i = threadIdx.x; i < nm; i += PRT_BLOCK) dst[i] = src[i];
        dst += nm;
        src = reinterpret_cast<const uint4*>(S.light_tris);
        const int nl = P.ltri_lds * (int)(sizeof(DLightTri) / 16);
        for (int i = threadIdx.x; i < nl; i += PRT_BLOCK) dst[i] = src[i];
        __syncthreads();
    }
#define MATERIAL(i) (LLDS ? lds_mats[(i)] : S.materials[(i)])
    d3 pst_[2]; // acc (this item's sum of sample radiance / spp), beta (path throughput)
#define PST_LD(k) (pst_[(k) / 3])
#define PST_ST(k, v) (pst_[(k) / 3] = (v))
#define S_ACC 0
#define S_BETA 3
// A radiance term x met by the current path (emission, background, NEE): colorAttachment[m] += RayColor(...) *
// pixelSamplesScale (Camera.cpp:56) with RayColor unrolled into sum_k beta_k * x_k; each term is scaled and
// added on the spot, so no per-sample radiance has to live in registers across traversals.
#define ADD_RADIANCE(x) PST_ST(S_ACC, PST_LD(S_ACC) + (PST_LD(S_BETA) * (x)) * inv_spp)
// prt_render_samples with a trace buffer (counting instantiation, one sample per work item): the path's signature,
// vertex v = max_depth - depth (prt.h, PRT_TRACE_*)
#define TRACING (COUNT && P.scramble == PRT_ITEMS_FROM_LIST && ctr->trace != nullptr)
#define TRACE_VERTEX(prim_)                                                     \
    do {                                                                        \
        if (TRACING) {                                                          \
            const int v_ = P.max_depth - depth;                                 \
            if (v_ < PRT_TRACE_VERTS) {                                         \
                int32_t* tw_ = ctr->trace + (size_t)item * PRT_TRACE_WORDS;     \
                tw_[0] = v_ + 1;                                                \
                tw_[1 + 2 * v_] = (prim_);                                      \
                tw_[2 + 2 * v_] = 0;                                            \
            }                                                                   \
        }                                                                       \
    } while (0)
#define TRACE_FLAG_AT(v_, bit_)                                                 \
    do {                                                                        \
        if (TRACING) {                                                          \
            if ((v_) < PRT_TRACE_VERTS) ctr->trace[(size_t)item * PRT_TRACE_WORDS + 2 + 2 * (v_)] |= (bit_); \
        }                                                                       \
    } while (0)
#define TRACE_FLAG(bit_)                                                        \
    do {                                                                        \
        if (TRACING) {                                                          \
            const int v_ = P.max_depth - depth;                                 \
            if (v_ < PRT_TRACE_VERTS) ctr->trace[(size_t)item * PRT_TRACE_WORDS + 2 + 2 * v_] |= (bit_); \
        }                                                                       \
    } while (0)

    WorkCount wc{0, 0, 0, 0, 0};
    // Rays are counted per WAVE in LDS (ballot + popcount, one 64-bit LDS add by lane 0 per pass: closest | shadow << 32): no
    // register holds a count.  Camera samples are not counted at all: their number follows from the launch (host).
    uint32_t n_refills = 0;

    int state = ST_FETCH;
    uint32_t item = 0; // work items of a launch are counted in 32 bits (the host refuses more): every division below is a 32-bit one
    int px = 0, py = 0, s = 0, s_end = 0, depth = 0;
    uint32_t pixel = 0; // j * W + i of the work item's pixel: the RNG key
    bool first = true, prev_skip = false;
    PST_ST(S_ACC, mk3(0, 0, 0));  // sum over this item's samples of colour * (1/spp)
    PST_ST(S_BETA, mk3(1, 1, 1)); // path throughput
    // Across a continuation traversal the ray lives in tr.o / tr.d only.  Across a shadow traversal
    // tr.o is the shading point itself, so only the incoming direction, the hit's barycentrics and
    // the light pick need to be kept.
    d3 rd = mk3(0, 0, 1);        // incoming direction at the shading point (valid in ST_SHADOW)
    int32_t sh_tri = -1;
    real ldist = 0;              // distance to the sampled light point (valid in ST_SHADOW)
    int32_t ltri = 0;
    // ONE_PASS (the lean and the CookTorrance permutation; not Phong, whose Eval draws a random number only when the light is
    // visible, and not the textured ones, which measure slower with it: DESIGN.md section 4): the pass that consumes a closest
    // hit shades the WHOLE vertex — light pick, the light's contribution as if it were visible,
    // roulette and Scatter — and the lane carries across its shadow traversal just that contribution, the scattered
    // direction and whether the path goes on.  A returning shadow ray then needs no shading: add the term if nothing was
    // hit, take the stored direction.  Lanes in that state are chained onto their continuation ray between traversal rounds
    // (P.chain_min) or by the next pass.  Same draws in the same order, same operations on the same values: the frames are
    // those of the two-pass flow bit for bit.  rd, sh_tri, ldist and ltri then live inside one pass only.
    constexpr bool ONE_PASS = PRT_ONE_PASS_VERTEX && !(FEAT & (PRT_FEAT_PHONG | PRT_FEAT_TEX));
    constexpr bool EVAL_FLAT = ONE_PASS && !(FEAT & PRT_FEAT_CT); // Lambertian / mirror / light only: Eval needs no shading frame
    // TURN (the one-pass permutations): a lane walks a pass in path order.  A returned shadow ray without continuation and a
    // traced ray that left the scene end their sample at the top of the pass, before anything is shaded; the turnover (next
    // sample index, stream seed, the parked camera hit) follows at once, and the closest-hit block below consumes the fresh
    // sample's camera vertex in the SAME pass — as it does for an item whose camera ray has just returned.  Only a sample that
    // ends inside the shading blocks (emitter, roulette without a light point, a camera vertex that ends its sample) waits, as
    // ST_CACHED, for the next pass's turnover.  Same draws, same expressions, same order of terms into acc.
    // Not the fp32 lean kernels: with this order the compiler contracts the multiply-adds of their Scatter (local_to_world,
    // normalize) differently, and their frames would leave the previous ones by a few fp32 ulps; they
    // keep the order they had.  fp32 CookTorrance and every fp64 kernel give the same bits either way.
    constexpr bool TURN = ONE_PASS && PRT_SAMPLE_TURNOVER && !(PRT_F32 && !(FEAT & PRT_FEAT_CT));
    // WAVE_DIET (the fp64 one-pass permutations): the wave loop below takes its control from lane masks in scalar registers
    // and tests leaves through Trav::test_leaf_pp — fewer vector instructions per round for the same rounds (DESIGN.md
    // section 4).  Every other permutation, and both fp32 translation units, keep the loop and the code they had.
    constexpr bool WAVE_DIET = ONE_PASS && !PRT_F32;
    d3 pending = mk3(0, 0, 0);   // ONE_PASS, ST_SHADOW: (throughput * direct light) / spp, added if the shadow ray escapes
    d3 next_d = mk3(0, 0, 1);    // ONE_PASS, ST_SHADOW: the scattered direction (valid if cont)
    bool cont = false;           // ONE_PASS, ST_SHADOW: the path goes on after this vertex
    int nee_v = 0;               // (tracing: the vertex the shadow ray belongs to, saved before depth--)
    Rng rng;
    rng.s = 0;
    const real inv_spp = RL(1.0) / (real)P.spp; // pixelSamplesScale, Camera.cpp:83
    Trav<PAD, PRT_BOX_PK != 0> tr; // packed-FMA box test: every K3 permutation has the registers for it (coefficients in scalar registers)
    tr.init(S, mk3(0, 0, 0), rd, RL(0.0), RL(0.0));
    tr.hit.alpha = tr.hit.beta = RL(0.0); // init() leaves the barycentrics alone (they survive shadow traversals)
    tr.active = false;

#if PRT_K3_PROFILE
    unsigned long long prof_[6] = {0, 0, 0, 0, 0, 0}, prof_t_ = __builtin_readcyclecounter();
#endif
    // (Two blocks the pass uses at two places, as macros: as lambdas they changed the code of the two-pass permutations.)
    // A sample has ended: the item's next one is due (`next`: how it is marked), or the item's sum is written and the lane fetches
#define END_OF_SAMPLE(next) do {                                                                                                                                          \
        s++;                                                                                                                                                              \
        if (s < s_end) state = (next);                                                                                                                                     \
        else {                                                                                                                                                            \
            const d3 acc = PST_LD(S_ACC); /* read here, at the item's end: a sample that merely ends carries no copy of the sum */                                        \
            double* o = cold_args()->partial + (size_t)item * 3;                                                                                                          \
            o[0] = (double)acc.x; /* the partial sums are fp64 in either mode (K5 adds them in fp64) */                                                                   \
            o[1] = (double)acc.y;                                                                                                                                         \
            o[2] = (double)acc.z;                                                                                                                                         \
            state = ST_FETCH;                                                                                                                                             \
        }                                                                                                                                                                 \
    } while (0)
    // Sample s of the item starts: its stream, its camera ray (P.jitter: to be traced, ST_CLOSEST) or that ray's parked hit
    // (`parked`: the state of a lane that holds it, with nothing to trace)
#define NEW_SAMPLE(parked) do {                                                                                                                                           \
        /* per-sample stream keyed (seed, j*W+i, s) */                                                                                                                    \
        rng.seed_keyed(P.seed_key, (uint64_t)pixel, (uint64_t)s);                                                                                                         \
        if (!RAYS && JITTER) {                                                                                                                                            \
            /* the disabled SampleSquare() offset of Camera.cpp:110-111, drawn per sample: y first (g++ argument order); */                                               \
            /* a camera ray of its own, traced like any other */                                                                                                          \
            const ColdRenderArgs q = cold_args();                                                                                                                         \
            const int W = q->C.width;                                                                                                                                     \
            const int jy = (int)(pixel / (uint32_t)W), jx = (int)(pixel - (uint32_t)jy * (uint32_t)W);                                                                    \
            const real fy = (real)jy + (rng.next() - RL(0.5));                                                                                                            \
            const real fx = (real)jx + (rng.next() - RL(0.5));                                                                                                            \
            const d3 ps = mk3(q->C.pixel00[0], q->C.pixel00[1], q->C.pixel00[2]) + fx * mk3(q->C.du[0], q->C.du[1], q->C.du[2]) +                                         \
                          fy * mk3(q->C.dv[0], q->C.dv[1], q->C.dv[2]);                                                                                                   \
            tr.o = mk3(q->C.center[0], q->C.center[1], q->C.center[2]);                                                                                                   \
            tr.d = ps - tr.o;                                                                                                                                             \
            state = ST_CLOSEST;                                                                                                                                           \
        } else {                                                                                                                                                          \
            /* Camera::GetRay gives every sample of the pixel the same ray (Camera.cpp:53-57, no jitter): the sample starts */                                            \
            /* from the parked hit of that ray.  Nothing to trace.  Two-pass permutations: the lane waits for the next pass, which */                                     \
            /* consumes the hit (the LDS reads below have the traversal rounds in between to arrive); TURN: this pass does. */                                            \
            if (RAYS) { /* the lane's own ray, read again (the parked words hold its hit only) */                                                                         \
                load_ray(ctr->ray_list, (uint32_t)px, tr.o, tr.d);                                                                                                        \
            } else if (PARK_DIR_GLOBAL(FEAT)) { /* Camera::GetRay again (same expressions as at the fetch: the same bits) */                                              \
                tr.o = mk3(s_center[0], s_center[1], s_center[2]);                                                                                                        \
                const ColdRenderArgs q = cold_args();                                                                                                                     \
                const d3 ps = mk3(q->C.pixel00[0], q->C.pixel00[1], q->C.pixel00[2]) + (real)px * mk3(q->C.du[0], q->C.du[1], q->C.du[2]) +                               \
                              (real)py * mk3(q->C.dv[0], q->C.dv[1], q->C.dv[2]);                                                                                         \
                tr.d = ps - tr.o;                                                                                                                                         \
            } else {                                                                                                                                                      \
                tr.o = mk3(s_center[0], s_center[1], s_center[2]);                                                                                                        \
                tr.d = mk3(unpark_real<NPARK>(park, PARK_DIR), unpark_real<NPARK>(park, PARK_DIR + PRT_RW), unpark_real<NPARK>(park, PARK_DIR + 2 * PRT_RW));             \
            }                                                                                                                                                             \
            tr.hit.t = unpark_real<NPARK>(park, PARK_T);                                                                                                                  \
            tr.hit.tri = (int32_t)park[PARK_TRI * NPARK];                                                                                                                 \
            if (FEAT & PRT_FEAT_TEX) {                                                                                                                                    \
                tr.hit.alpha = unpark_real<NPARK>(park, PARK_AB_AT(FEAT));                                                                                                \
                tr.hit.beta = unpark_real<NPARK>(park, PARK_AB_AT(FEAT) + PRT_RW);                                                                                        \
            }                                                                                                                                                             \
            state = (parked);                                                                                                                                             \
        }                                                                                                                                                                 \
        PST_ST(S_BETA, mk3(1, 1, 1));                                                                                                                                     \
        depth = P.max_depth;                                                                                                                                              \
        first = true;                                                                                                                                                     \
        prev_skip = false;                                                                                                                                                \
    } while (0)
    for (;;) {
        if (COUNT) n_refills++;
        PROF_MARK(0); // traversal rounds (and loop control) since the last mark
        int started = 0; // this pass started a traversal of this kind on this lane (1 closest, 2 shadow): counted below, where the wave has reconverged
        if (!tr.active) {
            // ---------------- a traversal has just finished on this lane: consume its result
            bool end_sample = false, do_scatter = false;
            bool nee = false; // ONE_PASS: this pass found a light point worth a shadow ray (tr.d is the direction towards it)
            // The ray this lane traces next is written straight into tr.o / tr.d as soon as it is known (shadow ray:
            // origin = shading point, direction towards the light; continuation: same origin, scattered direction; new
            // sample: the camera ray) — no staging copies, no selects at the traversal set-up.  After a closest hit has
            // been consumed tr.o IS the shading point.
            bool have_fr = false;
            d3 fr_seen = mk3(0, 0, 0);
            if (state == ST_PRIMARY) {
                // The item's camera ray has been traced.  If it left the scene or met an emitter, every sample of the item is
                // that one radiance (Camera.cpp:127,129-132: no random number is drawn): the item's samples are added up
                // right here, in the order and with the operations ADD_RADIANCE would use one pass at a time (same bits),
                // and the lane moves on to its next item instead of sitting through one pass per sample.
                bool flat = false;
                d3 x = mk3(0, 0, 0);
                // (Measured: veach-mis -2.0 %, where many pixels look at a light or past the scene; cornell +0.7 %, bathroom2 +-0 —
                // so only the permutations with glossy materials carry it.  prt_render_samples keeps the per-sample flow.)
                if ((FEAT & (PRT_FEAT_PHONG | PRT_FEAT_CT)) && !FROM_LIST) {
                    if (tr.hit.tri < 0) {
                        const ColdRenderArgs q = cold_args();
                        x = mk3(q->P.background[0], q->P.background[1], q->P.background[2]);
                        flat = true;
                    } else {
                        const DMaterial& m = MATERIAL(S.shade[tr.hit.tri].material);
                        if (m.has_emission) {
                            x = ld3(m.emission);
                            flat = true;
                        }
                    }
                }
                if (flat) {
                    const d3 term = (mk3(1, 1, 1) * x) * inv_spp; // throughput 1 at the camera vertex
                    d3 acc = PST_LD(S_ACC);
                    for (; s < s_end; ++s) acc = acc + term;
                    double* o = cold_args()->partial + (size_t)item * 3;
                    o[0] = (double)acc.x;
                    o[1] = (double)acc.y;
                    o[2] = (double)acc.z;
                    state = ST_FETCH;
                }
            }
            if (state == ST_PRIMARY) {
                // its hit serves every sample of the item (the barycentrics are only ever read for texture coordinates:
                // untextured permutations keep t and the triangle)
                park_real<NPARK>(park, PARK_T, tr.hit.t);
                park[PARK_TRI * NPARK] = (uint32_t)tr.hit.tri;
                if (FEAT & PRT_FEAT_TEX) {
                    park_real<NPARK>(park, PARK_AB_AT(FEAT), tr.hit.alpha);
                    park_real<NPARK>(park, PARK_AB_AT(FEAT) + PRT_RW, tr.hit.beta);
                }
                state = ST_NEW_SAMPLE; // two-pass: set up at the bottom of this pass, consumed by the next one; TURN: set up right below
            }
            // WAVE_DIET: the lane's next ray is the continuation ray of a vertex already shaded.  Both places that find this out
            // (a returned shadow ray at the top of the pass, a vertex without a light point below) only say so; the direction
            // is taken once, where the traversal is set up, so tr.d has one assignment in the pass instead of a copy of all
            // three components in every branch of the turnover block (six v_mov_b64 four times over, tools/isa_sections.py).
            bool take_next = false;
            bool hit_ready = false; // TURN: the lane holds a closest hit to consume in this pass (else, in ST_CLOSEST, a ray to trace)
            if (TURN) {
                // ---- ends that need no shading, then the turnover: a fresh sample's camera hit is consumed below, in this pass
                bool ended = false;
                if (state == ST_CACHED) state = ST_NEW_SAMPLE; // its sample ended inside the previous pass's shading blocks
                else if (state == ST_SHADOW) {
                    // shadow ray returned, vertex already shaded (the lanes the wave loop below did not chain)
                    if (tr.hit.tri < 0) {
                        PST_ST(S_ACC, PST_LD(S_ACC) + pending);
                        TRACE_FLAG_AT(nee_v, PRT_TRACE_VISIBLE);
                    }
                    if (cont) {
                        if (WAVE_DIET) take_next = true;
                        else tr.d = next_d;
                        state = ST_CLOSEST;
                    } else {
                        ended = true;
                    }
                } else if (state == ST_CLOSEST) {
                    if (tr.hit.tri < 0) {
                        // a traced ray left the scene: background for the camera ray (Camera.cpp:127); with bSampleLights a bounce miss adds 0 (:187)
                        if (first || !SAMPLE_LIGHTS) {
                            const ColdRenderArgs q = cold_args();
                            ADD_RADIANCE(mk3(q->P.background[0], q->P.background[1], q->P.background[2]));
                        }
                        TRACE_VERTEX(-1);
                        ended = true;
                    } else {
                        hit_ready = true;
                    }
                }
                if (ended) END_OF_SAMPLE(ST_NEW_SAMPLE);
                if (state == ST_NEW_SAMPLE) {
                    NEW_SAMPLE(ST_CLOSEST);
                    hit_ready = RAYS || !JITTER; // (a jittered sample's camera ray is traced first: the set-up at the bottom starts it)
                }
                PROF_MARK(3); // cheap ends + sample turnover: booked with the end of sample / fetch section below
            } else {
                if (state == ST_CACHED) state = ST_CLOSEST; // a sample set up by the previous pass from the parked hit: nothing to trace
            }
            if (TURN ? hit_ready : state == ST_CLOSEST) {
                if (tr.hit.tri < 0) {
                    // miss: background for the camera ray (Camera.cpp:127); with bSampleLights a bounce miss adds 0 (:187)
                    if (first || !SAMPLE_LIGHTS) {
                        const ColdRenderArgs q = cold_args();
                        ADD_RADIANCE(mk3(q->P.background[0], q->P.background[1], q->P.background[2]));
                    }
                    TRACE_VERTEX(-1);
                    end_sample = true;
                } else {
                    const DMaterial& m = MATERIAL(S.shade[tr.hit.tri].material);
                    TRACE_VERTEX(S.shade[tr.hit.tri].prim);
                    if (m.has_emission) {
                        // Camera.cpp:129-132; via a bounce only after SkipLightSampling materials (:191-195)
                        if (first || !SAMPLE_LIGHTS || (!DIFFUSE && prev_skip)) ADD_RADIANCE(ld3(m.emission));
                        end_sample = true;
                    } else {
                        rd = tr.d;
                        sh_tri = tr.hit.tri;
                        tr.o = tr.o + tr.d * tr.hit.t; // record.position = ray(t): from here on the origin of whatever comes next
                        do_scatter = true;
                        if (SAMPLE_LIGHTS && HAS_LIGHTS && !SKIPS_LIGHTS(m)) {
                            // next-event estimation, Camera.cpp:137-155: pick the light point now (4 draws)
                            const d3 gn = ld3(tri_at<PAD>(S, (uint32_t)sh_tri)->n);
                            const d3 fn = dot(rd, gn) < RL(0.) ? gn : -gn;
                            const LightPick lp = sample_lights<LLDS, (FEAT & PRT_FEAT_EXTRA) != 0>(S, tr.o, rng, lds_lights, P.light_lds, lds_ltris, LTRI_LDS);
                            real dist;
                            const d3 ldir = normalize_len(lp.pos - tr.o, dist);
                            if (dot(fn, ldir) > RL(0.0) && lp.front) {
                                ltri = lp.tri;
                                ldist = dist;
                                tr.d = ldir;
                                TRACE_FLAG(PRT_TRACE_NEE);
                                if (ONE_PASS) {
                                    nee = true; // the vertex is finished below; the shadow ray starts at the end of this pass
                                    if (COUNT) nee_v = P.max_depth - depth;
                                    if (EVAL_FLAT) {
                                        // Eval reads the material alone here (albedo / pi, or 0) and cos(theta) is the dot product
                                        // just tested — the shading frame's normal IS fn — so the light's contribution needs no
                                        // shading context: the expressions of the two-pass flow's ST_SHADOW block, same order
                                        d3 ln0;
                                        real pdf;
                                        int32_t lmat;
                                        if (LLDS && LTRI_LDS > 0) {
                                            const DLightTri* lt = lds_ltris + lp.tri;
                                            ln0 = ld3(lt->n); pdf = lt->pdf; lmat = lt->material;
                                        } else {
                                            const DLightTri* lt = S.light_tris + lp.tri;
                                            ln0 = ld3(lt->n); pdf = lt->pdf; lmat = lt->material;
                                        }
                                        const d3 ln = dot(ldir, ln0) < RL(0.) ? ln0 : -ln0;
                                        const d3 emission = ld3(MATERIAL(lmat).emission);
                                        d2 no_uv;
                                        no_uv.x = no_uv.y = RL(0.0);
                                        const d3 fr = mat_eval<FEAT>(S, m, ldir, ldir, no_uv, rng); // (directions and uv unread, no draw)
                                        const real cosT = dot(ldir, fn); // world_to_local(ldir, frame).z
                                        const real cosTB = -dot(ln, ldir);
                                        const d3 direct = (emission * fr) * fast_div(cosT * cosTB, (dist * dist) * pdf);
                                        pending = (PST_LD(S_BETA) * direct) * inv_spp; // what ADD_RADIANCE(direct) adds: the throughput BEFORE Scatter
                                    }
                                } else {
                                    state = ST_SHADOW; // trace the shadow ray, then scatter
                                    do_scatter = false;
                                }
                            }
                        }
                    }
                }
            } else if (ONE_PASS && !TURN && state == ST_SHADOW) {
                // ---- shadow ray returned, vertex already shaded (the lanes the wave loop below did not chain)
                if (tr.hit.tri < 0) {
                    PST_ST(S_ACC, PST_LD(S_ACC) + pending);
                    TRACE_FLAG_AT(nee_v, PRT_TRACE_VISIBLE);
                }
                if (cont) {
                    tr.d = next_d;
                    state = ST_CLOSEST;
                } else {
                    end_sample = true;
                }
            } else if (!ONE_PASS && state == ST_SHADOW) {
                // ---- shadow ray returned: visibility = closest hit no nearer than dist - 1e-3 (Camera.cpp:152-155)
                const real dist = ldist;
                // The shadow ray was traced over [0.001, dist - 0.001] only: the reference's test
                // `dist - |ps - pNearest| < 0.001` on the closest hit of [0.001, DBL_MAX) (|direction| = 1, so the distance
                // IS t) fails exactly when some triangle is hit inside that interval; an escaping ray counts as unoccluded (B9)
                const bool visible = tr.hit.tri < 0;
                if (visible) {
                    // the barycentrics are still the shading point's: shadow traversals leave them alone
                    const ShadeCtx c = make_ctx<FEAT, PAD>(S, rd, tr.hit.alpha, tr.hit.beta, sh_tri);
                    const DMaterial& m = MATERIAL(c.material);
                    d3 ln0;
                    real pdf;
                    int32_t lmat;
                    if (LLDS && LTRI_LDS > 0) {
                        const DLightTri* lt = lds_ltris + ltri;
                        ln0 = ld3(lt->n); pdf = lt->pdf; lmat = lt->material;
                    } else {
                        const DLightTri* lt = S.light_tris + ltri;
                        ln0 = ld3(lt->n); pdf = lt->pdf; lmat = lt->material;   // Triangle.cpp:92, BVH.cpp:91,66
                    }
                    // SetFaceNormal(Ray(origin, p - origin), normal) (Triangle.cpp:89-90); p - origin = tr.d * dist
                    const d3 ln = dot(tr.d, ln0) < RL(0.) ? ln0 : -ln0;
                    const d3 emission = ld3(MATERIAL(lmat).emission);
                    const d3 wo = world_to_local(-rd, c.f);
                    const d3 lwi = world_to_local(tr.d, c.f);
                    const d3 fr = mat_eval<FEAT>(S, m, lwi, wo, c.uv, rng);
                    if (FEAT & PRT_FEAT_TEX) {
                        have_fr = m.type == 0; // Lambertian: Eval returned albedo / pi, which Scatter needs again
                        fr_seen = fr;
                    }
                    const real cosT = lwi.z;
                    // cosThetaB = dot(WorldToLocal(lightNormal), -wi) (Camera.cpp:166-170): the shading frame is
                    // orthonormal (tangent in the triangle's plane, bitangent = t x n), so the local dot product IS the
                    // world one — three multiplies instead of a third change of basis; differs by rounding only
                    const real cosTB = -dot(ln, tr.d);
                    // Camera.cpp:172: emission*fr*cosT*cosTB/dist^2/pdf, the scalar factor folded into one division
                    const d3 direct = (emission * fr) * fast_div(cosT * cosTB, (dist * dist) * pdf);
                    ADD_RADIANCE(direct);
                    TRACE_FLAG(PRT_TRACE_VISIBLE);
                }
                state = ST_CLOSEST;
                do_scatter = true;
            }

            PROF_MARK(1); // consume: closest hit (emission, light pick) or shadow ray (light evaluation)
            if (ONE_PASS && do_scatter) {
                // ---- the light's contribution (Camera.cpp:157-172, the expressions of the ST_SHADOW block above), Russian
                // roulette and Scatter (Camera.cpp:176-202, those of the block below) on ONE shading context.  Eval draws
                // nothing in these permutations, so the roulette number — the next one of the stream either way — is drawn
                // first: a lane that has no light point and does not survive the roulette needs no context at all.
                end_sample = true;
                const bool rr_ok = rng.next() < P.rr;
                if ((nee && !EVAL_FLAT) || rr_ok) {
                    const ShadeCtx c = make_ctx<FEAT, PAD>(S, rd, tr.hit.alpha, tr.hit.beta, sh_tri);
                    const DMaterial& m = MATERIAL(c.material);
                    if (nee && !EVAL_FLAT) {
                        d3 ln0;
                        real pdf;
                        int32_t lmat;
                        if (LLDS && LTRI_LDS > 0) {
                            const DLightTri* lt = lds_ltris + ltri;
                            ln0 = ld3(lt->n); pdf = lt->pdf; lmat = lt->material;
                        } else {
                            const DLightTri* lt = S.light_tris + ltri;
                            ln0 = ld3(lt->n); pdf = lt->pdf; lmat = lt->material;
                        }
                        const d3 ln = dot(tr.d, ln0) < RL(0.) ? ln0 : -ln0;
                        const d3 emission = ld3(MATERIAL(lmat).emission);
                        const d3 wo = world_to_local(-rd, c.f);
                        const d3 lwi = world_to_local(tr.d, c.f);
                        const d3 fr = mat_eval<FEAT>(S, m, lwi, wo, c.uv, rng);
                        const real cosT = lwi.z;
                        const real cosTB = -dot(ln, tr.d);
                        const d3 direct = (emission * fr) * fast_div(cosT * cosTB, (ldist * ldist) * pdf);
                        pending = (PST_LD(S_BETA) * direct) * inv_spp; // what ADD_RADIANCE(direct) adds: the throughput BEFORE Scatter
                    }
                    if (rr_ok) {
                        d3 att;
                        TRACE_FLAG(PRT_TRACE_ROULETTE);
                        if (mat_scatter<FEAT>(S, m, rd, c.f, c.uv, rng, att, next_d)) {
                            TRACE_FLAG(PRT_TRACE_SCATTER);
                            depth--;
                            if (depth >= 0) {
                                const d3 beta = (PST_LD(S_BETA) * att) * P.inv_rr;
                                PST_ST(S_BETA, beta);
                                if (!(beta.x == RL(0.) && beta.y == RL(0.) && beta.z == RL(0.))) {
                                    prev_skip = SKIPS_LIGHTS(m);
                                    first = false;
                                    end_sample = false;
                                }
                            }
                        }
                    }
                }
                if (nee) { // the shadow ray first (tr.d points at the light already); what follows it is known
                    cont = !end_sample;
                    end_sample = false;
                    state = ST_SHADOW;
                } else if (!end_sample) {
                    if (WAVE_DIET) take_next = true;
                    else tr.d = next_d;
                }
            } else if (do_scatter) {
                // ---- Russian roulette + Scatter, Camera.cpp:176-202
                end_sample = true;
                if (rng.next() < P.rr) {
                    const ShadeCtx c = make_ctx<FEAT, PAD>(S, rd, tr.hit.alpha, tr.hit.beta, sh_tri);
                    const DMaterial& m = MATERIAL(c.material);
                    d3 att, wi;
                    TRACE_FLAG(PRT_TRACE_ROULETTE);
                    if (mat_scatter<FEAT>(S, m, rd, c.f, c.uv, rng, att, wi, have_fr, fr_seen)) {
                        TRACE_FLAG(PRT_TRACE_SCATTER);
                        depth--; // RayColor(scattered, depth-1): returns 0 when depth-1 < 0
                        if (depth >= 0) {
                            const d3 beta = (PST_LD(S_BETA) * att) * P.inv_rr;
                            PST_ST(S_BETA, beta);
                            // a zero throughput (Phong bad sample) contributes exactly 0 from here on
                            if (!(beta.x == RL(0.) && beta.y == RL(0.) && beta.z == RL(0.))) {
                                tr.d = wi;
                                prev_skip = SKIPS_LIGHTS(m);
                                first = false;
                                end_sample = false;
                            }
                        }
                    }
                }
            }
            PROF_MARK(2); // roulette + Scatter
            // TURN: a sample that ended inside the shading blocks waits for the next pass's turnover (ST_CACHED: nothing in flight)
            if (end_sample) END_OF_SAMPLE(TURN ? ST_CACHED : ST_NEW_SAMPLE);

            // ---------------- give the lane its next piece of work
            if (state == ST_FETCH) {
                const ColdRenderArgs q = cold_args(); // everything a fetch needs is read here, on demand
                const uint32_t n_items = (uint32_t)q->P.n_items;
                // One returning atomic per wave and pass on the wave's current queue (the queue index is wave-uniform,
                // so the compiler aggregates the lanes that execute it); a queue that hands out an index past the end
                // is dry for good (its indices only grow) and the lanes that drew a blank move on to the next one.
                // s_qoff[wave] = queues this wave has seen run dry.
                {
                    uint32_t off = __builtin_amdgcn_readfirstlane(s_qoff[wave]);
                    item = n_items;
                    while (off < (uint32_t)PRT_ITEM_QUEUES) {
                        const uint32_t qi = (blockIdx.x + off) % (uint32_t)PRT_ITEM_QUEUES;
                        const unsigned long long idx = atomicAdd(&ctr->queue[qi * PRT_QUEUE_STRIDE], 1ULL);
                        const unsigned long long it = ((idx >> 6) * PRT_ITEM_QUEUES + qi) * 64ULL + (idx & 63ULL);
                        if (it < n_items) {
                            item = (uint32_t)it;
                            break;
                        }
                        ++off;
                    }
                    atomicMax(&s_qoff[wave], off);
                }
                if (item >= n_items) {
                    state = ST_DONE;
                } else {
                    const uint32_t ipc = (uint32_t)q->P.items_per_chunk;
                    const uint32_t chunk = item / ipc;
                    const uint32_t oi = item - chunk * ipc;
                    const int W = q->C.width;
                    bool valid;
                    if (RAYS) { // prt_ray_color: item oi of a chunk is ray oi of the batch
                        px = (int)oi;
                        valid = true;
                    } else if (FROM_LIST) { // prt_render_samples: the pixels of a list
                        const int32_t pix = ctr->pixel_list[oi];
                        py = pix / W;
                        px = pix - py * W;
                        valid = true;
                        if (COUNT && ctr->trace != nullptr) ctr->trace[(size_t)item * PRT_TRACE_WORDS] = 0;
                    } else {
                        valid = tile_pixel(P.scramble, ipc, q->P.tile, q->P.tiles_x, q->P.n_tiles, q->P.rank, q->P.nranks, W, q->C.height, oi, px, py);
                    }
                    if (valid) {
                        s = q->P.chunk_begin[chunk];
                        s_end = q->P.chunk_begin[chunk + 1];
                        if (RAYS) {
                            const uint32_t* keys = ctr->key_list;
                            pixel = keys ? keys[oi] : oi;
                        } else {
                            pixel = (uint32_t)(py * W + px);
                        }
                        PST_ST(S_ACC, mk3(0, 0, 0));
                        if (s >= s_end) {
                            double* o = q->partial + (size_t)item * 3;
                            o[0] = o[1] = o[2] = 0.0;
                        } else if (RAYS) {
                            load_ray(ctr->ray_list, oi, tr.o, tr.d);
                            state = ST_PRIMARY;
                        } else if (JITTER) {
                            state = TURN ? ST_CACHED : ST_NEW_SAMPLE; // a camera ray of its own per sample (below; TURN: the next pass's turnover)
                        } else {
                            // Camera::GetRay (Camera.cpp:108-117), once per work item: the pixel's one camera ray.  Its direction
                            // is parked next to the hit it is about to find.
                            const d3 ps = mk3(q->C.pixel00[0], q->C.pixel00[1], q->C.pixel00[2]) + (real)px * mk3(q->C.du[0], q->C.du[1], q->C.du[2]) +
                                          (real)py * mk3(q->C.dv[0], q->C.dv[1], q->C.dv[2]);
                            tr.o = mk3(q->C.center[0], q->C.center[1], q->C.center[2]);
                            tr.d = ps - tr.o;
                            if (!PARK_DIR_GLOBAL(FEAT)) {
                                park_real<NPARK>(park, PARK_DIR, tr.d.x);
                                park_real<NPARK>(park, PARK_DIR + PRT_RW, tr.d.y);
                                park_real<NPARK>(park, PARK_DIR + 2 * PRT_RW, tr.d.z);
                            }
                            state = ST_PRIMARY;
                        }
                    }
                }
            }
            if (!TURN && state == ST_NEW_SAMPLE) NEW_SAMPLE(ST_CACHED);
            PROF_MARK(3); // end of sample, item fetch, new sample
            // ---------------- start the traversal this lane needs next
            if (state == ST_CLOSEST || state == ST_SHADOW || state == ST_PRIMARY) {
                // ONE traversal set-up for both kinds of ray (as two divergent call sites every pass executed both, one
                // after the other: -1...2 %, 8 more spilled registers).  Camera / continuation rays: Interval(0.0001, inf),
                // closest hit (Camera.cpp:125).  Shadow rays: Ray(ps, normalize(pl-ps)) (Camera.cpp:143-150); the reference
                // takes the closest hit of Interval(0.001, DBL_MAX) and calls the light visible when that hit is no nearer
                // than dist - 0.001, so only [0.001, dist - 0.001] needs tracing and ANY hit in it settles the question:
                // boxes beyond the light are culled from the start and traversal stops at the first accepted triangle.
                const bool sh_ray = state == ST_SHADOW;
                started = sh_ray ? 2 : 1;
                if (WAVE_DIET && take_next) tr.d = next_d;
                if (COUNT && ctr->ray_dump != nullptr) { // developer experiment: K3's own ray stream, for K1 to replay
                    const unsigned long long k = atomicAdd(&ctr->ray_dump_n, 1ULL);
                    if (k < ctr->ray_dump_cap) {
                        PrtRay r;
                        r.o[0] = (double)tr.o.x; r.o[1] = (double)tr.o.y; r.o[2] = (double)tr.o.z;
                        r.d[0] = (double)tr.d.x; r.d[1] = (double)tr.d.y; r.d[2] = (double)tr.d.z;
                        r.tmin = sh_ray ? 0.001 : 0.0001;
                        r.tmax = sh_ray ? (double)(ldist - RL(0.001)) : __builtin_huge_val();
                        static_cast<PrtRay*>(ctr->ray_dump)[k] = r;
                    }
                }
                tr.start(S, sh_ray ? RL(0.001) : RL(0.0001), sh_ray ? ldist - RL(0.001) : PRT_INF);
            }
        }
        PROF_MARK(4); // traversal set-up
        {
            const unsigned long long nc = (unsigned long long)__popcll(__ballot(started == 1)), ns = (unsigned long long)__popcll(__ballot(started == 2));
            if (lane == 0) atomicAdd(&s_rays[wave], nc | (ns << 32));
        }
        if (__ballot(state != ST_DONE) == 0ULL) break;
        // Lanes that started a sample from the parked hit (TURN: whose sample ended inside the shading blocks, or whose jittered
        // item has just been fetched) have nothing to trace: with enough of them the next pass comes at once (it starts their
        // samples and hands them real rays) instead of after traversal rounds they would sit out.
        if (wave_count(state == ST_CACHED) >= P.cached_min) continue;

        // ---------------- traversal steps until enough lanes have finished to be worth refilling
        if constexpr (WAVE_DIET) {
            // The loop below with its control in scalar code.  Trav::round and the tests around it ask the wave five questions
            // per round (lanes parked, lanes descending, a leaf to test, chained lanes, lanes active), each a __ballot of a bool
            // that lives in a scalar mask across branches: a select and a compare per question (the ballot builtin costs the
            // same; only a mask taken from a comparison IS the comparison's result).  So every mask here is a compare of tr.cur:
            // inside this loop an idle lane holds cur == PRT_NOCUR.  Both steps of Trav drop `active` only with that value,
            // and Trav::start leaves cur = 0 with `active` set (no triangles: not set, hence the two assignments), so
            //   at an inner node  <=>  cur >= 0,    parked at a leaf  <=>  cur > PRT_NOCUR as unsigned,    active  <=>  either.
            // The two masks are taken once after the node visit, the active lanes again after a leaf step; the chain test needs
            // no vector instruction: the lanes in ST_SHADOW whose path goes on change only in a pass or a chain step (m_chain),
            // and `fin` is those of them that are idle.  Same thresholds, same order of node visit, leaf step and chain step,
            // same lanes in each: the schedule is the loop's below, round for round.
            bool sh = state == ST_SHADOW;                                // the lane traces a shadow ray: interval and any-hit rule
            unsigned long long m_chain = lane_mask(sh && cont);          // ... and its path goes on after it
            unsigned long long m_act;
            if (!tr.active) tr.cur = PRT_NOCUR;
            do {
                if (COUNT && lane_mask(tr.cur >= 0) != 0ULL) wc.inner_rounds++;
                if (tr.cur >= 0) tr.template inner_step<COUNT>(S, stk, wc);
                const unsigned long long m_inner = lane_mask(tr.cur >= 0);
                const unsigned long long m_parked = lane_mask((uint32_t)tr.cur > (uint32_t)PRT_NOCUR);
                m_act = m_inner | m_parked;
                if (__popcll(m_parked) >= P.leaf_batch || __popcll(m_inner) <= P.inner_min) {
                    if (COUNT && m_parked != 0ULL) wc.leaf_rounds++;
                    // (the counting instantiations keep test_leaf: with their counters the two-at-a-time loop spills 9 to 10 registers more)
                    if ((uint32_t)tr.cur > (uint32_t)PRT_NOCUR) tr.template leaf_step<COUNT, !COUNT>(S, stk, wc, sh ? RL(0.001) : RL(0.0001), sh);
                    m_act = lane_mask(tr.cur != PRT_NOCUR);
                }
                const unsigned long long m_fin = m_chain & ~m_act; // shadow ray back, path goes on (the loop below's `fin`)
                if (__popcll(m_fin) >= P.chain_min) {
                    PROF_MARK(0);
                    if (tr.cur == PRT_NOCUR && sh && cont) {
                        if (tr.hit.tri < 0) {
                            PST_ST(S_ACC, PST_LD(S_ACC) + pending);
                            TRACE_FLAG_AT(nee_v, PRT_TRACE_VISIBLE);
                        }
                        tr.d = next_d;
                        state = ST_CLOSEST;
                        sh = false;
                        if (COUNT && ctr->ray_dump != nullptr) { // (developer experiment, as at the end of a pass)
                            const unsigned long long k = atomicAdd(&ctr->ray_dump_n, 1ULL);
                            if (k < ctr->ray_dump_cap) {
                                PrtRay r;
                                r.o[0] = (double)tr.o.x; r.o[1] = (double)tr.o.y; r.o[2] = (double)tr.o.z;
                                r.d[0] = (double)tr.d.x; r.d[1] = (double)tr.d.y; r.d[2] = (double)tr.d.z;
                                r.tmin = 0.0001;
                                r.tmax = __builtin_huge_val();
                                static_cast<PrtRay*>(ctr->ray_dump)[k] = r;
                            }
                        }
                        tr.start(S, RL(0.0001), PRT_INF);
                        if (!tr.active) tr.cur = PRT_NOCUR;
                    }
                    if (lane == 0) atomicAdd(&s_rays[wave], (unsigned long long)__popcll(m_fin)); // closest rays: the low half
                    m_chain &= m_act; // the chained lanes have left ST_SHADOW; the others keep their state
                    m_act = lane_mask(tr.cur != PRT_NOCUR);
                    PROF_MARK(5); // chain step
                }
            } while (__popcll(m_act) > P.keep);
            tr.active = tr.cur != PRT_NOCUR; // (what the steps left there: said once, so that the loop itself need not carry it)
        } else
        do {
            // the interval's lower end and the any-hit rule follow from the kind of ray: not kept as traversal state
            tr.template round<COUNT>(S, stk, wc, P.leaf_batch, P.inner_min, state == ST_SHADOW ? RL(0.001) : RL(0.0001), state == ST_SHADOW);
            if (ONE_PASS) {
                // Lanes whose shadow ray has returned and whose path goes on need no pass.  With enough of them to be worth the
                // traversal set-up (executed whole for one lane) they take their light term and start the continuation ray right
                // here; the others are chained by the next pass.  A finished shadow ray only ever becomes an active closest ray,
                // so the loop ends as before.  (Measured: the same step as a pass of its own that only these lanes enter — one
                // set-up site, no second copy of Trav::start in the loop — costs what the chaining gains)
                const bool fin = !tr.active && state == ST_SHADOW && cont;
                const int n_fin = wave_count(fin);
                if (n_fin >= P.chain_min) {
                    PROF_MARK(0);
                    if (fin) {
                        if (tr.hit.tri < 0) {
                            PST_ST(S_ACC, PST_LD(S_ACC) + pending);
                            TRACE_FLAG_AT(nee_v, PRT_TRACE_VISIBLE);
                        }
                        tr.d = next_d;
                        state = ST_CLOSEST;
                        if (COUNT && ctr->ray_dump != nullptr) { // (developer experiment, as at the end of a pass)
                            const unsigned long long k = atomicAdd(&ctr->ray_dump_n, 1ULL);
                            if (k < ctr->ray_dump_cap) {
                                PrtRay r;
                                r.o[0] = (double)tr.o.x; r.o[1] = (double)tr.o.y; r.o[2] = (double)tr.o.z;
                                r.d[0] = (double)tr.d.x; r.d[1] = (double)tr.d.y; r.d[2] = (double)tr.d.z;
                                r.tmin = 0.0001;
                                r.tmax = __builtin_huge_val();
                                static_cast<PrtRay*>(ctr->ray_dump)[k] = r;
                            }
                        }
                        tr.start(S, RL(0.0001), PRT_INF);
                    }
                    if (lane == 0) atomicAdd(&s_rays[wave], (unsigned long long)n_fin); // closest rays: the low half
                    PROF_MARK(5); // chain step
                }
            }
        } while (wave_count(tr.active) > P.keep);
    }

    unsigned long long d = wave_sum((unsigned long long)wc.nodes);
    unsigned long long e = wave_sum((unsigned long long)wc.tris);
    unsigned long long f = wave_sum((unsigned long long)wc.tris_full);
    if (lane == 0) {
        const unsigned long long rays = s_rays[wave];
        atomicAdd(&ctr->rays_closest, rays & 0xffffffffULL);
        atomicAdd(&ctr->rays_shadow, rays >> 32);
        if (COUNT) {
            atomicAdd(&ctr->tri_full, f);
#if PRT_K3_PROFILE
            atomicAdd(&ctr->node_fetches, prof_[5]);
            atomicAdd(&ctr->tri_tests, prof_[0]);
            atomicAdd(&ctr->inner_rounds, prof_[1]);
            atomicAdd(&ctr->leaf_rounds, prof_[2]);
            atomicAdd(&ctr->refills, prof_[3]);
            atomicAdd(&ctr->tri_full, prof_[4]);
#else
            atomicAdd(&ctr->node_fetches, d);
            atomicAdd(&ctr->tri_tests, e);
            atomicAdd(&ctr->inner_rounds, (unsigned long long)wc.inner_rounds);
            atomicAdd(&ctr->leaf_rounds, (unsigned long long)wc.leaf_rounds);
            atomicAdd(&ctr->refills, (unsigned long long)n_refills);
#endif
        }
    }
}

#if !PRT_F32_TU
// ------------------------------------------------------------------------------------------- K5
// Sum over the chunks (fixed order) of owned item oi's partial sums: the one summation k_finalize and k_accumulate share.
PRT_DEV void chunk_sum(const DRenderParams& P, const double* __restrict__ partial, uint64_t oi, double& r, double& g, double& b) {
    r = 0, g = 0, b = 0;
    for (int c = 0; c < P.chunks; ++c) {
        const double* p = partial + ((uint64_t)c * P.items_per_chunk + oi) * 3;
        r += p[0];
        g += p[1];
        b += p[2];
    }
}

// out[pixel] = sum over chunks (fixed order) of the item partial sums; pixels of other ranks' tiles
// were zeroed by a memset so that the cross-rank sum is exact.
__global__ void k_finalize(DCamera C, DRenderParams P, const double* __restrict__ partial, double* __restrict__ out64,
                           float* __restrict__ out32) {
    const uint64_t oi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (oi >= P.items_per_chunk) return;
    int px, py;
    if (!owned_to_pixel(P, C, oi, px, py)) return;
    double r, g, b;
    chunk_sum(P, partial, oi, r, g, b);
    const size_t m = ((size_t)py * C.width + px) * 3;
    if (out64) {
        out64[m] = r;
        out64[m + 1] = g;
        out64[m + 2] = b;
    }
    if (out32) {
        out32[m] = (float)r;
        out32[m + 1] = (float)g;
        out32[m + 2] = (float)b;
    }
}

// prt_ray_color: out[i] = the same sum for ray i of a batch (item c * n + i of chunk c); no pixel mapping, no other ranks.
__global__ void k_finalize_rays(DRenderParams P, const double* __restrict__ partial, double* __restrict__ out64, float* __restrict__ out32) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.items_per_chunk) return;
    double r, g, b;
    chunk_sum(P, partial, i, r, g, b);
    if (out64) {
        out64[i * 3] = r;
        out64[i * 3 + 1] = g;
        out64[i * 3 + 2] = b;
    }
    if (out32) {
        out32[i * 3] = (float)r;
        out32[i * 3 + 1] = (float)g;
        out32[i * 3 + 2] = (float)b;
    }
}

// Progressive rendering (prt_accum_render): sum[pixel] += the pass's item sum, taken over the chunks exactly as
// k_finalize takes it.  The pass ran with spp = 1, so items hold raw sums of RayColor.  One thread per owned item, so
// every pixel has one writer and no atomic is needed (the sums are deterministic); other ranks' pixels are not touched.
__global__ void k_accumulate(DCamera C, DRenderParams P, const double* __restrict__ partial, double* __restrict__ sum) {
    const uint64_t oi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (oi >= P.items_per_chunk) return;
    int px, py;
    if (!owned_to_pixel(P, C, oi, px, py)) return;
    double r, g, b;
    chunk_sum(P, partial, oi, r, g, b);
    const size_t m = ((size_t)py * C.width + px) * 3;
    sum[m] += r;
    sum[m + 1] += g;
    sum[m + 2] += b;
}

__global__ void k_sample_lights(DScene S, const double* __restrict__ origins, size_t n, uint64_t seed,
                                PrtLightSample* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng.seed(seed, i, 0);
    const LightPick lp = sample_lights<false, true>(S, mk3(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]), rng);
    PrtLightSample o;
    o.position[0] = lp.pos.x; o.position[1] = lp.pos.y; o.position[2] = lp.pos.z;
    o.normal[0] = lp.n.x; o.normal[1] = lp.n.y; o.normal[2] = lp.n.z;
    o.pdf = lp.pdf;
    o.prim = S.light_tris[lp.tri].prim;
    o.front = lp.front ? 1 : 0;
    out[i] = o;
}

// Test hooks for the material arithmetic (prt_material_eval / prt_material_scatter / prt_texture_value): the device
// functions K3 shades with, on caller-supplied directions; item i draws from the stream keyed (seed, i, 0).
__global__ void k_material_eval(DScene S, int material, const double* __restrict__ wi, const double* __restrict__ wo,
                                const double* __restrict__ uv, size_t n, uint64_t seed, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng.seed(seed, i, 0);
    const d2 t = uv ? d2{uv[i * 2], uv[i * 2 + 1]} : d2{0., 0.};
    const d3 f = mat_eval<PRT_FEAT_ALL | PRT_FEAT_EXTRA>(S, S.materials[material], ld3(wi + i * 3), ld3(wo + i * 3), t, rng);
    out[i * 3] = f.x; out[i * 3 + 1] = f.y; out[i * 3 + 2] = f.z;
}
__global__ void k_material_scatter(DScene S, int material, const double* __restrict__ rd, d3 normal, d3 tangent,
                                   const double* __restrict__ uv, size_t n, uint64_t seed, double* __restrict__ wi_out,
                                   double* __restrict__ att_out, int32_t* __restrict__ ok_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng.seed(seed, i, 0);
    const Frame f{normal, tangent};
    const d2 t = uv ? d2{uv[i * 2], uv[i * 2 + 1]} : d2{0., 0.};
    d3 att = mk3(0, 0, 0), wi = mk3(0, 0, 0);
    const bool ok = mat_scatter<PRT_FEAT_ALL | PRT_FEAT_EXTRA>(S, S.materials[material], ld3(rd + i * 3), f, t, rng, att, wi);
    ok_out[i] = ok ? 1 : 0;
    wi_out[i * 3] = ok ? wi.x : 0.; wi_out[i * 3 + 1] = ok ? wi.y : 0.; wi_out[i * 3 + 2] = ok ? wi.z : 0.;
    att_out[i * 3] = ok ? att.x : 0.; att_out[i * 3 + 1] = ok ? att.y : 0.; att_out[i * 3 + 2] = ok ? att.z : 0.;
}
__global__ void k_texture_value(DScene S, int texture, const double* __restrict__ uv, size_t n, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const d3 c = tex_value<true>(S, texture, uv[i * 2], uv[i * 2 + 1]);
    out[i * 3] = c.x; out[i * 3 + 1] = c.y; out[i * 3 + 2] = c.z;
}

// Camera::WriteColorAttachment's per-pixel transform (Camera.cpp:279-301): NaN -> 0, LinearToSRGB
// (:214-221), clamp to [0, 0.9999], * 255 truncated to uint8.  Shared by k_tonemap and k_resolve.
PRT_DEV uint8_t srgb8_of(float x) {
    double v = (double)x;
    if (v != v) v = 0.0;
    double sv = (v <= 0.0031308) ? 12.92 * v : 1.055 * pow(v, (1. / 2.4)) - 0.055;
    sv = sv < 0.0 ? 0.0 : (sv > 0.9999 ? 0.9999 : sv);
    return (uint8_t)(sv * 255);
}
__global__ void k_tonemap(const float* __restrict__ in, size_t n, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = srgb8_of(in[i]);
}

// Progressive rendering (prt_accum_resolve): the frame of `samples` accumulated samples, element-wise over the n
// reals of the full frame: sum / samples in fp64, the fp32 frame its rounding, the 8-bit sRGB frame k_tonemap's bytes of
// that fp32 value.  An accumulator without samples resolves to zeros.  Memory-bound: grid-stride over a capped grid.
// Adaptive accumulators pass `counts` (one per pixel, n / 3 of them): each pixel is divided by its own count instead.
__global__ void k_resolve(const double* __restrict__ sum, size_t n, uint64_t samples, const uint32_t* __restrict__ counts,
                          double* __restrict__ out64, float* __restrict__ out32, uint8_t* __restrict__ out8) {
    const double ns = (double)samples;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t c = counts ? counts[i / 3] : 0u;
        const double v = counts ? (c ? sum[i] / (double)c : 0.0) : (samples ? sum[i] / ns : 0.0);
        const float f = (float)v;
        if (out64) out64[i] = v;
        if (out32) out32[i] = f;
        if (out8) out8[i] = srgb8_of(f);
    }
}

// ------------------------------------------------------------------------------------------- adaptive sampling
// prt_accum_render_adaptive (include/prt.h).  Memory-bound over the owned pixels, like K5.  The rule and the moments are
// evaluated without fused multiply-adds, so that a host-side restatement of them (tests/adaptive_model.py) computes the
// same bits from the same sums.
PRT_DEV double luma(double r, double g, double b) {
#pragma clang fp contract(off)
    return 0.2126 * r + 0.7152 * g + 0.0722 * b;
}

// Batch means: the unbiased per-sample luminance variance of a pixel with c samples, var = max(0, moment - S^2 / c) /
// (c / batch - 1); S = Y(sum) is returned too.  c >= 2 * batch.
PRT_DEV double adapt_variance(const double* __restrict__ sum, const double* __restrict__ moment, uint32_t c, uint32_t batch,
                              uint32_t pix, double& S) {
#pragma clang fp contract(off)
    S = luma(sum[(size_t)pix * 3], sum[(size_t)pix * 3 + 1], sum[(size_t)pix * 3 + 2]);
    const double d = moment[pix] - S * S / (double)c;
    return (d < 0.0 ? 0.0 : d) / (double)(c / batch - 1u);
}

// The activity rule: count == n, count < max_spp and not (count >= min_spp and converged).  Batch means: C = count / batch
// batches of equal size, var = max(0, moment - S^2 / count) / (C - 1) estimates the per-sample luminance variance, and
// the pixel has converged when sqrt(var / count) <= max(rel_tol |mean|, abs_tol).  Every comparison is false for NaN,
// so a NaN pixel never converges.
PRT_DEV bool adapt_active(const DAdaptRule& R, const double* __restrict__ sum, const double* __restrict__ moment,
                          const uint32_t* __restrict__ count, uint32_t pix) {
#pragma clang fp contract(off)
    const uint32_t c = count[pix];
    if (c != R.n || c >= R.max_spp) return false;
    if (c < R.min_spp) return true;
    const double np = (double)c;
    double S;
    const double var = adapt_variance(sum, moment, c, R.batch, pix, S);
    const double se = sqrt(var / np);
    double thr = R.rel_tol * fabs(S / np);
    if (thr < R.abs_tol) thr = R.abs_tol;
    return !(se <= thr);
}

// Owned item oi of the tile order is an active pixel; its index j*W+i in `pix`.
PRT_DEV bool adapt_item(const DCamera& C, const DRenderParams& P, const DAdaptRule& R, const double* __restrict__ sum,
                        const double* __restrict__ moment, const uint32_t* __restrict__ count, uint64_t oi, uint32_t& pix) {
    int px, py;
    if (oi >= P.items_per_chunk || !owned_to_pixel(P, C, (uint32_t)oi, px, py)) return false;
    pix = (uint32_t)(py * C.width + px);
    return adapt_active(R, sum, moment, count, pix);
}

// The active pixels, compacted in owned-item order by three kernels (no atomics: the list is the same on every run).
// Segment g = owned items [g * PRT_BLOCK, (g + 1) * PRT_BLOCK), one per thread of a block; blocks stride over segments.
// (1) seg[g] = active items of segment g.
__global__ void k_adapt_count(DCamera C, DRenderParams P, DAdaptRule R, const double* __restrict__ sum,
                              const double* __restrict__ moment, const uint32_t* __restrict__ count, uint32_t* __restrict__ seg,
                              uint32_t n_seg) {
    for (uint32_t g = blockIdx.x; g < n_seg; g += gridDim.x) {
        uint32_t pix;
        const bool a = adapt_item(C, P, R, sum, moment, count, (uint64_t)g * PRT_BLOCK + threadIdx.x, pix);
        const int k = __syncthreads_count(a);
        if (threadIdx.x == 0) seg[g] = (uint32_t)k;
    }
}
// (2) One block of PRT_ADAPT_SCAN threads: seg[] becomes its exclusive prefix sum, *total the number of active pixels.
#define PRT_ADAPT_SCAN 1024
__global__ void __launch_bounds__(PRT_ADAPT_SCAN) k_adapt_scan(uint32_t* __restrict__ seg, uint32_t n_seg, uint32_t* __restrict__ total) {
    __shared__ uint32_t s[PRT_ADAPT_SCAN];
    const uint32_t t = threadIdx.x, per = (n_seg + PRT_ADAPT_SCAN - 1) / PRT_ADAPT_SCAN;
    const uint32_t b = min(n_seg, t * per), e = min(n_seg, b + per);
    uint32_t mine = 0;
    for (uint32_t g = b; g < e; ++g) mine += seg[g];
    s[t] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < PRT_ADAPT_SCAN; off *= 2) { // inclusive scan (Hillis-Steele)
        const uint32_t v = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    uint32_t run = s[t] - mine;
    for (uint32_t g = b; g < e; ++g) {
        const uint32_t v = seg[g];
        seg[g] = run;
        run += v;
    }
    if (t == PRT_ADAPT_SCAN - 1) *total = s[t];
}
// (3) list[seg[g] + rank of the item among the active ones of its segment] = pixel.
__global__ void k_adapt_write(DCamera C, DRenderParams P, DAdaptRule R, const double* __restrict__ sum,
                              const double* __restrict__ moment, const uint32_t* __restrict__ count,
                              const uint32_t* __restrict__ seg, uint32_t n_seg, int32_t* __restrict__ list) {
    __shared__ uint32_t s_wave[PRT_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t g = blockIdx.x; g < n_seg; g += gridDim.x) {
        uint32_t pix = 0;
        const bool a = adapt_item(C, P, R, sum, moment, count, (uint64_t)g * PRT_BLOCK + threadIdx.x, pix);
        const unsigned long long m = __ballot(a);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t at = seg[g] + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL));
        for (uint32_t w = 0; w < wave; ++w) at += s_wave[w];
        if (a) list[at] = (int32_t)pix;
        __syncthreads(); // s_wave is reused by the next segment
    }
}

// prt_accum_variance: the variance of each pixel's mean luminance, var / count in fp64 rounded to fp32; 0 where the count
// is 0 (a pixel of another rank, or nothing rendered yet).
__global__ void k_accum_variance(const double* __restrict__ sum, const double* __restrict__ moment, const uint32_t* __restrict__ count,
                                 uint32_t npx, uint32_t batch, float* __restrict__ out) {
#pragma clang fp contract(off)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = count[i];
        double S;
        out[i] = c ? (float)(adapt_variance(sum, moment, c, batch, (uint32_t)i, S) / (double)c) : 0.f;
    }
}

// One adaptive launch: for list entry i, sum[pixel] += the item sum over the chunks (chunk_sum, as k_accumulate takes it),
// moment[pixel] += sum over the chunks, in order, of Y(chunk partial)^2 / batch, count[pixel] += the launch's samples.
// One thread per entry, and a pixel is listed once: one writer per pixel, no atomics.
__global__ void k_accumulate_list(DRenderParams P, const double* __restrict__ partial, const int32_t* __restrict__ list,
                                  uint32_t batch, uint32_t samples, double* __restrict__ sum, double* __restrict__ moment,
                                  uint32_t* __restrict__ count) {
#pragma clang fp contract(off)
    const double b = (double)batch;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.items_per_chunk; i += (uint64_t)gridDim.x * blockDim.x) {
        const size_t pix = (size_t)list[i];
        double r, g, bl;
        chunk_sum(P, partial, i, r, g, bl);
        double m = 0.0;
        for (int c = 0; c < P.chunks; ++c) {
            const double* p = partial + ((uint64_t)c * P.items_per_chunk + i) * 3;
            const double t = luma(p[0], p[1], p[2]);
            m += t * t / b;
        }
        sum[pix * 3] += r;
        sum[pix * 3 + 1] += g;
        sum[pix * 3 + 2] += bl;
        moment[pix] += m;
        count[pix] += samples;
    }
}

// ------------------------------------------------------------------------------------------- feature buffers
// prt_render_features (include/prt.h): the first-hit features a denoiser is guided by.  One thread per pixel; sample s of the
// pixel is K3's camera ray of sample s (the pixel centre, or with jitter the SampleSquare offset drawn as the first two numbers
// of the stream keyed (seed, j*W+i, s)), traced with the closest-hit traversal K1 and K3 use.  Without jitter every sample is
// the same ray: it is traced once and its features are the means.  Sums are fp64, the outputs their fp32 rounding.
template <bool PAD>
__global__ __launch_bounds__(PRT_BLOCK) void k_features(DScene S, DCamera C, uint64_t seed_key, int jitter, int spp,
                                                        float* __restrict__ albedo, float* __restrict__ normal,
                                                        float* __restrict__ depth, int32_t* __restrict__ prim) {
    __shared__ uint32_t s_stack[PRT_BLOCK / 64][PRT_STACK_DEPTH][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* stk = &s_stack[wave][0][lane];
    const uint32_t W = (uint32_t)C.width, npx = W * (uint32_t)C.height;
    const uint32_t pix = blockIdx.x * PRT_BLOCK + threadIdx.x;
    const bool valid = pix < npx;
    const int py = valid ? (int)(pix / W) : 0, px = valid ? (int)(pix - (uint32_t)py * W) : 0;
    const d3 center = mk3(C.center[0], C.center[1], C.center[2]);
    const d3 p00 = mk3(C.pixel00[0], C.pixel00[1], C.pixel00[2]), du = mk3(C.du[0], C.du[1], C.du[2]), dv = mk3(C.dv[0], C.dv[1], C.dv[2]);
    d3 a_sum = mk3(0, 0, 0), n_sum = mk3(0, 0, 0);
    double z_sum = 0.0;
    int n_hit = 0;
    int32_t prim0 = -1;
    WorkCount wc{0, 0, 0, 0, 0};
    Trav<PAD> tr;
    const int traced = jitter ? spp : 1; // wave-uniform
    for (int s = 0; s < traced; ++s) {
        real fx = (real)px, fy = (real)py;
        if (jitter) {
            Rng rng;
            rng.seed_keyed(seed_key, (uint64_t)pix, (uint64_t)s);
            fy = fy + (rng.next() - RL(0.5)); // offset.y first, as K3 draws it
            fx = fx + (rng.next() - RL(0.5));
        }
        const d3 ps = p00 + fx * du + fy * dv;
        tr.init(S, center, ps - center, RL(0.0001), PRT_INF);
        tr.hit.alpha = tr.hit.beta = RL(0.0);
        if (!valid) tr.active = false;
        while (__ballot(tr.active) != 0ULL) tr.template round<false>(S, stk, wc, PRT_LEAF_BATCH, PRT_INNER_MIN, RL(0.0001), false);
        if (!valid) continue;
        if (s == 0) prim0 = tr.hit.tri >= 0 ? S.shade[tr.hit.tri].prim : -1;
        if (tr.hit.tri < 0) {
            a_sum = a_sum + mk3(1, 1, 1);
            continue;
        }
        const DTriShade* sh = S.shade + tr.hit.tri;
        const DMaterial& m = S.materials[sh->material];
        const d3 gn = ld3(tri_at<PAD>(S, (uint32_t)tr.hit.tri)->n);
        const d3 fn = face_normal(tr.d, gn); // SetFaceNormal, as make_ctx
        const d2 uv = hit_uv(sh, tr.hit.alpha, tr.hit.beta);
        const d3 a = feature_albedo<PRT_FEAT_ALL | PRT_FEAT_EXTRA>(S, m, uv);
        a_sum = a_sum + a;
        n_sum = n_sum + fn;
        z_sum += (double)tr.hit.t * sqrt((double)dot(tr.d, tr.d)); // world distance: d is not normalised
        n_hit++;
    }
    if (!valid) return;
    const real nt = (real)traced; // means over the traced samples (the untraced ones repeat the one ray)
    if (albedo) {
        albedo[(size_t)pix * 3] = (float)(a_sum.x / nt);
        albedo[(size_t)pix * 3 + 1] = (float)(a_sum.y / nt);
        albedo[(size_t)pix * 3 + 2] = (float)(a_sum.z / nt);
    }
    if (normal) {
        normal[(size_t)pix * 3] = (float)(n_sum.x / nt);
        normal[(size_t)pix * 3 + 1] = (float)(n_sum.y / nt);
        normal[(size_t)pix * 3 + 2] = (float)(n_sum.z / nt);
    }
    if (depth) depth[pix] = n_hit ? (float)(z_sum / (double)n_hit) : __builtin_huge_valf();
    if (prim) prim[pix] = prim0;
}

// dst += src (fp32 framebuffers of tile shares that live on ONE device: disjoint tiles, so every element is x + 0)
__global__ void k_add_f32(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

#endif // !PRT_F32_TU

} // namespace

// ------------------------------------------------------------------------------------------- launchers
namespace PRT_NS {

// The compiled permutations: lean, textures only, Phong only, CookTorrance only, everything.  A scene gets the smallest one
// that covers its materials.
int render_permutation(int feat) {
    feat &= ~(PRT_FEAT_RAYS | PRT_FEAT_PLAIN | PRT_FEAT_DIFFUSE); // (not material features: the ray source of prt_ray_color, the PLAIN form and its DIFFUSE form)
    if (feat == 0 || feat == PRT_FEAT_TEX || feat == PRT_FEAT_PHONG || feat == PRT_FEAT_CT) return feat;
    return PRT_FEAT_ALL;
}

// Bytes of LDS a block may spend on shading tables next to its traversal stacks without costing a resident block:
// 160 KB per CU, `blocks` resident blocks (4 waves per block, 4 SIMDs per CU: blocks per CU = waves per SIMD).
int render_lds_budget(int feat, int stack_depth) {
    int blocks = render_waves(render_permutation(feat));
    if (PRT_F32_TU && stack_depth <= 32) blocks = PRT_F32_WAVES > 4 && stack_depth <= 24 ? 5 : 4; // fp32: registers allow a fourth wave per SIMD when the stacks do
    const int perm = render_permutation(feat);
    return ((160 * 1024 / blocks - (int)sizeof(uint32_t) * (stack_depth + PARK_WORDS(perm)) * PRT_BLOCK - 256) / 512) * 512; // stacks + parked camera rays
}
size_t render_table_bytes(int light_lds, int mat_lds, int ltri_lds) {
    return (size_t)light_lds * sizeof(DLightNode) + (size_t)mat_lds * sizeof(DMaterial) + (size_t)ltri_lds * sizeof(DLightTri);
}

typedef void (*RenderKernel)(RenderArgs);
// The permutations that have a PLAIN form of k_render: the fp64 ones except the textured one, whose PLAIN form measured 1.4 %
// SLOWER than its generic kernel on bathroom2; no fp32 kernel gained from it (all bit-identical).
constexpr bool plain_permutation(int perm) { return !PRT_F32_TU && perm != PRT_FEAT_TEX; }
// THE decision between the two forms of a launch's kernel, from the values the generic kernel tests at run time (k_render,
// PLAIN): prt_api.cpp asks here, for the occupancy query and for the launch, and hands the answer to both as `plain`.
bool render_plain(int feat, bool count, bool rays, int n_lights, int ltri_lds, int jitter, int scramble, int sample_lights) {
    return plain_permutation(render_permutation(feat)) && !count && !rays && n_lights > 0 && ltri_lds > 0 && !jitter &&
           scramble != PRT_ITEMS_FROM_LIST && sample_lights;
}
// The permutation whose PLAIN form has a DIFFUSE form: the lean fp64 one (the fp32 twin has no PLAIN form and gets none).
constexpr bool diffuse_permutation(int perm) { return plain_permutation(perm) && perm == 0; }
// ... and THE decision for it (k_render, DIFFUSE): a PLAIN launch of the lean permutation in a scene whose material table says
// so (`all_diffuse`: every material an untextured Lambertian or an emitter, none skipping light sampling — computed by the host
// where the table is made, never per launch).  prt_api.cpp asks here, for the occupancy query and for the launch.
bool render_diffuse(int feat, bool count, bool rays, int n_lights, int ltri_lds, int jitter, int scramble, int sample_lights, bool all_diffuse) {
    return render_plain(feat, count, rays, n_lights, ltri_lds, jitter, scramble, sample_lights) && diffuse_permutation(render_permutation(feat)) &&
           all_diffuse;
}
// COUNT instantiations exist only with PRT_FEAT_EXTRA (statistics runs: speed is not what they are for); so do the
// PRT_FEAT_RAYS ones (prt_ray_color: one kernel per permutation and layout, no counting form).  PLAIN ones exist with LDS
// tables only (render_plain asks for the light triangles there), with and without PRT_FEAT_EXTRA; so do the DIFFUSE ones.
template <int FEAT, bool PAD>
static RenderKernel render_kernel_feat(bool count, bool llds, bool extra, bool rays, bool plain, bool diffuse) {
    constexpr int X = FEAT | PRT_FEAT_EXTRA;
    if constexpr (diffuse_permutation(FEAT)) {
        constexpr int D = PRT_FEAT_PLAIN | PRT_FEAT_DIFFUSE;
        if (plain && diffuse) return extra ? k_render<false, X | D, true, PAD> : k_render<false, FEAT | D, true, PAD>;
    }
    if constexpr (plain_permutation(FEAT)) {
        if (plain) return extra ? k_render<false, X | PRT_FEAT_PLAIN, true, PAD> : k_render<false, FEAT | PRT_FEAT_PLAIN, true, PAD>;
    }
    if (rays) return llds ? k_render<false, X | PRT_FEAT_RAYS, true, PAD> : k_render<false, X | PRT_FEAT_RAYS, false, PAD>;
    if (count) return llds ? k_render<true, X, true, PAD> : k_render<true, X, false, PAD>;
    if (extra) return llds ? k_render<false, X, true, PAD> : k_render<false, X, false, PAD>;
    return llds ? k_render<false, FEAT, true, PAD> : k_render<false, FEAT, false, PAD>;
}
template <bool PAD>
static RenderKernel render_kernel_pad(bool count, int feat, bool llds, bool extra) {
    const bool rays = (feat & PRT_FEAT_RAYS) != 0;
    const bool plain = (feat & PRT_FEAT_PLAIN) != 0 && llds && !count && !rays; // (what render_plain implies: said again for the instantiations' sake)
    const bool diffuse = plain && (feat & PRT_FEAT_DIFFUSE) != 0;
    switch (render_permutation(feat)) {
    case 0: return render_kernel_feat<0, PAD>(count, llds, extra, rays, plain, diffuse);
    case PRT_FEAT_TEX: return render_kernel_feat<PRT_FEAT_TEX, PAD>(count, llds, extra, rays, plain, diffuse);
    case PRT_FEAT_PHONG: return render_kernel_feat<PRT_FEAT_PHONG, PAD>(count, llds, extra, rays, plain, diffuse);
    case PRT_FEAT_CT: return render_kernel_feat<PRT_FEAT_CT, PAD>(count, llds, extra, rays, plain, diffuse);
    default: return render_kernel_feat<PRT_FEAT_ALL, PAD>(count, llds, extra, rays, plain, diffuse);
    }
}
// `pad`: the scene's intersection records sit 128 bytes apart (DScene::tri_stride); `extra`: the scene has light tables or
// plain texel arrays (PRT_FEAT_EXTRA kernels); `feat` with PRT_FEAT_RAYS: the kernel of prt_ray_color; with PRT_FEAT_PLAIN: the
// PLAIN form (render_plain said so); with PRT_FEAT_DIFFUSE as well: its DIFFUSE form (render_diffuse said so)
static RenderKernel render_kernel(bool count, int feat, bool llds, bool pad, bool extra) {
    return pad ? render_kernel_pad<true>(count, feat, llds, extra) : render_kernel_pad<false>(count, feat, llds, extra);
}

static size_t stack_bytes(int stack_depth) { return PRT_DYN_STACK ? (size_t)PRT_BLOCK * stack_depth * sizeof(uint32_t) : 0; }

// Resident blocks per CU of the instantiation a launch will use (`pad`: the scene's records sit at the padded stride —
// a different function with its own register count).
int render_blocks_per_cu(bool count, int feat, size_t table_bytes, int stack_depth, bool pad, bool extra, bool rays, bool plain, bool diffuse) {
    int nb = 0;
    if (rays) feat |= PRT_FEAT_RAYS;
    if (plain) feat |= PRT_FEAT_PLAIN;
    if (diffuse) feat |= PRT_FEAT_DIFFUSE;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, render_kernel(count, feat, table_bytes != 0, pad, extra), PRT_BLOCK,
                                                                table_bytes + stack_bytes(stack_depth));
    if (e != hipSuccess || nb < 1) nb = 1;
    return nb;
}

// One batch of rays through K1: `mode` (PRT_TRACE_*, prt_types.h) picks the closest-hit form (d_out = one PrtHit per ray), the
// any-hit form (one byte per ray) or the surface form (one PrtSurface per ray, 32-byte aligned).  Returns hipGetLastError()
// behind the launch (an empty batch launches nothing and still polls, as its callers always have).
hipError_t launch_trace(const DScene& S, const PrtRay* d_rays, size_t n, void* d_out, DCounters* d_ctr, bool count, int mode,
                        int n_cu, hipStream_t st, const uint32_t* d_perm) {
    if (n == 0) return hipGetLastError();
    size_t want = (n + PRT_BLOCK - 1) / PRT_BLOCK;
    const size_t per_cu = std::max<size_t>(1, (160u * 1024u) / (sizeof(uint32_t) * PRT_STACK_DEPTH * PRT_BLOCK)); // LDS stacks per CU
    unsigned grid = (unsigned)std::min<size_t>(want, (size_t)n_cu * per_cu);
    const bool pad = S.tri_stride == PRT_TRI_PAD_STRIDE(real) && sizeof(DTri) != PRT_TRI_PAD_STRIDE(real);
    const bool any_hit = mode == PRT_TRACE_ANY;
    const int pick = (count ? 4 : 0) | (pad ? 2 : 0) | (any_hit ? 1 : 0);
    auto go = [&](auto k, auto* out) {
        hipLaunchKernelGGL(k, dim3(grid), dim3(PRT_BLOCK), 0, st, S, d_rays, n, out, d_ctr, d_perm);
        return hipGetLastError();
    };
    PrtHit* hits = static_cast<PrtHit*>(d_out);
    uint8_t* bytes = static_cast<uint8_t*>(d_out);
    if (mode == PRT_TRACE_SURFACE) {
        PrtSurface* recs = static_cast<PrtSurface*>(d_out);
        switch (pick >> 1) {
        case 0: return go(k_trace_surface<false, false>, recs);
        case 1: return go(k_trace_surface<false, true>, recs);
        case 2: return go(k_trace_surface<true, false>, recs);
        default: return go(k_trace_surface<true, true>, recs);
        }
    }
    switch (pick) {
    case 0: return go(k_trace<false, false, false>, hits);
    case 1: return go(k_trace<false, false, true>, bytes);
    case 2: return go(k_trace<false, true, false>, hits);
    case 3: return go(k_trace<false, true, true>, bytes);
    case 4: return go(k_trace<true, false, false>, hits);
    case 5: return go(k_trace<true, false, true>, bytes);
    case 6: return go(k_trace<true, true, false>, hits);
    default: return go(k_trace<true, true, true>, bytes);
    }
}

// `rays`: the ray-batch kernels (prt_ray_color; DCounters::ray_list / key_list are set, C is not read)
void launch_render(const DScene& S, const DCamera& C, const DRenderParams& P, double* d_partial, DCounters* d_ctr,
                   bool count, int feat, unsigned grid, hipStream_t st, bool rays, bool plain, bool diffuse) {
    static_assert(sizeof(DMaterial) % 16 == 0, "materials are staged in 16-byte pieces");
    const size_t tables = render_table_bytes(P.light_lds, P.mat_lds, P.ltri_lds);
    const size_t dyn_lds = tables + stack_bytes(P.stack_depth);
    const bool pad = S.tri_stride == PRT_TRI_PAD_STRIDE(real) && sizeof(DTri) != PRT_TRI_PAD_STRIDE(real);
    RenderArgs A;
    A.S = S;
    A.C = C;
    A.P = P;
    A.partial = d_partial;
    A.ctr = d_ctr;
    if (rays) feat |= PRT_FEAT_RAYS;
    if (plain) feat |= PRT_FEAT_PLAIN;
    if (diffuse) feat |= PRT_FEAT_DIFFUSE;
    hipLaunchKernelGGL(render_kernel(count, feat, tables != 0, pad, S.light_tab != nullptr || S.tex_compact != 0), dim3(grid), dim3(PRT_BLOCK), dyn_lds, st, A);
}

#if PRT_F32_TU
// ------------------------------------------------------------------------------------------- fp64 -> fp32 tables
// The fp32 records are derived on the device from the resident fp64 ones (which are already in BVH leaf order for
// either builder): one thread per record, each value rounded to nearest.
namespace {
__global__ void k_convert_tris(const char* __restrict__ in, uint32_t in_stride, uint32_t n, char* __restrict__ out, uint32_t out_stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* a = reinterpret_cast<const double*>(in + (size_t)i * in_stride);
    float4* o = reinterpret_cast<float4*>(out + (size_t)i * out_stride);
    static_assert(sizeof(DTriT<double>) % 32 == 0 && sizeof(DTriT<float>) * 2 == sizeof(DTriT<double>), "same fields, half the size");
    for (uint32_t k = 0; k < sizeof(DTriT<float>) / 16; ++k)
        o[k] = make_float4((float)a[4 * k], (float)a[4 * k + 1], (float)a[4 * k + 2], (float)a[4 * k + 3]);
}
__global__ void k_convert_shade(const DTriShadeT<double>* __restrict__ in, uint32_t n, DTriShadeT<float>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DTriShadeT<double> a = in[i];
    DTriShadeT<float> o;
    for (int k = 0; k < 3; ++k) o.tangent[k] = (float)a.tangent[k];
    for (int k = 0; k < 2; ++k) {
        o.uv0[k] = (float)a.uv0[k];
        o.uv1[k] = (float)a.uv1[k];
        o.uv2[k] = (float)a.uv2[k];
    }
    o.material = a.material;
    o.prim = a.prim;
    o.pad[0] = 0.f;
    out[i] = o;
}
__global__ void k_convert_reals(const double* __restrict__ in, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
} // namespace
void launch_convert_tris(const void* in, uint32_t in_stride, uint32_t n, void* out, uint32_t out_stride, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_convert_tris, dim3((n + 255) / 256), dim3(256), 0, st, static_cast<const char*>(in), in_stride, n, static_cast<char*>(out), out_stride);
}
void launch_convert_shade(const DTriShadeT<double>* in, uint32_t n, DTriShadeT<float>* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_convert_shade, dim3((n + 255) / 256), dim3(256), 0, st, in, n, out);
}
void launch_convert_reals(const double* in, size_t n, float* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_convert_reals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n, out);
}
#endif // PRT_F32_TU

#if !PRT_F32_TU
void launch_finalize(const DCamera& C, const DRenderParams& P, const double* d_partial, double* d64, float* d32,
                     hipStream_t st) {
    unsigned grid = (unsigned)((P.items_per_chunk + 255) / 256);
    if (grid == 0) return;
    hipLaunchKernelGGL(k_finalize, dim3(grid), dim3(256), 0, st, C, P, d_partial, d64, d32);
}
void launch_finalize_rays(const DRenderParams& P, const double* d_partial, double* d64, float* d32, hipStream_t st) {
    unsigned grid = (unsigned)((P.items_per_chunk + 255) / 256);
    if (grid == 0) return;
    hipLaunchKernelGGL(k_finalize_rays, dim3(grid), dim3(256), 0, st, P, d_partial, d64, d32);
}
void launch_accumulate(const DCamera& C, const DRenderParams& P, const double* d_partial, double* d_sum, hipStream_t st) {
    unsigned grid = (unsigned)((P.items_per_chunk + 255) / 256);
    if (grid == 0) return;
    hipLaunchKernelGGL(k_accumulate, dim3(grid), dim3(256), 0, st, C, P, d_partial, d_sum);
}
void launch_resolve(const double* d_sum, size_t n, uint64_t samples, const uint32_t* d_counts, double* d64, float* d32,
                    uint8_t* d8, hipStream_t st) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_resolve, dim3(grid), dim3(256), 0, st, d_sum, n, samples, d_counts, d64, d32, d8);
}
uint32_t adapt_segments(uint64_t owned_items) { return (uint32_t)((owned_items + PRT_BLOCK - 1) / PRT_BLOCK); }
void launch_adapt_select(const DCamera& C, const DRenderParams& P, const DAdaptRule& R, const double* d_sum,
                         const double* d_moment, const uint32_t* d_count, uint32_t* d_seg, int32_t* d_list, uint32_t* d_total,
                         hipStream_t st) {
    const uint32_t n_seg = adapt_segments(P.items_per_chunk);
    if (n_seg == 0) {
        (void)hipMemsetAsync(d_total, 0, sizeof(uint32_t), st);
        return;
    }
    const unsigned grid = std::min<uint32_t>(n_seg, 2048);
    hipLaunchKernelGGL(k_adapt_count, dim3(grid), dim3(PRT_BLOCK), 0, st, C, P, R, d_sum, d_moment, d_count, d_seg, n_seg);
    hipLaunchKernelGGL(k_adapt_scan, dim3(1), dim3(PRT_ADAPT_SCAN), 0, st, d_seg, n_seg, d_total);
    hipLaunchKernelGGL(k_adapt_write, dim3(grid), dim3(PRT_BLOCK), 0, st, C, P, R, d_sum, d_moment, d_count, d_seg, n_seg, d_list);
}
void launch_accumulate_list(const DRenderParams& P, const double* d_partial, const int32_t* d_list, uint32_t batch,
                            uint32_t samples, double* d_sum, double* d_moment, uint32_t* d_count, hipStream_t st) {
    if (P.items_per_chunk == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((P.items_per_chunk + 255) / 256, 2048);
    hipLaunchKernelGGL(k_accumulate_list, dim3(grid), dim3(256), 0, st, P, d_partial, d_list, batch, samples, d_sum, d_moment, d_count);
}

void launch_accum_variance(const double* d_sum, const double* d_moment, const uint32_t* d_count, size_t npx, uint32_t batch,
                           float* d_var, hipStream_t st) {
    if (npx == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((npx + 255) / 256, 2048);
    hipLaunchKernelGGL(k_accum_variance, dim3(grid), dim3(256), 0, st, d_sum, d_moment, d_count, (uint32_t)npx, batch, d_var);
}

void launch_sample_lights(const DScene& S, const double* d_origins, size_t n, uint64_t seed, PrtLightSample* d_out,
                          hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_sample_lights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, d_origins, n, seed, d_out);
}

void launch_material_eval(const DScene& S, int material, const double* wi, const double* wo, const double* uv, size_t n,
                          uint64_t seed, double* out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_material_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, material, wi, wo, uv, n, seed, out);
}
void launch_material_scatter(const DScene& S, int material, const double* rd, const double* normal, const double* tangent,
                             const double* uv, size_t n, uint64_t seed, double* wi_out, double* att_out, int32_t* ok_out,
                             hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_material_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, material, rd,
                       d3{normal[0], normal[1], normal[2]}, d3{tangent[0], tangent[1], tangent[2]}, uv, n, seed, wi_out, att_out, ok_out);
}
void launch_texture_value(const DScene& S, int texture, const double* uv, size_t n, double* out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_texture_value, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, texture, uv, n, out);
}

void launch_features(const DScene& S, const DCamera& C, uint64_t seed_key, int jitter, int spp, float* albedo, float* normal,
                     float* depth, int32_t* prim, hipStream_t st) {
    const size_t npx = (size_t)C.width * C.height;
    if (npx == 0) return;
    const bool pad = S.tri_stride == PRT_TRI_PAD_STRIDE(real) && sizeof(DTri) != PRT_TRI_PAD_STRIDE(real);
    hipLaunchKernelGGL(pad ? k_features<true> : k_features<false>, dim3((unsigned)((npx + PRT_BLOCK - 1) / PRT_BLOCK)), dim3(PRT_BLOCK), 0,
                       st, S, C, seed_key, jitter, spp, albedo, normal, depth, prim);
}

void launch_add_f32(float* dst, const float* src, size_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_add_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n);
}

void launch_tonemap(const float* d_in, size_t n, uint8_t* d_out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_tonemap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_in, n, d_out);
}
#endif // !PRT_F32_TU

} // namespace PRT_NS
