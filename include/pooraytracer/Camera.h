// Camera.h — mirror of Source/Camera.h:11-53: same public fields, Render(world, lights) and
// colorAttachment.  Render flattens `world` (cached per object graph), uploads it once, and runs the
// HIP path tracer through the C ABI (prt_render); colorAttachment receives the fp64 framebuffer.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "HittableList.h"
#include "Math.h"
#include "Ray.h"

struct PrtCamera;
struct PrtRenderParams;
struct PrtDenoiseParams;

namespace Pooraytracer {
class Camera {
public:
    int imageWidth = 100;
    int imageHeight = 100;
    int samplesPerPixel = 1;
    int threadNums = 16; // kept for source compatibility; the device schedules its own wavefronts
    int maxDepth = 10;
    color background = color(0., 0., 0.);

    double fovy = 90.;
    vec3 eye = vec3(0., 0., 0.);
    vec3 lookAt = vec3(0., 0., -1.);
    vec3 up = vec3(0., 1., 0.);

    std::vector<color> colorAttachment;
    void Render(Hittable& world, Hittable& lights);
    // Addition (not in the reference): one progressive render for a whole spp ladder instead of one Render per rung.
    // sppLadder must be strictly increasing and >= 1.  The frame of rung k is the frame Render would make with
    // samplesPerPixel = sppLadder[k] (within ~1e-13: summation order, prt.h prt_accum_*), at the cost of the last rung
    // alone.  Before each onSnapshot call colorAttachment holds that frame and samplesPerPixel equals the rung, so
    // GetParametersStr() / WriteColorAttachment() name and write it as main.cpp:52 does; `seconds` is the wall clock
    // since the call began (the first call on a world includes its scene build and upload).  On return
    // samplesPerPixel is the last rung.  Single device only: a `devices` list of more than one throws
    // std::invalid_argument.
    void RenderProgressive(Hittable& world, Hittable& lights, const std::vector<int>& sppLadder,
                           const std::function<void(int spp, double seconds)>& onSnapshot);
    // Addition (not in the reference): adaptive sampling (prt.h prt_accum_*_adaptive).  Every pixel gets samples in rounds
    // until its noise estimate meets max(relTol * |mean|, absTol), never fewer than minSpp and never more than maxSpp;
    // a pixel that stopped after n samples holds the value Render gives it at samplesPerPixel = n (within ~1e-13).  The
    // first round renders minSpp samples, every later one roundSpp (0: minSpp).  minSpp, maxSpp and roundSpp are multiples
    // of batch (0: the library's default, PRT_ADAPTIVE_DEFAULT_BATCH).  On return colorAttachment holds the frame,
    // samplesPerPixel the largest per-pixel count, and `counts` (when given) the W*H counts, row by row.  Returns the number
    // of rounds that rendered.  Single device only, like RenderProgressive.  It also fills varianceAttachment (below).
    int RenderAdaptive(Hittable& world, Hittable& lights, double relTol, int minSpp, int maxSpp,
                       std::vector<uint32_t>* counts = nullptr, double absTol = 0.0, int batch = 0, int roundSpp = 0);
    // Addition (not in the reference): RayColor for rays of the caller's own (prt.h prt_ray_color) — probes, lightmap texels,
    // camera models this class lacks.  out[i] = the mean over `samples` samples of RayColor(rays[i], maxDepth, world, lights)
    // (Camera.cpp:119-204) with this camera's maxDepth, russianRoulette, bSampleLights, background, seed and precision; ray
    // i draws from the streams keyed (seed, i, s).  Directions are not normalised.  The image fields, samplesPerPixel and
    // bPixelJitter are not used.  Throws std::invalid_argument for a non-finite ray or a zero direction.  Single device
    // only, like RenderProgressive.
    void RayColor(const std::vector<Ray>& rays, Hittable& world, Hittable& lights, int samples, std::vector<color>& out);
    // Addition (not in the reference): the edge-aware a-trous denoiser (prt.h prt_denoise) on colorAttachment, guided by the
    // first-hit features of this camera (prt_render_features: albedo, normal, depth).  Runs after Render, RenderProgressive
    // or RenderAdaptive on the same world; params NULL = prt_denoise_defaults.  The result goes to denoisedAttachment;
    // colorAttachment is left as it is.  Single device only, like RenderProgressive.
    std::vector<color> denoisedAttachment;
    void Denoise(Hittable& world, const PrtDenoiseParams* params = nullptr);
    // Addition: the variance-guided form of the filter (prt.h prt_denoise_guided), whose colour tolerance is each pixel's
    // own estimated standard deviation.  Valid after RenderAdaptive on the same world, which leaves the variance of every
    // pixel's mean luminance in varianceAttachment (W*H, row by row); params NULL = prt_denoise_guided_defaults.  It fills
    // denoisedAttachment.  RenderAdaptive's accumulator, which holds the moments, does not outlive the call, so the variance
    // cannot be computed on demand here: every RenderAdaptive reads it back (one small kernel and a W*H float copy), whether
    // DenoiseGuided follows or not.
    std::vector<float> varianceAttachment;
    void DenoiseGuided(Hittable& world, const PrtDenoiseParams* params = nullptr);
    // 8-bit sRGB PNG (+ Radiance .hdr), Camera.cpp:279-331
    void WriteColorAttachment(const std::string& outputPath, bool bWriteHDR = true) const;
    // The same for denoisedAttachment.
    void WriteDenoisedAttachment(const std::string& outputPath, bool bWriteHDR = true) const;
    std::string GetParametersStr() const;
    // <camera width height fovy><eye/><lookat/><up/></camera>, Camera.cpp:339-389
    void SetViewParametersByXmlFile(const std::string& xmlFilePath);

    bool bSampleLights = true;
    double russianRoulette = 0.8;

    // additions (not in the reference): RNG key, device index, counters of the last Render
    unsigned long long seed = 1;
    bool bBuildBvhOnDevice = false; // PRT_SCENE_DEVICE_BVH: build the traversal BVH on the GPU (first Render of a world)
    bool bFloatPrecision = false; // PRT_PRECISION_F32: the fp32 fast mode (tolerance tier 2; the reference computes in double)
    bool bPixelJitter = false; // per-sample SampleSquare() pixel offset: the AA the reference has commented out (Camera.cpp:110-111)
    int device = 0;
    std::vector<int> devices; // non-empty: cut the frame into tiles over these GPUs (one host thread each); overrides `device`
    unsigned long long lastRays = 0;
    double lastKernelMs = 0.0;

private:
    // Render / RenderProgressive: world's scene with the `lights` list, uploaded to devs (cached on world), and this
    // camera's fields as the C ABI takes them
    Hittable::DeviceCache& PrepareScene(Hittable& world, Hittable& lights, const std::vector<int>& devs, PrtCamera& c,
                                        PrtRenderParams& p);
    void FillParams(PrtCamera& c, PrtRenderParams& p) const;
    // Denoise / DenoiseGuided: the features of this camera and the filter on colorAttachment, into denoisedAttachment
    void DenoiseInto(Hittable& world, const PrtDenoiseParams* params, bool guided);
};
} // namespace Pooraytracer
