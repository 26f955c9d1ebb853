// pooraytracer_main.cpp — the reference's main.cpp (main.cpp:6-55) against the drop-in host API, with
// the hard-coded scene name / spp / depth turned into arguments:
//   pooraytracer_main <resources_dir> <scene_name> [spp=100] [depth=100] [out_dir=.] [out.f64] [--ladder=S1,S2,...]
//                     [--adaptive=REL_TOL [--min-spp=M] [--counts=counts.u32] [--denoise-guided[=ITER]]] [--denoise[=ITER]]
// Reads <resources_dir>/<scene>/<scene>.obj|.mtl|.xml like the reference, renders on the GPU, writes
// <scene>_spp<S>-depth<D>_<seconds>s.png + .hdr (main.cpp:52 naming, timestamp omitted).
// --ladder (anywhere on the line): one progressive render (Camera::RenderProgressive) that writes a .png + .hdr per rung
// of the strictly increasing spp list, for the cost of the last rung; spp is then ignored, <seconds> is the time since the
// render began, and out.f64 receives the last rung's frame.
// --adaptive=REL_TOL (anywhere on the line): adaptive sampling (Camera::RenderAdaptive, abs_tol 0, the library's default
// batch): spp is then the largest number of samples a pixel may get (max_spp, rounded down to a multiple of the batch),
// no pixel gets fewer than --min-spp (default 64, capped at max_spp), and every round after the first adds min_spp
// samples.  The frame is written as <scene>_adaptive<REL_TOL>_spp<S>-depth<D>_<seconds>s.png + .hdr, S = the largest
// per-pixel count; --counts=FILE receives the W*H per-pixel counts (uint32, row by row) and out.f64 the frame.
// --denoise[=ITER] (anywhere on the line): every frame written (plain, each --ladder rung, --adaptive) is also denoised
// (Camera::Denoise: the library's default parameters, ITER a-trous levels in 1..10 when given) and written next to it as
// <name>_denoised.png + .hdr.
// --denoise-guided[=ITER] (anywhere on the line, with --adaptive= only): the adaptive frame is also put through the
// variance-guided filter (Camera::DenoiseGuided: prt_denoise_guided_defaults, ITER levels in 1..10 when given), driven by the
// per-pixel variance the adaptive render estimated, and written next to it as <name>_guided.png + .hdr.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "pooraytracer/BVH.h"
#include "pooraytracer/Camera.h"
#include "prt.h"
#include "pooraytracer/Model.h"

int main(int argc_all, char** argv_all) {
    using namespace Pooraytracer;
    // --ladder=... may stand anywhere: the positional arguments are the others, in order
    std::vector<int> ladder;
    std::vector<char*> args;
    std::string adaptive, minSppArg, countsPath;
    bool denoise = false, denoiseGuided = false;
    int denoiseIter = 0, guidedIter = 0; // 0: the library's default
    // --NAME or --NAME=ITER, ITER in 1..10
    auto levelsArg = [](const std::string& a, const std::string& name, int& iter) {
        if (a == name) return true;
        const std::string v = a.substr(name.size() + 1);
        char* end = nullptr;
        const long n = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end != '\0' || n < 1 || n > 10) {
            std::fprintf(stderr, "error: %s wants a number of a-trous levels in 1..10, got '%s'\n", name.c_str(), v.c_str());
            return false;
        }
        iter = (int)n;
        return true;
    };
    for (int i = 0; i < argc_all; ++i) {
        const std::string a = argv_all[i];
        if (i > 0 && (a == "--denoise" || a.rfind("--denoise=", 0) == 0)) {
            denoise = true;
            if (!levelsArg(a, "--denoise", denoiseIter)) return 2;
        } else if (i > 0 && (a == "--denoise-guided" || a.rfind("--denoise-guided=", 0) == 0)) {
            denoiseGuided = true;
            if (!levelsArg(a, "--denoise-guided", guidedIter)) return 2;
        } else if (i > 0 && a.rfind("--adaptive=", 0) == 0) {
            adaptive = a.substr(11);
        } else if (i > 0 && a.rfind("--min-spp=", 0) == 0) {
            minSppArg = a.substr(10);
        } else if (i > 0 && a.rfind("--counts=", 0) == 0) {
            countsPath = a.substr(9);
        } else if (i > 0 && a.rfind("--ladder=", 0) == 0) {
            std::string list = a.substr(9);
            for (size_t at = 0; at <= list.size();) {
                const size_t comma = std::min(list.find(',', at), list.size());
                const std::string item = list.substr(at, comma - at);
                char* end = nullptr;
                const long v = std::strtol(item.c_str(), &end, 10);
                if (item.empty() || *end != '\0' || v < 1 || v > 0x7fffffffL || (!ladder.empty() && v <= ladder.back())) {
                    std::fprintf(stderr, "error: --ladder wants a strictly increasing list of spp >= 1, got '%s'\n", list.c_str());
                    return 2;
                }
                ladder.push_back((int)v);
                at = comma + 1;
            }
        } else {
            args.push_back(argv_all[i]);
        }
    }
    const int argc = (int)args.size();
    char** argv = args.data();
    double relTol = 0.0;
    if (!adaptive.empty()) {
        char* end = nullptr;
        relTol = std::strtod(adaptive.c_str(), &end);
        if (*end != '\0' || !(relTol >= 0.0) || relTol > 1e300) {
            std::fprintf(stderr, "error: --adaptive wants a relative tolerance >= 0, got '%s'\n", adaptive.c_str());
            return 2;
        }
        if (!ladder.empty()) {
            std::fprintf(stderr, "error: --adaptive and --ladder exclude each other\n");
            return 2;
        }
    }
    if (denoiseGuided && adaptive.empty()) {
        std::fprintf(stderr, "error: --denoise-guided needs --adaptive=REL_TOL (the variance comes from the adaptive accumulator's moments)\n");
        return 2;
    }
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s resources_dir scene_name [spp] [depth] [out_dir] [out.f64] [--ladder=S1,S2,...] [--adaptive=REL_TOL [--min-spp=M] [--counts=FILE] [--denoise-guided[=ITER]]] [--denoise[=ITER]]\n", argv_all[0]);
        return 2;
    }
    try {
        const std::string fileName = argv[2];
        const std::string filePath = std::string(argv[1]) + "/" + fileName;
        Camera camera;
        camera.bSampleLights = true;
        camera.russianRoulette = 0.8;
        camera.samplesPerPixel = argc > 3 ? std::atoi(argv[3]) : 100;
        camera.maxDepth = argc > 4 ? std::atoi(argv[4]) : 100;
        camera.threadNums = 16;
        camera.background = color(0.0, 0.0, 0.0);
        camera.SetViewParametersByXmlFile(filePath + "/" + fileName + ".xml");

        std::shared_ptr<Model> model = std::make_shared<Model>(filePath, fileName);
        HittableList world;
        HittableList lights;
        for (auto& mesh : model->meshes) {
            world.Add(make_shared<BVHNode>(mesh));
            if (mesh->material->HasEmission()) lights.Add(make_shared<BVHNode>(mesh));
        }
        world = HittableList(make_shared<BVHNode>(world));
        lights = HittableList(make_shared<BVHNode>(lights));

        const std::string outDir = argc > 5 ? argv[5] : ".";
        // --denoise: the frame in colorAttachment, denoised, next to `png`
        auto writeDenoised = [&](const std::string& png) {
            if (!denoise) return;
            PrtDenoiseParams dp;
            prt_denoise_defaults(&dp);
            if (denoiseIter > 0) dp.iterations = denoiseIter;
            camera.Denoise(world, &dp);
            const std::string out = png.substr(0, png.size() - 4) + "_denoised.png";
            camera.WriteDenoisedAttachment(out);
            std::printf("  denoised (%d levels) -> %s\n", dp.iterations, out.c_str());
        };
        if (!adaptive.empty()) {
            const int batch = PRT_ADAPTIVE_DEFAULT_BATCH;
            const int maxSpp = camera.samplesPerPixel / batch * batch;
            int minSpp = minSppArg.empty() ? 64 : std::atoi(minSppArg.c_str());
            minSpp = std::min(minSpp, maxSpp) / batch * batch;
            if (maxSpp < 2 * batch || minSpp < 2 * batch) {
                std::fprintf(stderr, "error: --adaptive needs spp and --min-spp of at least %d (two batches of %d)\n", 2 * batch, batch);
                return 2;
            }
            std::vector<uint32_t> counts;
            const auto start = std::chrono::steady_clock::now();
            const int rounds = camera.RenderAdaptive(world, lights, relTol, minSpp, maxSpp, &counts);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
            char t[64];
            std::snprintf(t, sizeof(t), "%.2fs", sec);
            const std::string png = outDir + "/" + fileName + "_adaptive" + adaptive + "_" + camera.GetParametersStr() + "_" + t + ".png";
            camera.WriteColorAttachment(png);
            writeDenoised(png);
            if (denoiseGuided) {
                PrtDenoiseParams dp;
                prt_denoise_guided_defaults(&dp);
                if (guidedIter > 0) dp.iterations = guidedIter;
                camera.DenoiseGuided(world, &dp);
                const std::string out = png.substr(0, png.size() - 4) + "_guided.png";
                camera.WriteDenoisedAttachment(out);
                std::printf("  variance-guided denoise (%d levels) -> %s\n", dp.iterations, out.c_str());
            }
            double total = 0;
            for (const uint32_t n : counts) total += n;
            std::printf("%s: %dx%d adaptive rel_tol %s, spp %d..%d, %d rounds, mean %.1f samples per pixel, %.3f s (includes BVH build + upload) -> %s\n",
                        fileName.c_str(), camera.imageWidth, camera.imageHeight, adaptive.c_str(), minSpp, maxSpp, rounds,
                        total / std::max<size_t>(1, counts.size()), sec, png.c_str());
            if (!countsPath.empty()) {
                std::ofstream o(countsPath, std::ios::binary);
                o.write(reinterpret_cast<const char*>(counts.data()), (std::streamsize)(counts.size() * sizeof(uint32_t)));
            }
            if (argc > 6) {
                std::ofstream o(argv[6], std::ios::binary);
                o.write(reinterpret_cast<const char*>(camera.colorAttachment.data()),
                        (std::streamsize)(camera.colorAttachment.size() * sizeof(color)));
            }
            prt_shutdown();
            return 0;
        }
        if (!ladder.empty()) {
            camera.RenderProgressive(world, lights, ladder, [&](int, double sec) {
                char t[64];
                std::snprintf(t, sizeof(t), "%.2fs", sec);
                const std::string png = outDir + "/" + fileName + "_" + camera.GetParametersStr() + "_" + t + ".png";
                camera.WriteColorAttachment(png);
                std::printf("%s: %dx%d %s, %.3f s since the start (the first rung includes BVH build + upload), %llu rays, kernel %.2f ms -> %s\n",
                            fileName.c_str(), camera.imageWidth, camera.imageHeight, camera.GetParametersStr().c_str(), sec,
                            camera.lastRays, camera.lastKernelMs, png.c_str());
                writeDenoised(png);
            });
            if (argc > 6) {
                std::ofstream o(argv[6], std::ios::binary);
                o.write(reinterpret_cast<const char*>(camera.colorAttachment.data()),
                        (std::streamsize)(camera.colorAttachment.size() * sizeof(color)));
            }
            prt_shutdown();
            return 0;
        }
        auto start = std::chrono::steady_clock::now();
        camera.Render(world, lights);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        char t[64];
        std::snprintf(t, sizeof(t), "%.2fs", sec);
        const std::string png = outDir + "/" + fileName + "_" + camera.GetParametersStr() + "_" + t + ".png";
        camera.WriteColorAttachment(png);
        writeDenoised(png);
        if (argc > 6) {
            std::ofstream o(argv[6], std::ios::binary);
            o.write(reinterpret_cast<const char*>(camera.colorAttachment.data()),
                    (std::streamsize)(camera.colorAttachment.size() * sizeof(color)));
        }
        std::printf("%s: %zu meshes, %dx%d %s, %.3f s (first Render includes BVH build + upload), %llu rays, kernel %.2f ms -> %s\n",
                    fileName.c_str(), model->meshes.size(), camera.imageWidth, camera.imageHeight,
                    camera.GetParametersStr().c_str(), sec, camera.lastRays, camera.lastKernelMs, png.c_str());
        prt_shutdown(); // releases the RCCL communicators a multi-device Camera::devices render cached (no-op otherwise)
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
