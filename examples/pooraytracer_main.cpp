// pooraytracer_main.cpp — the reference's main.cpp (main.cpp:6-55) against the drop-in host API, with
// the hard-coded scene name / spp / depth turned into arguments:
//   pooraytracer_main <resources_dir> <scene_name> [spp=100] [depth=100] [out_dir=.] [out.f64] [--ladder=S1,S2,...]
// Reads <resources_dir>/<scene>/<scene>.obj|.mtl|.xml like the reference, renders on the GPU, writes
// <scene>_spp<S>-depth<D>_<seconds>s.png + .hdr (main.cpp:52 naming, timestamp omitted).
// --ladder (anywhere on the line): one progressive render (Camera::RenderProgressive) that writes a .png + .hdr per rung
// of the strictly increasing spp list, for the cost of the last rung; spp is then ignored, <seconds> is the time since the
// render began, and out.f64 receives the last rung's frame.
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
    for (int i = 0; i < argc_all; ++i) {
        const std::string a = argv_all[i];
        if (i > 0 && a.rfind("--ladder=", 0) == 0) {
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
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s resources_dir scene_name [spp] [depth] [out_dir] [out.f64] [--ladder=S1,S2,...]\n", argv_all[0]);
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
        if (!ladder.empty()) {
            camera.RenderProgressive(world, lights, ladder, [&](int, double sec) {
                char t[64];
                std::snprintf(t, sizeof(t), "%.2fs", sec);
                const std::string png = outDir + "/" + fileName + "_" + camera.GetParametersStr() + "_" + t + ".png";
                camera.WriteColorAttachment(png);
                std::printf("%s: %dx%d %s, %.3f s since the start (the first rung includes BVH build + upload), %llu rays, kernel %.2f ms -> %s\n",
                            fileName.c_str(), camera.imageWidth, camera.imageHeight, camera.GetParametersStr().c_str(), sec,
                            camera.lastRays, camera.lastKernelMs, png.c_str());
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
