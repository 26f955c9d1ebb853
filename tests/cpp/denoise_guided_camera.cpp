// Test helper: pooraytracer_main's --adaptive flow followed by Camera::DenoiseGuided with the library's defaults:
//   denoise_guided_camera <resources_dir> <scene> <spp> <depth> <rel_tol> <min_spp> <out.f64> <out.png>
// out.f64 receives denoisedAttachment (W*H*3 doubles), out.png (+ .hdr) what WriteDenoisedAttachment makes of it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>

#include "pooraytracer/BVH.h"
#include "pooraytracer/Camera.h"
#include "pooraytracer/Model.h"
#include "prt.h"

int main(int argc, char** argv) {
    using namespace Pooraytracer;
    if (argc < 9) return 2;
    try {
        const std::string name = argv[2], path = std::string(argv[1]) + "/" + name;
        Camera camera;
        camera.bSampleLights = true;
        camera.russianRoulette = 0.8;
        camera.samplesPerPixel = std::atoi(argv[3]);
        camera.maxDepth = std::atoi(argv[4]);
        camera.background = color(0.0, 0.0, 0.0);
        camera.SetViewParametersByXmlFile(path + "/" + name + ".xml");
        auto model = std::make_shared<Model>(path, name);
        HittableList world, lights;
        for (auto& mesh : model->meshes) {
            world.Add(make_shared<BVHNode>(mesh));
            if (mesh->material->HasEmission()) lights.Add(make_shared<BVHNode>(mesh));
        }
        world = HittableList(make_shared<BVHNode>(world));
        lights = HittableList(make_shared<BVHNode>(lights));
        try {
            camera.DenoiseGuided(world); // nothing rendered yet
            std::printf("DenoiseGuided before RenderAdaptive was not refused\n");
            return 3;
        } catch (const std::logic_error&) {
        }
        const int batch = PRT_ADAPTIVE_DEFAULT_BATCH;
        const int maxSpp = camera.samplesPerPixel / batch * batch;
        const int minSpp = std::min(std::atoi(argv[6]), maxSpp) / batch * batch;
        camera.RenderAdaptive(world, lights, std::atof(argv[5]), minSpp, maxSpp);
        camera.DenoiseGuided(world);
        std::ofstream o(argv[7], std::ios::binary);
        o.write(reinterpret_cast<const char*>(camera.denoisedAttachment.data()),
                (std::streamsize)(camera.denoisedAttachment.size() * sizeof(color)));
        camera.WriteDenoisedAttachment(argv[8]);
        std::printf("ok %zu pixels\n", camera.denoisedAttachment.size());
        prt_shutdown();
        return 0;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
}
