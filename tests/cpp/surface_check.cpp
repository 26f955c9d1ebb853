// Test helper: the batch Hittable::Hit against the single-ray Hittable::Hit on main.cpp's world.
//   surface_check <resources_dir> <scene> <n_rays> <device_bvh: 0|1>
// With device_bvh = 1 a one-sample Camera::Render with bBuildBvhOnDevice comes first: the world's scene is created by its
// first use, so the queries that follow run on the GPU-built tree.
// Rays start inside the scene's box in pseudo-random directions; half of them get a finite interval.  For every ray the
// batch call must return the single-ray call's bool and, on a hit, its record: time, bFrontFace and the material pointer
// exactly, position / normal / tangent / uv to 1e-12.  Prints "rays N hits H mismatches M worst W"; exit status 0 only
// when M == 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pooraytracer/BVH.h"
#include "pooraytracer/Camera.h"
#include "pooraytracer/HittableList.h"
#include "pooraytracer/Model.h"
#include "pooraytracer/Ray.h"

int main(int argc, char** argv) {
    using namespace Pooraytracer;
    if (argc < 5) return 2;
    try {
        const std::string name = argv[2], path = std::string(argv[1]) + "/" + name;
        const int n = std::atoi(argv[3]);
        auto model = std::make_shared<Model>(path, name);
        HittableList world, lights;
        for (auto& mesh : model->meshes) {
            world.Add(make_shared<BVHNode>(mesh));
            if (mesh->material->HasEmission()) lights.Add(make_shared<BVHNode>(mesh));
        }
        world = HittableList(make_shared<BVHNode>(world));
        lights = HittableList(make_shared<BVHNode>(lights));
        if (std::atoi(argv[4]) != 0) {
            Camera camera;
            camera.samplesPerPixel = 1;
            camera.maxDepth = 1;
            camera.bBuildBvhOnDevice = true;
            camera.SetViewParametersByXmlFile(path + "/" + name + ".xml");
            camera.Render(world, lights);
        }
        const AABB box = world.BoundingBox();
        unsigned long long state = 0x9e3779b97f4a7c15ULL;
        auto next = [&]() { // splitmix64 -> [0, 1)
            unsigned long long z = (state += 0x9e3779b97f4a7c15ULL);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
            return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
        };
        const double diag = box.x.Length() + box.y.Length() + box.z.Length();
        const Interval domains[2] = {Interval(1e-3, std::numeric_limits<double>::infinity()), Interval(1e-3, 0.15 * diag)};
        int hits = 0, bad = 0, total = 0;
        double worst = 0.0;
        auto gap3 = [&](const vec3& a, const vec3& b) { worst = std::fmax(worst, std::fmax(std::fabs(a.x - b.x), std::fmax(std::fabs(a.y - b.y), std::fabs(a.z - b.z)))); };
        for (const Interval& dom : domains) {
            std::vector<Ray> rays;
            for (int i = 0; i < n / 2; ++i) {
                const vec3 o(box.x.min + next() * box.x.Length(), box.y.min + next() * box.y.Length(), box.z.min + next() * box.z.Length());
                const vec3 d(2 * next() - 1, 2 * next() - 1, 2 * next() - 1);
                rays.emplace_back(o, d);
            }
            std::vector<HitRecord> recs;
            const std::vector<bool> batch = world.Hit(rays, dom, recs);
            if (batch.size() != rays.size() || recs.size() != rays.size()) return 4;
            for (size_t i = 0; i < rays.size(); ++i) {
                HitRecord one;
                const bool hit = world.Hit(rays[i], dom, one);
                hits += hit;
                total++;
                if (hit != (bool)batch[i]) {
                    bad++;
                    continue;
                }
                if (!hit) {
                    bad += recs[i].material != nullptr;
                    continue;
                }
                const HitRecord& b = recs[i];
                const double before = worst;
                worst = 0.0;
                gap3(b.position, one.position);
                gap3(b.normal, one.normal);
                gap3(b.tangent, one.tangent);
                worst = std::fmax(worst, std::fmax(std::fabs(b.uv.x - one.uv.x), std::fabs(b.uv.y - one.uv.y)));
                const bool same = worst <= 1e-12 && b.time == one.time && b.bFrontFace == one.bFrontFace && b.material == one.material &&
                                  b.material != nullptr;
                bad += !same;
                worst = std::fmax(worst, before);
            }
        }
        std::printf("rays %d hits %d mismatches %d worst %.3g\n", total, hits, bad, worst);
        return bad == 0 ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 3;
    }
}
