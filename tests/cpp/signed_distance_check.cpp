// Test helper: Hittable::SignedDistance on a model's world, built as main.cpp builds it.
//   signed_distance_check <resources_dir> <scene> <points.f64> <max_dist> <out.f64>
// points.f64: n x 3 doubles.  out.f64: per point 5 doubles - found, signed distance, closest[3] (zeros where nothing was
// found).  Prints "points N found F inside I".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pooraytracer/BVH.h"
#include "pooraytracer/HittableList.h"
#include "pooraytracer/Model.h"

int main(int argc, char** argv) {
    using namespace Pooraytracer;
    if (argc < 6) return 2;
    try {
        const std::string name = argv[2], path = std::string(argv[1]) + "/" + name;
        auto model = std::make_shared<Model>(path, name);
        HittableList world;
        for (auto& mesh : model->meshes) world.Add(make_shared<BVHNode>(mesh));
        world = HittableList(make_shared<BVHNode>(world));
        std::vector<double> raw;
        {
            std::FILE* f = std::fopen(argv[3], "rb");
            if (!f) return 2;
            double buf[3];
            while (std::fread(buf, sizeof(double), 3, f) == 3) raw.insert(raw.end(), buf, buf + 3);
            std::fclose(f);
        }
        const double maxDist = std::atof(argv[4]);
        std::vector<point3> p;
        for (size_t i = 0; i + 2 < raw.size(); i += 3) p.emplace_back(raw[i], raw[i + 1], raw[i + 2]);
        std::vector<point3> closest;
        std::vector<double> sdist;
        const std::vector<bool> found = world.SignedDistance(p, maxDist, closest, sdist);
        std::vector<double> out(p.size() * 5, 0.0);
        int n_found = 0, n_inside = 0;
        for (size_t i = 0; i < p.size(); ++i) {
            if (!found[i]) continue;
            double* o = out.data() + i * 5;
            o[0] = 1.0, o[1] = sdist[i], o[2] = closest[i].x, o[3] = closest[i].y, o[4] = closest[i].z;
            n_found++;
            n_inside += sdist[i] < 0.0;
        }
        std::FILE* f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
        std::fclose(f);
        std::printf("points %zu found %d inside %d\n", p.size(), n_found, n_inside);
        return 0;
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 3;
    }
}
