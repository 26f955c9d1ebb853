// Test helper: Hittable::WindingNumber on a model's world, built as main.cpp builds it.
//   winding_check <resources_dir> <scene> <points.f64> <beta> <out.f64>
// points.f64: n x 3 doubles.  out.f64: one double per point.  Prints "points N inside I".
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
        const double beta = std::atof(argv[4]); // ("inf" parses as infinity)
        std::vector<point3> p;
        for (size_t i = 0; i + 2 < raw.size(); i += 3) p.emplace_back(raw[i], raw[i + 1], raw[i + 2]);
        const std::vector<double> w = world.WindingNumber(p, beta);
        if (w.size() != p.size()) return 4;
        int n_inside = 0;
        for (double x : w) n_inside += x > 0.5;
        std::FILE* f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(w.data(), sizeof(double), w.size(), f) != w.size()) return 2;
        std::fclose(f);
        std::printf("points %zu inside %d\n", p.size(), n_inside);
        return 0;
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 3;
    }
}
