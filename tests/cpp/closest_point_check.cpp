// Test helper: Hittable::ClosestPoint, single and batch, on main.cpp's world.
//   closest_point_check <resources_dir> <scene> <points.f64> <max_dist> <out.f64>
// points.f64: n x 3 doubles.  out.f64: per point 10 doubles - the batch call's found, distance, closest[3], then the
// single call's found, distance, closest[3] (zeros where nothing was found).  Prints "points N found F".
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
        std::vector<double> distance;
        const std::vector<bool> found = world.ClosestPoint(p, maxDist, closest, distance);
        std::vector<double> out(p.size() * 10, 0.0);
        int n_found = 0;
        for (size_t i = 0; i < p.size(); ++i) {
            double* o = out.data() + i * 10;
            if (found[i]) {
                o[0] = 1.0, o[1] = distance[i], o[2] = closest[i].x, o[3] = closest[i].y, o[4] = closest[i].z;
                n_found++;
            }
            point3 c(0, 0, 0);
            double d = 0.0;
            if (world.ClosestPoint(p[i], maxDist, c, d)) o[5] = 1.0, o[6] = d, o[7] = c.x, o[8] = c.y, o[9] = c.z;
        }
        std::FILE* f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
        std::fclose(f);
        std::printf("points %zu found %d\n", p.size(), n_found);
        return 0;
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 3;
    }
}
