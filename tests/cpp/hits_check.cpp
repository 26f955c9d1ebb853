// Test helper: Hittable::Hits on main.cpp's world.
//   hits_check <resources_dir> <scene> <n_rays> <max_hits>
// Rays start inside the scene's box in pseudo-random directions; half of them get a finite interval.  Prints one line per
// ray - origin, direction, the domain, the number of records of the batch Hits and their times (padded with -1) - for the
// caller to compare with the library's own lists, and "# single-ray mismatches M": rays on which the one-ray Hits differs
// from the batch form, or a record is not filled as Hit fills its one (position = ray(time), a material, the normal
// against the ray).  Exit status 0 only when M == 0.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pooraytracer/BVH.h"
#include "pooraytracer/HittableList.h"
#include "pooraytracer/Model.h"
#include "pooraytracer/Ray.h"

int main(int argc, char** argv) {
    using namespace Pooraytracer;
    if (argc < 5) return 2;
    try {
        const std::string name = argv[2], path = std::string(argv[1]) + "/" + name;
        const int n = std::atoi(argv[3]), k = std::atoi(argv[4]);
        auto model = std::make_shared<Model>(path, name);
        HittableList world;
        for (auto& mesh : model->meshes) world.Add(make_shared<BVHNode>(mesh));
        world = HittableList(make_shared<BVHNode>(world));
        const AABB box = world.BoundingBox();
        unsigned long long state = 0x9e3779b97f4a7c15ULL;
        auto next = [&]() { // splitmix64 -> [0, 1)
            unsigned long long z = (state += 0x9e3779b97f4a7c15ULL);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
            return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
        };
        const double diag = box.x.Length() + box.y.Length() + box.z.Length();
        const Interval domains[2] = {Interval(-std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()),
                                     Interval(1e-3, 0.3 * diag)};
        int bad = 0;
        for (const Interval& dom : domains) {
            std::vector<Ray> rays;
            for (int i = 0; i < n / 2; ++i) {
                const vec3 o(box.x.min + next() * box.x.Length(), box.y.min + next() * box.y.Length(), box.z.min + next() * box.z.Length());
                const vec3 d(2 * next() - 1, 2 * next() - 1, 2 * next() - 1);
                rays.emplace_back(o, d);
            }
            const std::vector<std::vector<HitRecord>> batch = world.Hits(rays, dom, k);
            for (size_t i = 0; i < rays.size(); ++i) {
                const std::vector<HitRecord> one = world.Hits(rays[i], dom, k);
                bool ok = one.size() == batch[i].size() && (int)one.size() <= k;
                for (size_t j = 0; ok && j < one.size(); ++j) {
                    const HitRecord& r = batch[i][j];
                    const vec3 p = rays[i](r.time);
                    ok = one[j].time == r.time && r.material && r.position.x == p.x && r.position.y == p.y && r.position.z == p.z &&
                         r.normal.x * rays[i].direction.x + r.normal.y * rays[i].direction.y + r.normal.z * rays[i].direction.z <= 0 &&
                         (j == 0 || batch[i][j - 1].time <= r.time);
                }
                bad += !ok;
                std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %zu", rays[i].origin.x, rays[i].origin.y, rays[i].origin.z,
                            rays[i].direction.x, rays[i].direction.y, rays[i].direction.z, dom.min, dom.max, batch[i].size());
                for (int j = 0; j < k; ++j) std::printf(" %.17g", j < (int)batch[i].size() ? batch[i][j].time : -1.0);
                std::printf("\n");
            }
        }
        std::printf("# single-ray mismatches %d\n", bad);
        return bad == 0 ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("# failed: %s\n", e.what());
        return 3;
    }
}
