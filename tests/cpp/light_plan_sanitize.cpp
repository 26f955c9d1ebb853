// Stand-alone check (ASan + UBSan, CPU only) of the host half of a light update: the plan of the O(1) tables
// (scene_setup.cpp, plan_light_tables) of a tree built WITHOUT tables must be the layout the full host build gives the
// same geometry — same top nodes, same root, same header words, same word count — for lights lists of one to five meshes
// with odd triangle counts, a mesh collapsed onto a point, and lists whose every mesh is degenerate; and the listed
// Triangle precompute (update_triangles_listed) must equal the full one on the listed triangles.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "prt_host.h"

using namespace prt;

static int check(unsigned mask, const std::vector<double>& v, const std::vector<uint64_t>& first, const std::vector<int32_t>& mat,
                 const PrtMaterial* pm) {
    std::vector<int32_t> lm;
    for (int m = 0; m + 1 < (int)first.size(); ++m)
        if (mask >> m & 1) lm.push_back(m);
    PrtSceneDesc d;
    std::memset(&d, 0, sizeof(d));
    d.vertices = v.data();
    d.n_tris = v.size() / 9;
    d.n_meshes = (uint32_t)mat.size();
    d.mesh_first_tri = first.data();
    d.mesh_material = mat.data();
    d.materials = pm;
    d.n_materials = 1;
    d.light_meshes = lm.data();
    d.n_light_meshes = (uint32_t)lm.size();
    std::vector<HostTri> tris;
    std::vector<DMaterial> mats;
    setup_triangles(d, tris);
    setup_materials(d, mats);
    LightTree full, bare;
    build_light_tree(d, tris, mats, full);
    build_light_tree(d, tris, mats, bare, false);
    if (bare.n_tables || !bare.tab.empty() || bare.nodes.size() != bare.full_nodes.size() || bare.root != bare.full_root) return 1;
    if (std::memcmp(bare.full_nodes.data(), full.full_nodes.data(), full.full_nodes.size() * sizeof(DLightNode))) return 2;
    if (bare.tris.size() != full.tris.size() || std::memcmp(bare.tris.data(), full.tris.data(), full.tris.size() * sizeof(DLightTri))) return 3;
    LightTablePlan plan;
    const bool tables = plan_light_tables(bare, plan);
    if (tables != (full.n_tables != 0)) return 4;
    if (tables) {
        if (plan.node.size() != full.n_tables || plan.area.size() != full.n_tables || plan.tab.size() != full.tab.size()) return 5;
        if (std::memcmp(plan.tab.data(), full.tab.data(), 8 * sizeof(uint32_t) * full.n_tables)) return 6; // the headers
        for (size_t w = 8 * full.n_tables; w < plan.tab.size(); ++w)
            if (plan.tab[w]) return 7; // the fill's words are zero in a plan
        if (plan.root != full.root || plan.top.size() != full.nodes.size() ||
            (!full.nodes.empty() && std::memcmp(plan.top.data(), full.nodes.data(), full.nodes.size() * sizeof(DLightNode))))
            return 8;
        apply_light_tables(bare, plan, full.tab);
        if (bare.root != full.root || bare.n_tables != full.n_tables || bare.tab != full.tab) return 9;
        const float total = (float)full.area;
        for (int k = 0; k <= 4096; ++k) { // the planned top part + the host's words pick what the full tree picks
            const float p = total * (float)k / 4096.f;
            if (light_pick(bare, p) != light_pick_full_tree(full, p)) return 10;
        }
    }
    // the listed precompute on the light triangles, from moved vertices
    std::vector<double> moved(v);
    for (size_t i = 0; i < moved.size(); ++i) moved[i] = moved[i] * 1.25 + 0.5;
    std::vector<HostTri> all(tris), some(tris);
    update_triangles(moved.data(), nullptr, all);
    std::vector<int32_t> prims;
    std::vector<double> gathered;
    for (const DLightTri& lt : full.tris) {
        prims.push_back(lt.prim);
        gathered.insert(gathered.end(), moved.begin() + (size_t)lt.prim * 9, moved.begin() + (size_t)lt.prim * 9 + 9);
    }
    update_triangles_listed(prims.data(), prims.size(), gathered.data(), nullptr, some);
    for (int32_t p : prims)
        if (std::memcmp(&some[(size_t)p], &all[(size_t)p], sizeof(HostTri))) return 11;
    std::printf("mask %u: %zu light triangles, %u tables, %zu words ok\n", mask, full.tris.size(), full.n_tables, full.tab.size());
    return 0;
}

int main() {
    const int counts[] = {17, 33, 300, 16, 40, 15, 2, 1280};
    const int nm = 8;
    std::vector<double> v;
    std::vector<uint64_t> first{0};
    std::vector<int32_t> mat;
    std::mt19937_64 g(5);
    std::uniform_real_distribution<double> U(-1, 1);
    for (int m = 0; m < nm; ++m) {
        for (int t = 0; t < counts[m]; ++t) {
            const double c[3] = {U(g) * 3 + m, U(g) * 3, U(g) * 3};
            for (int k = 0; k < 9; ++k) v.push_back(m == 4 ? 0.5 : c[k % 3] + 0.2 * U(g)); // mesh 4: collapsed onto a point
        }
        first.push_back(v.size() / 9);
        mat.push_back(0);
    }
    PrtMaterial pm;
    std::memset(&pm, 0, sizeof(pm));
    pm.type = PRT_MAT_DIFFUSE_LIGHT;
    pm.emission[0] = 1;
    pm.texture = -1;
    const unsigned masks[] = {255u, 4u, 8u, 16u, 32u, 80u, 17u, 132u, 7u, 13u, 28u, 143u};
    for (unsigned mask : masks)
        if (const int rc = check(mask, v, first, mat, &pm)) {
            std::printf("mask %u: check %d failed\n", mask, rc);
            return 2;
        }
    return 0;
}
