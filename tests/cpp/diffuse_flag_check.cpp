// Stand-alone check (CPU only) of the material-table flag behind the DIFFUSE form of the render kernel: materials_all_diffuse
// (scene_setup.cpp) on the tables setup_materials makes of hand-built PrtMaterial lists.  One line per table:
//   <name> <flag>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prt_host.h"

using namespace prt;

static PrtMaterial mat(int type, int texture = -1, double ns = 0.0) {
    PrtMaterial m;
    std::memset(&m, 0, sizeof(m));
    m.type = type;
    m.texture = texture;
    m.ns = ns;
    m.kd[0] = m.kd[1] = m.kd[2] = 0.5;
    m.emission[0] = m.emission[1] = m.emission[2] = type == PRT_MAT_DIFFUSE_LIGHT ? 5.0 : 0.0;
    m.alpha_x = m.alpha_y = 0.3;
    return m;
}

static void say(const char* name, const std::vector<PrtMaterial>& pm) {
    PrtSceneDesc d;
    std::memset(&d, 0, sizeof(d));
    d.materials = pm.data();
    d.n_materials = (uint32_t)pm.size();
    std::vector<DMaterial> mats;
    setup_materials(d, mats);
    std::printf("%s %d\n", name, materials_all_diffuse(mats) ? 1 : 0);
}

int main() {
    const PrtMaterial lam = mat(PRT_MAT_LAMBERTIAN), light = mat(PRT_MAT_DIFFUSE_LIGHT);
    say("empty", {});
    say("emitters_only", {light, light});
    say("lambertians_only", {lam, lam, lam});
    say("cornell", {lam, lam, lam, light, lam});
    say("textured_lambertian", {lam, mat(PRT_MAT_LAMBERTIAN, 0), light});
    say("textured_emitter", {lam, mat(PRT_MAT_DIFFUSE_LIGHT, 0)});
    say("mirror", {lam, light, mat(PRT_MAT_MIRROR)});
    say("phong_ns0", {lam, light, mat(PRT_MAT_PHONG, -1, 0.0)});   // (no SkipLightSampling at Ns <= 1: still not a Lambertian)
    say("phong_ns20", {lam, light, mat(PRT_MAT_PHONG, -1, 20.0)});
    say("cooktorrance", {lam, light, mat(PRT_MAT_COOKTORRANCE)});
    say("debug", {lam, light, mat(PRT_MAT_DEBUG)});
    say("empty_material", {lam, light, mat(PRT_MAT_EMPTY)});
    say("mirror_first", {mat(PRT_MAT_MIRROR), lam, light});
    // the flag reads the table, not the description: a Lambertian whose table entry is marked as skipping light sampling
    {
        PrtSceneDesc d;
        std::memset(&d, 0, sizeof(d));
        const std::vector<PrtMaterial> pm = {lam, light};
        d.materials = pm.data();
        d.n_materials = 2;
        std::vector<DMaterial> mats;
        setup_materials(d, mats);
        mats[0].skip_light_sampling = 1;
        std::printf("marked_skip %d\n", materials_all_diffuse(mats) ? 1 : 0);
    }
    return 0;
}
