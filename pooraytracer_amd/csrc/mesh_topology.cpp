// mesh_topology.cpp — weld, ids, adjacency and the PrtTopologyInfo counts of a triangle list (mesh_topology.h; the rules
// are stated in include/prt.h at prt_scene_topology_info).  No HIP: this file compiles on its own.
//
// Two open-addressing tables (vertices keyed by the three coordinate words, edges by the ordered id pair), sized for at
// most half full; ids are handed out in the order of first appearance, so the result is a pure function of the input.
#include "mesh_topology.h"

#include <algorithm>
#include <cstring>

#if defined(__clang__)
#pragma clang fp contract(off) // "cross(v1-v0, v2-v0) is exactly zero" is a statement about individually rounded operations
#endif

namespace prt {
namespace {

inline uint64_t mix(uint64_t x) { // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

size_t table_size(size_t items) {
    size_t c = 16;
    while (c < items * 2) c <<= 1;
    return c;
}

// start[i] = number of entries before list i, from per-list counts in start[i + 1]
void prefix(std::vector<uint32_t>& start) {
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
}

} // namespace

void build_topology(const double* corners, size_t stride, size_t n_tris, MeshTopology& out, bool lists) {
    out = MeshTopology();
    std::memset(&out.info, 0, sizeof(out.info));
    const size_t nc = n_tris * 3;
    out.vid.assign(nc, 0);
    out.eid.assign(nc, kNoTopoId);

    // ---- weld: bitwise equal coordinates after -0.0 -> +0.0
    std::vector<uint64_t> vkey; // three words per vertex
    uint32_t nv = 0;
    {
        const size_t mask = table_size(nc) - 1;
        std::vector<uint32_t> slot(mask + 1, kNoTopoId);
        for (size_t c = 0; c < nc; ++c) {
            const double* x = corners + (c / 3) * stride + (c % 3) * 3;
            uint64_t b[3];
            for (int a = 0; a < 3; ++a) {
                double d = x[a];
                if (d == 0.0) d = 0.0; // -0.0 is +0.0
                std::memcpy(&b[a], &d, 8);
            }
            size_t i = (size_t)mix(b[0] ^ mix(b[1] ^ mix(b[2]))) & mask;
            while (slot[i] != kNoTopoId) {
                const uint64_t* k = vkey.data() + (size_t)slot[i] * 3;
                if (k[0] == b[0] && k[1] == b[1] && k[2] == b[2]) break;
                i = (i + 1) & mask;
            }
            if (slot[i] == kNoTopoId) {
                slot[i] = nv++;
                vkey.insert(vkey.end(), b, b + 3);
            }
            out.vid[c] = slot[i];
        }
    }
    vkey = std::vector<uint64_t>();

    // ---- edges: unordered pairs of distinct vertex ids; faces and forward traversals (low id -> high id) of each
    std::vector<uint64_t> ekey;
    std::vector<uint32_t> faces, forward;
    uint32_t ne = 0;
    {
        const size_t mask = table_size(nc) - 1;
        std::vector<uint32_t> slot(mask + 1, kNoTopoId);
        for (size_t c = 0; c < nc; ++c) {
            const size_t t = c / 3, k = c % 3;
            const uint32_t u = out.vid[c], w = out.vid[t * 3 + (k + 1) % 3];
            if (u == w) continue;
            const uint64_t key = ((uint64_t)std::min(u, w) << 32) | std::max(u, w);
            size_t i = (size_t)mix(key) & mask;
            while (slot[i] != kNoTopoId && ekey[slot[i]] != key) i = (i + 1) & mask;
            if (slot[i] == kNoTopoId) {
                slot[i] = ne++;
                ekey.push_back(key);
                faces.push_back(0);
                forward.push_back(0);
            }
            const uint32_t e = slot[i];
            out.eid[c] = e;
            faces[e]++;
            if (u < w) forward[e]++;
        }
    }
    ekey = std::vector<uint64_t>();

    // ---- the report
    PrtTopologyInfo& I = out.info;
    I.n_vertices = nv;
    I.n_edges = ne;
    for (uint32_t e = 0; e < ne; ++e) {
        if (faces[e] == 1) I.boundary_edges++;
        else if (faces[e] >= 3) I.nonmanifold_edges++;
        else if (forward[e] != 1) I.inconsistent_edges++;
    }
    for (size_t t = 0; t < n_tris; ++t) {
        const double* v = corners + t * stride;
        bool deg = out.eid[t * 3] == kNoTopoId || out.eid[t * 3 + 1] == kNoTopoId || out.eid[t * 3 + 2] == kNoTopoId;
        if (!deg) {
            const double a[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, b[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
            const double n[3] = {a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]};
            deg = n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0;
        }
        if (deg) I.degenerate_tris++;
    }
    I.closed = (I.boundary_edges == 0 && I.nonmanifold_edges == 0 && I.inconsistent_edges == 0) ? 1u : 0u;

    // ---- adjacency: counts, offsets, then the entries in (prim, corner) order - every list ascends
    out.v_start.assign((size_t)nv + 1, 0);
    for (size_t c = 0; c < nc; ++c) out.v_start[(size_t)out.vid[c] + 1]++;
    for (uint32_t v = 0; v < nv; ++v) I.max_valence = std::max<uint64_t>(I.max_valence, out.v_start[(size_t)v + 1]);
    if (!lists) {
        out = MeshTopology{{}, {}, {}, {}, {}, {}, I};
        return;
    }
    prefix(out.v_start);
    out.e_start.assign((size_t)ne + 1, 0);
    for (uint32_t e = 0; e < ne; ++e) out.e_start[(size_t)e + 1] = faces[e];
    prefix(out.e_start);
    out.v_list.assign(nc, 0);
    out.e_list.assign(out.e_start[ne], 0);
    std::vector<uint32_t> vat(out.v_start.begin(), out.v_start.end() - 1), eat(out.e_start.begin(), out.e_start.end() - 1);
    for (size_t c = 0; c < nc; ++c) {
        const uint32_t t = (uint32_t)(c / 3), k = (uint32_t)(c % 3);
        out.v_list[vat[out.vid[c]]++] = (t << 2) | k;
        if (out.eid[c] != kNoTopoId) out.e_list[eat[out.eid[c]]++] = t;
    }
}

} // namespace prt
