// mesh_topology_sanitize.cpp — a stand-alone driver of build_topology (pooraytracer_amd/csrc/mesh_topology.cpp) for a build
// with -fsanitize=address,undefined (tests/test_signed_distance_cpu.py compiles the two files into one plain executable
// and runs it).  Every shape's counts are checked too, so a clean exit means "no report and the expected topology".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pooraytracer_amd/csrc/mesh_topology.h"

namespace {

using Tris = std::vector<double>; // nine doubles per triangle

void tri(Tris& t, const double* a, const double* b, const double* c) {
    t.insert(t.end(), a, a + 3);
    t.insert(t.end(), b, b + 3);
    t.insert(t.end(), c, c + 3);
}

Tris tetrahedron(bool reverse_first) {
    const double x[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
    const int f[4][3] = {{0, 1, 2}, {0, 3, 1}, {0, 2, 3}, {1, 3, 2}};
    Tris t;
    for (int i = 0; i < 4; ++i)
        if (i == 0 && reverse_first) tri(t, x[f[i][2]], x[f[i][1]], x[f[i][0]]);
        else tri(t, x[f[i][0]], x[f[i][1]], x[f[i][2]]);
    return t;
}

Tris notched_pyramid(int m, double h, double n) {
    const double poly[6][2] = {{0, 0}, {2, 0}, {2, n}, {n, n}, {n, 2}, {0, 2}};
    std::vector<double> ring;
    for (int i = 0; i < 6; ++i) {
        const double *a = poly[i], *b = poly[(i + 1) % 6];
        const int pieces = (i == 2 || i == 3) ? m : 1;
        for (int j = 0; j < pieces; ++j) {
            const double s = (double)j / pieces;
            ring.insert(ring.end(), {a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1]), 0.0});
        }
    }
    const double apex[3] = {n / 2, n / 2, h}, bottom[3] = {n / 2, n / 2, 0.0};
    const size_t r = ring.size() / 3;
    Tris t;
    for (size_t i = 0; i < r; ++i) {
        const double *a = &ring[i * 3], *b = &ring[((i + 1) % r) * 3];
        tri(t, apex, a, b);
        tri(t, bottom, b, a);
    }
    return t;
}

int failures = 0;

void expect(const char* what, const Tris& t, uint64_t nv, uint64_t ne, uint64_t boundary, uint64_t nonmanifold, uint64_t inconsistent,
            uint64_t degenerate, uint64_t valence, uint32_t closed) {
    for (int lists = 0; lists < 2; ++lists) {
        prt::MeshTopology T;
        // a stride beyond nine doubles, as the library's host triangle records have
        const size_t n = t.size() / 9, stride = 11;
        std::vector<double> padded(n * stride + 1, -7.0);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 9; ++k) padded[i * stride + k] = t[i * 9 + k];
        prt::build_topology(padded.data(), stride, n, T, lists != 0);
        const PrtTopologyInfo& I = T.info;
        const bool ok = I.n_vertices == nv && I.n_edges == ne && I.boundary_edges == boundary && I.nonmanifold_edges == nonmanifold &&
                        I.inconsistent_edges == inconsistent && I.degenerate_tris == degenerate && I.max_valence == valence &&
                        I.closed == closed && I.table_bytes == 0;
        bool lists_ok = true;
        if (lists) {
            lists_ok = T.vid.size() == n * 3 && T.eid.size() == n * 3 && T.v_start.size() == nv + 1 && T.e_start.size() == ne + 1 &&
                       T.v_list.size() == n * 3 && T.v_start.back() == n * 3 && T.e_list.size() == T.e_start.back();
            for (size_t v = 0; lists_ok && v < nv; ++v) // every list ascends and names its own vertex
                for (uint32_t i = T.v_start[v]; i < T.v_start[v + 1]; ++i) {
                    const uint32_t e = T.v_list[i];
                    lists_ok = lists_ok && (e >> 2) < n && (e & 3u) < 3 && T.vid[(size_t)(e >> 2) * 3 + (e & 3u)] == v &&
                               (i == T.v_start[v] || T.v_list[i - 1] < e);
                }
            for (size_t e = 0; lists_ok && e < ne; ++e)
                for (uint32_t i = T.e_start[e]; i < T.e_start[e + 1]; ++i) {
                    const uint32_t p = T.e_list[i];
                    lists_ok = lists_ok && p < n && (T.eid[(size_t)p * 3] == e || T.eid[(size_t)p * 3 + 1] == e || T.eid[(size_t)p * 3 + 2] == e) &&
                               (i == T.e_start[e] || T.e_list[i - 1] <= p);
                }
        } else {
            lists_ok = T.vid.empty() && T.v_list.empty() && T.e_list.empty();
        }
        if (!ok || !lists_ok) {
            std::fprintf(stderr, "%s (lists %d): V %llu E %llu boundary %llu nonmanifold %llu inconsistent %llu degenerate %llu valence %llu closed %u%s\n",
                         what, lists, (unsigned long long)I.n_vertices, (unsigned long long)I.n_edges, (unsigned long long)I.boundary_edges,
                         (unsigned long long)I.nonmanifold_edges, (unsigned long long)I.inconsistent_edges,
                         (unsigned long long)I.degenerate_tris, (unsigned long long)I.max_valence, I.closed, lists_ok ? "" : " (bad lists)");
            ++failures;
        }
    }
}

} // namespace

int main() {
    expect("empty", Tris(), 0, 0, 0, 0, 0, 0, 0, 1);
    {
        Tris t;
        const double a[3] = {0, 0, 0}, b[3] = {1, 0, 0}, c[3] = {0, 1, 0};
        tri(t, a, b, c);
        expect("one triangle", t, 3, 3, 3, 0, 0, 0, 1, 0);
    }
    expect("tetrahedron", tetrahedron(false), 4, 6, 0, 0, 0, 0, 3, 1);
    expect("tetrahedron, one face reversed", tetrahedron(true), 4, 6, 0, 0, 3, 0, 3, 0);
    expect("notched pyramid", notched_pyramid(64, 2.0, 0.5), 134, 396, 0, 0, 0, 0, 132, 1);
    {
        // all degenerate: points, two welded corners (one through -0.0), collinear corners
        Tris t;
        const double a[3] = {0.0, 1.0, 2.0}, a2[3] = {-0.0, 1.0, 2.0}, b[3] = {1.0, 1.0, 2.0}, c[3] = {2.0, 1.0, 2.0};
        tri(t, a, a, a);
        tri(t, a, a2, b);
        tri(t, a, b, c);
        // vertices a, b, c; edges ab (twice from triangle 1, once from 2), bc, ca
        expect("all degenerate", t, 3, 3, 2, 1, 0, 3, 6, 0);
    }
    {
        Tris t;
        const double a[3] = {0, 0, 0}, b[3] = {1, 0.25, 0.5}, c[3] = {0.25, 1, 0.75};
        for (int i = 0; i < 3000; ++i) tri(t, a, b, c);
        expect("3000 duplicates", t, 3, 3, 0, 3, 0, 0, 3000, 0);
    }
    if (failures) return 1;
    std::puts("mesh_topology: ok");
    return 0;
}
