// mesh_topology.h — the weld, the vertex and edge ids and the adjacency lists behind the signed distance queries
// (prt_scene_set_signed_queries, include/prt.h).  Plain C++: no HIP, no other project header but prt.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/prt.h"

namespace prt {

constexpr uint32_t kNoTopoId = 0xffffffffu; // an edge whose two ends welded to one vertex has no id

struct MeshTopology {
    // per triangle, in description (prim) order
    std::vector<uint32_t> vid; // [n_tris][3]
    std::vector<uint32_t> eid; // [n_tris][3]: edge v0v1, v1v2, v2v0; kNoTopoId where the ends welded
    // CSR adjacency, each list ascending
    std::vector<uint32_t> v_start, v_list; // vertex -> (prim << 2 | corner); v_start has n_vertices + 1 entries
    std::vector<uint32_t> e_start, e_list; // edge -> prim; e_start has n_edges + 1 entries
    PrtTopologyInfo info;                  // table_bytes = 0: the caller knows what it uploaded
};

// corners: the first of n_tris records of `stride` doubles each, whose first nine doubles are v0, v1, v2.
// `lists` false: only `info` is filled (the ids and lists are made on the way and dropped).
// Throws std::bad_alloc; n_tris < 2^29 (the BVH's own limit) is the caller's business.
void build_topology(const double* corners, size_t stride, size_t n_tris, MeshTopology& out, bool lists = true);

} // namespace prt
