// Host-side plan of position averaging (position_averaging.hip): which path
// runs, the lanes G that walk a node's entries, path 2's three grids and path
// 1's dynamic LDS request, all from the size of the solved graph.  No HIP call
// and no device code: tests/position_plan_check.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sfm {

constexpr int PA_MAX_NODES = 512;  // path 1: solved nodes, the root included (SFM_POSITIONS_PATH1_MAX_NODES)
constexpr int PA_T1 = 512;         // path 1's workgroup: at 1024 the kernel's 166 VGPRs would spill
constexpr int PA_T2 = 256;         // path 2's workgroups
constexpr int PA_NODE_LDS = 168;   // path 1: x, r, p, z, q (3 doubles each) and the six entries of D^-1 per node

struct PaPlan {
    int path;                            // 0: nothing to solve, 1, 2
    bool fits;                           // false: path 1 was asked for past its bound (SFM_ERR_ARG)
    int G;                               // lanes per node
    int32_t nb_group, nb_node, nb_edge;  // path 2's grids: groups of G lanes per node, a thread per node, per edge
    size_t lds_bytes;                    // path 1's dynamic LDS
};

// lanes per node: the power of two next above an eighth of the mean entries per node, 1 .. 64; for path 1
// no more than fills its one workgroup once
inline int pa_group_lanes(int64_t n_entries, int32_t n_nodes, bool one_workgroup) {
    int G = 1;
    while (G < 64 && (int64_t)G * 8 * n_nodes < n_entries) G *= 2;
    if (one_workgroup)
        while (G > 1 && (int64_t)G * n_nodes > PA_T1) G /= 2;
    return G;
}

// the path that runs for `path` asked (0: chosen here) on n_nodes solved nodes
inline int pa_choose_path(int32_t n_nodes, int path) {
    return n_nodes == 0 ? 0 : path ? path : n_nodes <= PA_MAX_NODES ? 1 : 2;
}

inline int32_t pa_blocks(int64_t n, int64_t per_block) { return (int32_t)((n + per_block - 1) / per_block); }

// the plan of a solved graph of n_nodes nodes and n_edges edges (2 n_edges entries)
inline PaPlan pa_plan(int32_t n_nodes, int64_t n_edges, int path) {
    PaPlan p{};
    p.path = pa_choose_path(n_nodes, path);
    p.fits = !(p.path == 1 && n_nodes > PA_MAX_NODES);
    if (p.path == 0 || !p.fits) return p;
    p.G = pa_group_lanes(2 * n_edges, n_nodes, p.path == 1);
    p.nb_group = pa_blocks((int64_t)n_nodes * p.G, PA_T2);
    p.nb_node = pa_blocks(n_nodes, PA_T2);
    p.nb_edge = pa_blocks(n_edges, PA_T2);
    p.lds_bytes = p.path == 1 ? (size_t)n_nodes * PA_NODE_LDS + 3 * (PA_T1 / 64) * sizeof(double) : 0;
    return p;
}

}  // namespace sfm
