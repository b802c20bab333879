// Stand-alone print of csrc/position_plan.hpp's plan for one solved graph
// (built and run by tests/test_position_plan.py, host only, under ASan +
// UBSan).  No device call.
//
//   position_plan_check n_nodes n_edges path
//
// prints `path_used G nb_group nb_node nb_edge lds_bytes`, or `refused` where
// path 1 is asked for past its bound.
#include <cstdio>
#include <cstdlib>

#include "position_plan.hpp"

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s n_nodes n_edges path\n", argv[0]);
        return 2;
    }
    const long long n_nodes = std::atoll(argv[1]), n_edges = std::atoll(argv[2]), path = std::atoll(argv[3]);
    if (n_nodes < 0 || n_nodes > INT32_MAX || n_edges < 0 || n_edges > (1LL << 30) || path < 0 || path > 2) {
        std::fprintf(stderr, "out of range\n");
        return 2;
    }
    const sfm::PaPlan p = sfm::pa_plan((int32_t)n_nodes, (int64_t)n_edges, (int)path);
    if (!p.fits) {
        std::printf("refused\n");
        return 0;
    }
    std::printf("%d %d %d %d %d %zu\n", p.path, p.G, (int)p.nb_group, (int)p.nb_node, (int)p.nb_edge, p.lds_bytes);
    return 0;
}
