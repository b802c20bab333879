// Host-side view-graph helpers shared by the global stages (rotation and
// position averaging): the CSR adjacency over the cameras and union-find.
// Host code only.
#pragma once
#include <cstdint>
#include <numeric>
#include <vector>

namespace sfm {

// Both endpoints of every edge, ascending edge index inside a node.  For the
// edge e = (i, j): the entry (2 e, j) in i's list ("fwd") and (2 e + 1, i) in
// j's ("rev").  adj_start gets N + 1 row starts, ent_code and ent_nbr 2 E items.
inline void build_adjacency(int32_t N, const int32_t *pair_ij, int64_t E, std::vector<int64_t> &adj_start,
                            std::vector<int32_t> &ent_code, std::vector<int32_t> &ent_nbr) {
    adj_start.assign((size_t)N + 1, 0);
    for (int64_t e = 0; e < E; ++e) {
        ++adj_start[(size_t)pair_ij[2 * e] + 1];
        ++adj_start[(size_t)pair_ij[2 * e + 1] + 1];
    }
    for (int32_t n = 0; n < N; ++n) adj_start[(size_t)n + 1] += adj_start[n];
    ent_code.resize((size_t)(2 * E));
    ent_nbr.resize((size_t)(2 * E));
    std::vector<int64_t> fill(adj_start.begin(), adj_start.end() - 1);
    for (int64_t e = 0; e < E; ++e) {
        const int32_t i = pair_ij[2 * e], j = pair_ij[2 * e + 1];
        ent_code[(size_t)fill[i]] = (int32_t)(2 * e);
        ent_nbr[(size_t)fill[i]++] = j;
        ent_code[(size_t)fill[j]] = (int32_t)(2 * e + 1);
        ent_nbr[(size_t)fill[j]++] = i;
    }
}

// union-find over int32 nodes: the root of a set is its lowest node
struct NodeSets {
    std::vector<int32_t> parent;
    explicit NodeSets(int32_t n) : parent((size_t)n) { std::iota(parent.begin(), parent.end(), 0); }
    int32_t find(int32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    }
    void join(int32_t a, int32_t b) {
        a = find(a);
        b = find(b);
        if (a < b) parent[b] = a;
        else parent[a] = b;
    }
};

}  // namespace sfm
