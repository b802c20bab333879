// Global rotation averaging: every camera's rotation from the relative
// rotations of the verified pairs, in one call (sfm_average_rotations; the
// definitions are in include/sfmcore.h).  The reference has no counterpart.
//
// Host: argument checks, the CSR adjacency (both endpoints of every edge,
// ascending edge index), components and roots by union-find, the node lists by
// degree; after the download the groups of the inlier graph, again union-find.
//
//   k_ra_bfs        a thread per node, one launch per level: a node not yet
//                   reached looks for neighbours on level l and takes the entry
//                   of smallest (priority, e).  Levels past the deepest return
//                   at once (a device word holds the deepest level reached).
//   k_ra_consensus  the hot path: one workgroup of T = 64 / 128 / 256 threads
//                   per node by degree.  Thread a keeps P_a in registers; the
//                   P_b pass through LDS in tiles of T 72-byte records that
//                   every lane reads at the same address (a broadcast: no bank
//                   is hit twice; the writes, one record per lane at a stride
//                   of 18 dwords, are conflict-free over the 16 lanes of a
//                   ds_write_b64 group).  A node of more than T entries walks
//                   the (a, b) tiles and forms each tile's predictions again
//                   from global memory.  The winner is an integer maximum of
//                   (support, lowest a); thread 0 writes its prediction.
//   k_ra_refit      a thread per node: the weighted mean of the logs of the
//                   passing entries in CSR order (a serial sum by definition),
//                   R <- exp(omega) R, and the sweep's largest |omega| as an
//                   integer maximum over the doubles' bits.  A sweep first
//                   tests the one before it: once stopped, every later launch
//                   only copies its nodes through.
//   k_ra_edges      a thread per edge: the angle and the inlier flag on the
//                   final rotations.
//
// Every decision is an integer or one thread's fp64 expression in a fixed
// order, so the outputs do not depend on how the work is spread.
#include <cmath>
#include <cstring>

#include "staging.hpp"
#include "view_graph.hpp"

namespace sfm {

constexpr int RA_THREADS = 256;   // the per-node and per-edge kernels
constexpr int RA_BFS_BATCH = 8;   // levels launched between two looks at the deepest level
constexpr int RA_REFIT_BATCH = 8; // refit sweeps launched between two looks at the stop flags

struct RaGraph {
    const int64_t *adj_start;  // N + 1
    const int32_t *ent_code;   // 2 e + (0 fwd: predicts R_rel^T R_nbr, 1 rev: R_rel R_nbr)
    const int32_t *ent_nbr;
    const double *R_rel;       // E x 9
};

__host__ __device__ inline uint64_t ra_priority(uint64_t seed, uint64_t e) {
    uint64_t z = seed + (e + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// entry k's prediction from the neighbour's rotation in Rcur
__device__ __forceinline__ void ra_predict(const RaGraph &g, int64_t k, const double *__restrict__ Rcur,
                                           double (&P)[9]) {
#pragma clang fp contract(off)
    const int32_t code = g.ent_code[k];
    const double *A = g.R_rel + 9 * (int64_t)(code >> 1);
    const double *B = Rcur + 9 * (int64_t)g.ent_nbr[k];
    double a[9], b[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        a[j] = A[j];
        b[j] = B[j];
    }
    const bool rev = code & 1;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a0 = rev ? a[3 * r] : a[r], a1 = rev ? a[3 * r + 1] : a[3 + r];
            const double a2 = rev ? a[3 * r + 2] : a[6 + r];
            P[3 * r + c] = (a0 * b[c] + a1 * b[3 + c]) + a2 * b[6 + c];
        }
}

// the nine products of tr(P Q^T), added left to right
__device__ __forceinline__ double ra_trace(const double (&p)[9], const double *q) {
#pragma clang fp contract(off)
    double t = p[0] * q[0];
#pragma unroll
    for (int j = 1; j < 9; ++j) t = t + p[j] * q[j];
    return t;
}

// entry (r, c) of M = P R^T
__device__ __forceinline__ double ra_mrc(const double (&P)[9], const double (&R)[9], int r, int c) {
#pragma clang fp contract(off)
    return (P[3 * r] * R[3 * c] + P[3 * r + 1] * R[3 * c + 1]) + P[3 * r + 2] * R[3 * c + 2];
}

// M = P R^T: the axis part v of M and its norm s
__device__ __forceinline__ double ra_axis(const double (&P)[9], const double (&R)[9], double (&v)[3]) {
#pragma clang fp contract(off)
    v[0] = (ra_mrc(P, R, 2, 1) - ra_mrc(P, R, 1, 2)) / 2.0;
    v[1] = (ra_mrc(P, R, 0, 2) - ra_mrc(P, R, 2, 0)) / 2.0;
    v[2] = (ra_mrc(P, R, 1, 0) - ra_mrc(P, R, 0, 1)) / 2.0;
    return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

__global__ __launch_bounds__(RA_THREADS) void k_ra_bfs(RaGraph g, int32_t n_nodes, uint64_t seed, int32_t l,
                                                       int32_t *level, double *R, int32_t *deepest) {
    if (*deepest < l) return;  // nobody is on level l: the tree is complete
    const int32_t n = blockIdx.x * RA_THREADS + threadIdx.x;
    if (n >= n_nodes || level[n] >= 0) return;
    int64_t best_k = -1;
    uint64_t best_p = 0;
    for (int64_t k = g.adj_start[n]; k < g.adj_start[n + 1]; ++k) {
        // a neighbour joining level l + 1 in this launch reads as -1 or l + 1, never as l
        if (level[g.ent_nbr[k]] != l) continue;
        const uint64_t p = ra_priority(seed, (uint64_t)(g.ent_code[k] >> 1));
        if (best_k < 0 || p < best_p) {  // entries ascend in e: the first of equal priority stays
            best_k = k;
            best_p = p;
        }
    }
    if (best_k < 0) return;
    double P[9];
    ra_predict(g, best_k, R, P);  // the neighbour's rotation is final since level l was written
#pragma unroll
    for (int j = 0; j < 9; ++j) R[9 * (int64_t)n + j] = P[j];
    level[n] = l + 1;
    *deepest = l + 1;  // every writer of this launch stores the same value
}

template <int T>
__global__ __launch_bounds__(T) void k_ra_consensus(RaGraph g, const int32_t *__restrict__ nodes,
                                                    const double *__restrict__ Rprev, double *__restrict__ Rnext,
                                                    double tau) {
    __shared__ double tile[T * 9];
    __shared__ unsigned long long wave_best[T / 64];
    const int tid = threadIdx.x;
    const int32_t n = nodes[blockIdx.x];
    const int64_t k0 = g.adj_start[n];
    const int32_t d = (int32_t)(g.adj_start[n + 1] - k0);  // >= 1: the lists hold no root, and only roots lack edges
    unsigned long long best = 0;
    for (int32_t a0 = 0; a0 < d; a0 += T) {
        const int32_t a = a0 + tid;
        const bool has = a < d;
        double p[9];
        if (has) ra_predict(g, k0 + a, Rprev, p);
        int32_t support = 0;
        for (int32_t b0 = 0; b0 < d; b0 += T) {
            __syncthreads();  // the tile before has been read
            const int32_t b = b0 + tid;
            if (b < d) {
                double q[9];
                if (b0 == a0) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) q[j] = p[j];
                } else {
                    ra_predict(g, k0 + b, Rprev, q);
                }
#pragma unroll
                for (int j = 0; j < 9; ++j) tile[9 * tid + j] = q[j];
            }
            __syncthreads();
            const int32_t nb = min(T, d - b0);
            if (has)
                for (int32_t j = 0; j < nb; ++j) support += ra_trace(p, tile + 9 * j) >= tau ? 1 : 0;
        }
        if (has) {  // most support, then the lowest a
            const unsigned long long key = ((unsigned long long)support << 32) | (0xFFFFFFFFu - (uint32_t)a);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), off, 64), lo = __shfl_xor((uint32_t)best, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) wave_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < T / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
        const int32_t a = (int32_t)(0xFFFFFFFFu - (uint32_t)best);
        double p[9];
        ra_predict(g, k0 + a, Rprev, p);  // the same expression as its owner's: the same bits
#pragma unroll
        for (int j = 0; j < 9; ++j) Rnext[9 * (int64_t)n + j] = p[j];
    }
}

__global__ __launch_bounds__(RA_THREADS) void k_ra_refit(RaGraph g, const int32_t *__restrict__ nodes, int32_t n_list,
                                                         const double *__restrict__ weight,
                                                         const double *__restrict__ Rprev, double *__restrict__ Rnext,
                                                         double tau, double tol, int32_t sweep,
                                                         unsigned long long *max_bits, int32_t *stopped) {
#pragma clang fp contract(off)
    // the sweep before, complete since its launch ended: did it, or one before it, end the refit?
    const bool stop = sweep > 0 && (stopped[sweep - 1] != 0 ||
                                    (tol > 0.0 && __longlong_as_double((long long)max_bits[sweep - 1]) <= tol));
    const int32_t idx = blockIdx.x * RA_THREADS + threadIdx.x;
    if (idx == 0) stopped[sweep] = stop ? 1 : 0;
    double theta_w = 0.0;
    if (idx < n_list) {
        const int32_t n = nodes[idx];
        double R[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = Rprev[9 * (int64_t)n + j];
        if (!stop) {
            double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
            for (int64_t k = g.adj_start[n]; k < g.adj_start[n + 1]; ++k) {
                double P[9], v[3];
                ra_predict(g, k, Rprev, P);
                const double t = ra_trace(P, R);
                if (!(t >= tau)) continue;
                const double s = ra_axis(P, R, v);
                const double theta = atan2(s, (t - 1.0) / 2.0);
                const double f = s > 0.0 ? theta / s : 1.0;
                const double w = weight ? weight[g.ent_code[k] >> 1] : 1.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) num[j] = num[j] + w * (v[j] * f);
                den = den + w;
            }
            if (den > 0.0) {
                const double o0 = num[0] / den, o1 = num[1] / den, o2 = num[2] / den;
                const double th2 = (o0 * o0 + o1 * o1) + o2 * o2;
                theta_w = sqrt(th2);
                double A, B;
                if (theta_w < 1e-4) {
                    A = 1.0 - th2 / 6.0;
                    B = 0.5 - th2 / 24.0;
                } else {
                    const double sh = sin(theta_w / 2.0);
                    A = sin(theta_w) / theta_w;
                    B = (2.0 * sh * sh) / th2;
                }
                // exp = I + A [o]x + B ([o]x)^2, ([o]x)^2 = o o^T - |o|^2 I
                const double o[3] = {o0, o1, o2};
                double Ex[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) Ex[3 * r + c] = B * (o[r] * o[c]) + (r == c ? 1.0 - B * th2 : 0.0);
                Ex[1] = Ex[1] - A * o2;
                Ex[2] = Ex[2] + A * o1;
                Ex[3] = Ex[3] + A * o2;
                Ex[5] = Ex[5] - A * o0;
                Ex[6] = Ex[6] - A * o1;
                Ex[7] = Ex[7] + A * o0;
                double Rn[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        Rn[3 * r + c] = (Ex[3 * r] * R[c] + Ex[3 * r + 1] * R[3 + c]) + Ex[3 * r + 2] * R[6 + c];
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = Rn[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) Rnext[9 * (int64_t)n + j] = R[j];
    }
    // the largest |omega| of the sweep: non-negative doubles order as their bits
    unsigned long long bits = (unsigned long long)__double_as_longlong(theta_w);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(bits >> 32), off, 64), lo = __shfl_xor((uint32_t)bits, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(max_bits + sweep, bits);
}

__global__ __launch_bounds__(RA_THREADS) void k_ra_edges(const int32_t *__restrict__ pair_ij,
                                                         const double *__restrict__ R_rel, int64_t n_edges,
                                                         const double *__restrict__ R, double tau,
                                                         double *edge_angle, uint8_t *edge_inlier) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const double *A = R_rel + 9 * e, *B = R + 9 * (int64_t)pair_ij[2 * e];
    double P[9], Rj[9], v[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) P[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
#pragma unroll
    for (int j = 0; j < 9; ++j) Rj[j] = R[9 * (int64_t)pair_ij[2 * e + 1] + j];
    const double t = ra_trace(P, Rj);
    const double s = ra_axis(P, Rj, v);
    edge_angle[e] = atan2(s, (t - 1.0) / 2.0);
    edge_inlier[e] = t >= tau ? 1 : 0;
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_average_rotations(int32_t n_images, const int32_t *pair_ij, const double *R_rel,
                                     const double *weight, int64_t n_edges, uint64_t seed, double threshold,
                                     int32_t consensus_sweeps, int32_t max_sweeps, double tol, double *R,
                                     double *edge_angle, uint8_t *edge_inlier, int32_t *n_inlier_edges, int32_t *group,
                                     int32_t *info, int32_t *level, int32_t *sweeps, int device) {
    const int32_t N = n_images;
    const int64_t E = n_edges;
    SFM_CHECK_ARG(N >= 0 && E >= 0, "n_images < 0 or n_edges < 0");
    SFM_CHECK_ARG(E <= (int64_t)1 << 30, "more than 2^30 edges");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0 && threshold < M_PI, "threshold must lie in (0, pi)");
    SFM_CHECK_ARG(consensus_sweeps >= 0 && max_sweeps >= 0, "consensus_sweeps < 0 or max_sweeps < 0");
    SFM_CHECK_ARG(tol >= 0.0, "tol must be >= 0");
    SFM_CHECK_ARG(E == 0 || (pair_ij && R_rel), "null pointer");
    SFM_CHECK_ARG(sweeps && (N == 0 || (R && n_inlier_edges && group && info && level)) &&
                      (E == 0 || (edge_angle && edge_inlier)),
                  "null pointer");
    for (int64_t e = 0; e < E; ++e) {
        const int32_t i = pair_ij[2 * e], j = pair_ij[2 * e + 1];
        SFM_CHECK_ARG(i >= 0 && i < N && j >= 0 && j < N, "a pair image outside [0, n_images)");
        SFM_CHECK_ARG(i != j, "a pair of an image with itself");
        for (int k = 0; k < 9; ++k) SFM_CHECK_ARG(std::isfinite(R_rel[9 * e + k]), "R_rel is not finite");
        SFM_CHECK_ARG(!weight || (std::isfinite(weight[e]) && weight[e] > 0.0), "a weight is not finite and positive");
    }

    *sweeps = 0;
    if (N == 0) return 0;
    // adjacency: both endpoints of every edge, ascending e inside a node
    std::vector<int64_t> adj_start;
    std::vector<int32_t> ent_code, ent_nbr;  // fwd: R_i = R_rel^T R_j; rev: R_j = R_rel R_i
    build_adjacency(N, pair_ij, E, adj_start, ent_code, ent_nbr);
    // components of the input graph and their roots: highest degree, lowest index on ties
    std::vector<int32_t> root_of((size_t)N), is_root((size_t)N, 0);
    {
        NodeSets sets(N);
        for (int64_t e = 0; e < E; ++e) sets.join(pair_ij[2 * e], pair_ij[2 * e + 1]);
        std::vector<int32_t> best((size_t)N, -1);
        for (int32_t n = 0; n < N; ++n) {
            const int32_t c = sets.find(n);
            const int64_t dn = adj_start[(size_t)n + 1] - adj_start[n];
            if (best[c] < 0 || dn > adj_start[(size_t)best[c] + 1] - adj_start[best[c]]) best[c] = n;
        }
        for (int32_t n = 0; n < N; ++n) root_of[n] = best[sets.find(n)];
        for (int32_t n = 0; n < N; ++n) is_root[root_of[n]] = 1;
    }
    if (E == 0) {
        for (int32_t n = 0; n < N; ++n) {
            for (int k = 0; k < 9; ++k) R[9 * (size_t)n + k] = k % 4 == 0 ? 1.0 : 0.0;
            n_inlier_edges[n] = 0;
            group[n] = n;
            info[n] = -1;
            level[n] = 0;
        }
        return 0;
    }
    // the nodes that move, by the workgroup their degree asks for; all of them, ascending, for the refit
    std::vector<int32_t> list[4];
    for (int32_t n = 0; n < N; ++n) {
        if (is_root[n]) continue;
        const int64_t dn = adj_start[(size_t)n + 1] - adj_start[n];
        list[dn <= 64 ? 0 : dn <= 128 ? 1 : 2].push_back(n);
        list[3].push_back(n);
    }
    std::vector<double> R0((size_t)N * 9, 0.0);
    std::vector<int32_t> level0((size_t)N, -1);
    for (int32_t n = 0; n < N; ++n) {
        if (!is_root[n]) continue;
        R0[9 * (size_t)n] = R0[9 * (size_t)n + 4] = R0[9 * (size_t)n + 8] = 1.0;
        level0[n] = 0;
    }
    const double tau = 1.0 + 2.0 * std::cos(threshold);

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_ij = in.add<int32_t>(2 * E);
    const auto i_rel = in.add<double>(9 * E), i_w = in.add<double>(weight ? E : 0);
    const auto i_adj = in.add<int64_t>((size_t)N + 1);
    const auto i_code = in.add<int32_t>(2 * E), i_nbr = in.add<int32_t>(2 * E);
    Slot<int32_t> i_list[4];
    for (int k = 0; k < 4; ++k) i_list[k] = in.add<int32_t>(list[k].size());
    const auto o_R = out.add<double>(9 * (size_t)N), o_ang = out.add<double>(E);
    const auto o_inl = out.add<uint8_t>(E);
    const auto o_level = out.add<int32_t>(N);
    const auto w_R = work.add<double>(9 * (size_t)N);  // the other half of the double buffer
    const auto w_max = work.add<unsigned long long>((size_t)max_sweeps + 1);
    const auto w_stop = work.add<int32_t>((size_t)max_sweeps + 1);
    const auto w_deep = work.add<int32_t>(1);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    const bool timed = call_timing();
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_ij, pair_ij, s));
    SFM_TRY(in.upload(i_rel, R_rel, s));
    SFM_TRY(in.upload(i_w, weight, s));
    SFM_TRY(in.upload(i_adj, adj_start.data(), s));
    SFM_TRY(in.upload(i_code, ent_code.data(), s));
    SFM_TRY(in.upload(i_nbr, ent_nbr.data(), s));
    for (int k = 0; k < 4; ++k) SFM_TRY(in.upload(i_list[k], list[k].data(), s));
    SFM_TRY(out.upload(o_R, R0.data(), s));
    SFM_TRY(out.upload(o_level, level0.data(), s));
    SFM_HIP(hipMemsetAsync(work.ptr(w_max), 0, w_max.bytes(), s));
    SFM_HIP(hipMemsetAsync(work.ptr(w_stop), 0, w_stop.bytes(), s));
    SFM_HIP(hipMemsetAsync(work.ptr(w_deep), 0, sizeof(int32_t), s));
    SFM_TRY(tm.mark(s));

    const RaGraph g{in.ptr(i_adj), in.ptr(i_code), in.ptr(i_nbr), in.ptr(i_rel)};
    double *buf[2] = {out.ptr(o_R), work.ptr(w_R)};
    int cur = 0;  // buf[cur] holds the current rotations
    const dim3 T(RA_THREADS), g_nodes((unsigned)ceil_div(N, RA_THREADS));

    // stage 1: a level per launch; the deepest level reached is looked at every RA_BFS_BATCH levels
    for (int32_t l = 0; l < N - 1;) {
        const int32_t l_end = (int32_t)std::min<int64_t>((int64_t)l + RA_BFS_BATCH, (int64_t)N - 1);
        for (; l < l_end; ++l) {
            hipLaunchKernelGGL(k_ra_bfs, g_nodes, T, 0, s, g, N, seed, l, out.ptr(o_level), buf[0], work.ptr(w_deep));
            SFM_HIP(hipGetLastError());
        }
        int32_t deepest = 0;
        SFM_TRY(work.download(&deepest, w_deep, s));
        SFM_HIP(hipStreamSynchronize(s));
        if (deepest < l) break;  // the last launch found nobody
    }
    SFM_HIP(hipMemcpyAsync(buf[1], buf[0], o_R.bytes(), hipMemcpyDeviceToDevice, s));  // the roots, in both halves

    // stage 2
    if (timed) SFM_HIP(hipEventRecord(c->ev[5], s));
    for (int32_t it = 0; it < consensus_sweeps; ++it) {
        if (!list[0].empty())
            hipLaunchKernelGGL(k_ra_consensus<64>, dim3((unsigned)list[0].size()), dim3(64), 0, s, g, in.ptr(i_list[0]),
                               buf[cur], buf[cur ^ 1], tau);
        if (!list[1].empty())
            hipLaunchKernelGGL(k_ra_consensus<128>, dim3((unsigned)list[1].size()), dim3(128), 0, s, g,
                               in.ptr(i_list[1]), buf[cur], buf[cur ^ 1], tau);
        if (!list[2].empty())
            hipLaunchKernelGGL(k_ra_consensus<256>, dim3((unsigned)list[2].size()), dim3(256), 0, s, g,
                               in.ptr(i_list[2]), buf[cur], buf[cur ^ 1], tau);
        SFM_HIP(hipGetLastError());
        cur ^= 1;
    }
    if (timed) SFM_HIP(hipEventRecord(c->ev[6], s));

    // stage 3: a sweep per launch; the stop flags are looked at every RA_REFIT_BATCH sweeps
    int32_t n_run = 0;
    if (!list[3].empty()) {
        const dim3 g_list((unsigned)ceil_div((int64_t)list[3].size(), RA_THREADS));
        std::vector<int32_t> stopped((size_t)max_sweeps + 1, 0);
        for (int32_t it = 0; it < max_sweeps;) {
            const int32_t it_end = std::min(it + RA_REFIT_BATCH, max_sweeps);
            const int32_t first = it;
            for (; it < it_end; ++it) {
                hipLaunchKernelGGL(k_ra_refit, g_list, T, 0, s, g, in.ptr(i_list[3]), (int32_t)list[3].size(),
                                   weight ? in.ptr(i_w) : (const double *)nullptr, buf[cur], buf[cur ^ 1], tau, tol, it,
                                   work.ptr(w_max), work.ptr(w_stop));
                SFM_HIP(hipGetLastError());
                cur ^= 1;
            }
            if (tol > 0.0) {
                SFM_TRY(work.download(stopped.data() + first, w_stop, (size_t)first, (size_t)(it_end - first), s));
                SFM_HIP(hipStreamSynchronize(s));
            }
            for (int32_t k = first; k < it_end; ++k) n_run += stopped[k] ? 0 : 1;
            // the last sweep launched may have been the one that met tol: the next launch would say so
            if (stopped[it_end - 1]) break;
        }
    }
    hipLaunchKernelGGL(k_ra_edges, dim3((unsigned)ceil_div(E, RA_THREADS)), T, 0, s, in.ptr(i_ij), in.ptr(i_rel), E,
                       buf[cur], tau, out.ptr(o_ang), out.ptr(o_inl));
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));

    if (cur == 0) SFM_TRY(out.download(R, o_R, s));
    else SFM_TRY(work.download(R, w_R, s));
    SFM_TRY(out.download(edge_angle, o_ang, s));
    SFM_TRY(out.download(edge_inlier, o_inl, s));
    SFM_TRY(out.download(level, o_level, s));
    SFM_TRY(tm.finish(s));
    if (timed) {  // [3]: the consensus kernels alone
        float t[4] = {0, 0, 0, 0};
        for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&t[k], c->ev[k], c->ev[k + 1]);
        (void)hipEventElapsedTime(&t[3], c->ev[5], c->ev[6]);
        const double t4[4] = {t[0], t[1], t[2], t[3]};
        set_timings(t4, 4);
    }
    *sweeps = n_run;

    // the inlier graph: counts, groups, info
    NodeSets sets(N);
    for (int32_t n = 0; n < N; ++n) n_inlier_edges[n] = 0;
    for (int64_t e = 0; e < E; ++e) {
        if (!edge_inlier[e]) continue;
        ++n_inlier_edges[pair_ij[2 * e]];
        ++n_inlier_edges[pair_ij[2 * e + 1]];
        sets.join(pair_ij[2 * e], pair_ij[2 * e + 1]);
    }
    for (int32_t n = 0; n < N; ++n) {
        group[n] = sets.find(n);
        const bool edges = adj_start[(size_t)n + 1] > adj_start[n];
        info[n] = is_root[n] && edges ? 1 : n_inlier_edges[n] > 0 ? 0 : -1;
    }
    return 0;
}
