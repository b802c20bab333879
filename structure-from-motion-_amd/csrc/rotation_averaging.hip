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
// sfm_average_rotations_cg replaces the refit sweeps by Gauss-Newton rounds,
// each a conjugate-gradient solve shaped like position averaging's path 2:
//
//   k_rc_edges      a thread per edge: a_e w_e (the trace test) and g_e, the log
//                   of the edge's residual rotation.
//   k_rc_gather     G lanes per node: D, b, D^-1, r, z and the partials of |b|^2
//                   and r.z; a root and a node without an active entry get
//                   D^-1 = 0 and are no unknowns.
//   k_rc_apply      iteration k: every workgroup adds the partials of the launch
//                   before in their order, tests the stop, forms p = z + beta
//                   p_old for its nodes and their neighbours, applies the
//                   operator, leaves partials of p.q.
//   k_rc_update     alpha, x, r, z and the partials of r.z and |r|^2.
//   k_rc_retract    R <- exp(x) R and the round's largest |x|, an integer
//                   maximum as the refit's.
//
// Every decision is an integer or one thread's fp64 expression in a fixed
// order, so the outputs do not depend on how the work is spread.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fixed_sums.hpp"
#include "position_plan.hpp"
#include "staging.hpp"
#include "view_graph.hpp"

namespace sfm {

constexpr int RA_THREADS = 256;   // the per-node and per-edge kernels
constexpr int RA_BFS_BATCH = 8;   // levels launched between two looks at the deepest level
constexpr int RA_REFIT_BATCH = 8; // refit sweeps launched between two looks at the stop flags
constexpr int RC_CG_BATCH = 8;    // CG iterations launched between two looks at the stop word

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

// R <- exp(o) R, exp(o) = I + A [o]x + B ([o]x)^2 with ([o]x)^2 = o o^T - |o|^2 I; returns |o|
__device__ __forceinline__ double ra_retract(const double (&o)[3], double (&R)[9]) {
#pragma clang fp contract(off)
    const double o0 = o[0], o1 = o[1], o2 = o[2];
    const double th2 = (o0 * o0 + o1 * o1) + o2 * o2;
    const double theta_w = sqrt(th2);
    double A, B;
    if (theta_w < 1e-4) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        const double sh = sin(theta_w / 2.0);
        A = sin(theta_w) / theta_w;
        B = (2.0 * sh * sh) / th2;
    }
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
    return theta_w;
}

// the log of M = P Q^T by the stage-3 formulas, t the trace sum of P against Q: v theta / s, v where s = 0
__device__ __forceinline__ void ra_log(const double (&P)[9], const double (&Q)[9], double t, double (&g)[3]) {
#pragma clang fp contract(off)
    double v[3];
    const double s = ra_axis(P, Q, v);
    const double theta = atan2(s, (t - 1.0) / 2.0);
    const double f = s > 0.0 ? theta / s : 1.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] = v[j] * f;
}

// P = R_rel[e] R[i]
__device__ __forceinline__ void ra_edge_product(const double *__restrict__ A, const double *__restrict__ B,
                                                double (&P)[9]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) P[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
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
                const double o[3] = {num[0] / den, num[1] / den, num[2] / den};
                theta_w = ra_retract(o, R);
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

// ------------------------------------------------------------------ the Gauss-Newton CG refit
// A round: k_rc_edges (a thread per edge: a_e w_e and g_e), k_rc_gather (G lanes per node: b, D^-1, r, z and the
// partials of |b|^2, r.z, |r|^2), per CG iteration k_rc_apply and k_rc_update, then k_rc_retract.
struct RcState {
    double rho[2];  // r.z of iteration k in slot k & 1
    int32_t stopped, pad;
};

struct RcBufs {
    const int32_t *ij;      // E x 2
    const double *weight;   // E or null
    const int32_t *level;   // N: 0 marks a root
    double *aw, *g;         // E: a_e w_e; E x 3: g_e
    double *x, *r, *z, *q, *p[2], *Dinv;  // N x 3 each, Dinv N: 0 marks a node that is no unknown
    double *part_bb, *part_rz, *part_rr, *part_pq;
    RcState *st;
    int32_t *cg_iters;
    double *cg_residual;
    unsigned long long *step_bits;
    int32_t n_nodes, G;
    int64_t n_edges;
    int32_t nb_group, nb_node;  // the grids: groups of G lanes per node, a thread per node
};

// one read of the stop word per workgroup, so that all its waves agree (see pa_halted)
__device__ __forceinline__ bool rc_halted(const RcState *st) {
    __shared__ int32_t halt;
    if (threadIdx.x == 0) halt = st->stopped;
    __syncthreads();
    return halt != 0;
}

// y = A v (A row-major 3 x 3), or A^T v
__device__ __forceinline__ void rc_mul(const double *__restrict__ A, const double (&v)[3], bool transposed,
                                       double (&y)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        y[r] = transposed ? (A[r] * v[0] + A[3 + r] * v[1]) + A[6 + r] * v[2]
                          : (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}

__global__ __launch_bounds__(RA_THREADS) void k_rc_edges(RcBufs b, const double *__restrict__ R_rel,
                                                         const double *__restrict__ R, double tau) {
    const int64_t e = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x;
    if (e >= b.n_edges) return;
    double P[9], Rj[9], g[3];
    ra_edge_product(R_rel + 9 * e, R + 9 * (int64_t)b.ij[2 * e], P);
#pragma unroll
    for (int j = 0; j < 9; ++j) Rj[j] = R[9 * (int64_t)b.ij[2 * e + 1] + j];
    const double t = ra_trace(P, Rj);
    ra_log(P, Rj, t, g);
    b.aw[e] = t >= tau ? (b.weight ? b.weight[e] : 1.0) : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) b.g[3 * e + j] = g[j];
}

__global__ __launch_bounds__(RA_THREADS) void k_rc_gather(RaGraph gr, RcBufs b) {
    __shared__ double words[3 * (RA_THREADS / 64)];
    const int tid = threadIdx.x, G = b.G, g = tid & (G - 1);
    const int32_t n = (int32_t)(((int64_t)blockIdx.x * RA_THREADS + tid) / G);
    const bool inside = n < b.n_nodes;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, t3[3] = {0.0, 0.0, 0.0};  // a: D_n, b_n
    if (inside && b.level[n] != 0) {
        const int64_t k1 = gr.adj_start[n + 1];
        for (int64_t k = gr.adj_start[n] + g; k < k1; k += G) {
            const int32_t code = gr.ent_code[k];
            const int64_t e = code >> 1;
            const double w = b.aw[e];
            if (w == 0.0) continue;
            const double ge[3] = {b.g[3 * e], b.g[3 * e + 1], b.g[3 * e + 2]};
            a[0] += w;
            if (code & 1) {  // the node is the edge's j
                for (int i = 0; i < 3; ++i) a[1 + i] += w * ge[i];
            } else {
                double y[3];
                rc_mul(gr.R_rel + 9 * e, ge, true, y);
                for (int i = 0; i < 3; ++i) a[1 + i] -= w * y[i];
            }
        }
    }
    pa_group_sum<4>(a, G);
    if (g == 0 && inside) {
        const bool live = a[0] > 0.0;  // a root and a node without an active entry summed nothing
        const double dinv = live ? 1.0 / a[0] : 0.0;
        b.Dinv[n] = dinv;
        for (int i = 0; i < 3; ++i) {
            const double ri = live ? a[1 + i] : 0.0, zi = dinv * ri;
            b.r[3 * (int64_t)n + i] = ri;
            b.z[3 * (int64_t)n + i] = zi;
            b.x[3 * (int64_t)n + i] = b.q[3 * (int64_t)n + i] = 0.0;
            b.p[0][3 * (int64_t)n + i] = b.p[1][3 * (int64_t)n + i] = 0.0;
            t3[0] += ri * ri;
            t3[1] += ri * zi;
        }
        t3[2] = t3[0];  // r = b
    }
    pa_block_sum<3>(t3, words);
    if (tid == 0) {
        b.part_bb[blockIdx.x] = t3[0];
        b.part_rz[blockIdx.x] = t3[1];
        b.part_rr[blockIdx.x] = t3[2];
        if (blockIdx.x == 0) b.st->stopped = 0;
    }
}

// iteration k: the stop test on the sums of the launch before, p = z + beta p_old, q = A p, partials of p.q
__global__ __launch_bounds__(RA_THREADS) void k_rc_apply(RaGraph gr, RcBufs b, double cg_tol, int32_t cg_max_iters,
                                                         int32_t round, int32_t k) {
    __shared__ double words[2 * (RA_THREADS / 64)];
    if (rc_halted(b.st)) return;
    const int tid = threadIdx.x, G = b.G, g = tid & (G - 1);
    double t1[1], t2[2];
    const double *const p1[1] = {b.part_bb};
    const double *const p2[2] = {b.part_rz, b.part_rr};
    pa_resum<1>(t1, p1, b.nb_group, words);
    pa_resum<2>(t2, p2, k == 0 ? b.nb_group : b.nb_node, words);
    const double bn = sqrt(t1[0]), rho = t2[0], rn = sqrt(t2[1]);
    if (k >= cg_max_iters || !(rn > cg_tol * bn)) {
        if (blockIdx.x == 0 && tid == 0) {
            b.st->stopped = 1;
            b.cg_iters[round] = k;
            b.cg_residual[round] = bn > 0.0 ? rn / bn : 0.0;
        }
        return;
    }
    const double beta = k > 0 ? rho / b.st->rho[(k - 1) & 1] : 0.0;
    if (blockIdx.x == 0 && tid == 0) b.st->rho[k & 1] = rho;
    const double *p_old = b.p[(k + 1) & 1], *zz = b.z;
    double *p_new = b.p[k & 1];
    const bool first = k == 0;
    const int32_t n = (int32_t)(((int64_t)blockIdx.x * RA_THREADS + tid) / G);
    const bool live = n < b.n_nodes && b.Dinv[n] != 0.0;
    // a node that is no unknown has z = p = 0: its new p is 0 too
    auto new_p = [&](int64_t m, double (&out)[3]) {
        for (int i = 0; i < 3; ++i) out[i] = first ? zz[3 * m + i] : zz[3 * m + i] + beta * p_old[3 * m + i];
    };
    double qs[3] = {0.0, 0.0, 0.0}, pn[3] = {0.0, 0.0, 0.0}, pq[1] = {0.0};
    if (live) {
        new_p(n, pn);
        const int64_t k1 = gr.adj_start[n + 1];
        for (int64_t e_k = gr.adj_start[n] + g; e_k < k1; e_k += G) {
            const int32_t code = gr.ent_code[e_k];
            const int64_t e = code >> 1;
            const double w = b.aw[e];
            if (w == 0.0) continue;
            double pb[3], y[3];
            new_p(gr.ent_nbr[e_k], pb);
            const double *A = gr.R_rel + 9 * e;
            if (code & 1) {  // the node is j: + w (p_j - R_rel p_i)
                rc_mul(A, pb, false, y);
                for (int i = 0; i < 3; ++i) qs[i] += w * (pn[i] - y[i]);
            } else {         // the node is i: - w R_rel^T (p_j - R_rel p_i)
                double u[3];
                rc_mul(A, pn, false, y);
                for (int i = 0; i < 3; ++i) u[i] = pb[i] - y[i];
                rc_mul(A, u, true, y);
                for (int i = 0; i < 3; ++i) qs[i] -= w * y[i];
            }
        }
    }
    pa_group_sum<3>(qs, G);
    if (g == 0 && live) {
        for (int i = 0; i < 3; ++i) {
            b.q[3 * (int64_t)n + i] = qs[i];
            p_new[3 * (int64_t)n + i] = pn[i];
        }
        pq[0] = pn[0] * qs[0] + pn[1] * qs[1] + pn[2] * qs[2];
    }
    pa_block_sum<1>(pq, words);
    if (tid == 0) b.part_pq[blockIdx.x] = pq[0];
}

// iteration k: alpha, x, r, z and the partials of r.z and |r|^2; a thread per node
__global__ __launch_bounds__(RA_THREADS) void k_rc_update(RcBufs b, int32_t round, int32_t k) {
    __shared__ double words[2 * (RA_THREADS / 64)];
    if (rc_halted(b.st)) return;
    const int tid = threadIdx.x;
    double pq[1];
    const double *const p1[1] = {b.part_pq};
    pa_resum<1>(pq, p1, b.nb_group, words);
    if (!(pq[0] > 0.0)) {
        // p has vanished to working precision (cg_tol = 0 and an r that underflowed): alpha would be 0 / 0.  The
        // solve ends here with its k iterations and x as it is; every workgroup draws this from the same sum.
        double bb[1], rr[1];
        const double *const p2[1] = {b.part_bb}, *const p3[1] = {b.part_rr};
        pa_resum<1>(bb, p2, b.nb_group, words);
        pa_resum<1>(rr, p3, k == 0 ? b.nb_group : b.nb_node, words);
        if (blockIdx.x == 0 && tid == 0) {
            b.st->stopped = 1;
            b.cg_iters[round] = k;
            b.cg_residual[round] = bb[0] > 0.0 ? sqrt(rr[0]) / sqrt(bb[0]) : 0.0;
        }
        return;
    }
    const double alpha = b.st->rho[k & 1] / pq[0];
    const double *p = b.p[k & 1];
    const int64_t n = (int64_t)blockIdx.x * RA_THREADS + tid;
    double t2[2] = {0.0, 0.0};
    if (n < b.n_nodes && b.Dinv[n] != 0.0) {
        const double dinv = b.Dinv[n];
        for (int i = 0; i < 3; ++i) {
            b.x[3 * n + i] += alpha * p[3 * n + i];
            const double r = b.r[3 * n + i] - alpha * b.q[3 * n + i], z = dinv * r;
            b.r[3 * n + i] = r;
            b.z[3 * n + i] = z;
            t2[0] += r * z;
            t2[1] += r * r;
        }
    }
    pa_block_sum<2>(t2, words);
    if (tid == 0) {
        b.part_rz[blockIdx.x] = t2[0];
        b.part_rr[blockIdx.x] = t2[1];
    }
}

// R_n <- exp(x_n) R_n for the unknowns, and the round's largest |x_n| as an integer maximum over the doubles' bits
__global__ __launch_bounds__(RA_THREADS) void k_rc_retract(RcBufs b, double *R, int32_t round) {
    const int64_t n = (int64_t)blockIdx.x * RA_THREADS + threadIdx.x;
    double step = 0.0;
    if (n < b.n_nodes && b.Dinv[n] != 0.0) {
        double Rn[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) Rn[j] = R[9 * n + j];
        const double o[3] = {b.x[3 * n], b.x[3 * n + 1], b.x[3 * n + 2]};
        step = ra_retract(o, Rn);
#pragma unroll
        for (int j = 0; j < 9; ++j) R[9 * n + j] = Rn[j];
    }
    unsigned long long bits = (unsigned long long)__double_as_longlong(step);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(bits >> 32), off, 64), lo = __shfl_xor((uint32_t)bits, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax(b.step_bits + round, bits);
}

}  // namespace sfm

using namespace sfm;

namespace {

// what the two entry points differ in: stage 3
struct RaRefit {
    bool cg;
    int32_t passes;  // the budget of stage 3: Jacobi sweeps (max_sweeps) or Gauss-Newton rounds (rounds)
    double tol;
    double cg_tol;
    int32_t cg_max_iters;
    int32_t *cg_iters;
    double *cg_residual, *step;  // `passes` long each
};

// stages 1 and 2, the refit that `rf` names, the edge pass and the groups: the one driver of both entry points
int ra_run(int32_t n_images, const int32_t *pair_ij, const double *R_rel, const double *weight, int64_t n_edges,
           uint64_t seed, double threshold, int32_t consensus_sweeps, const RaRefit &rf, double *R, double *edge_angle,
           uint8_t *edge_inlier, int32_t *n_inlier_edges, int32_t *group, int32_t *info, int32_t *level,
           int32_t *sweeps, int device) {
    const int32_t N = n_images, passes = rf.passes;
    const int64_t E = n_edges;
    const double tol = rf.tol;
    SFM_CHECK_ARG(N >= 0 && E >= 0, "n_images < 0 or n_edges < 0");
    SFM_CHECK_ARG(E <= (int64_t)1 << 30, "more than 2^30 edges");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0 && threshold < M_PI, "threshold must lie in (0, pi)");
    SFM_CHECK_ARG(consensus_sweeps >= 0 && passes >= 0,
                  rf.cg ? "consensus_sweeps < 0 or rounds < 0" : "consensus_sweeps < 0 or max_sweeps < 0");
    SFM_CHECK_ARG(tol >= 0.0, "tol must be >= 0");
    if (rf.cg) {
        SFM_CHECK_ARG(std::isfinite(rf.cg_tol) && rf.cg_tol >= 0.0, "cg_tol must be finite and >= 0");
        SFM_CHECK_ARG(rf.cg_max_iters >= 1, "cg_max_iters must be >= 1");
        SFM_CHECK_ARG(passes == 0 || (rf.cg_iters && rf.cg_residual && rf.step), "null pointer");
    }
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
    for (int32_t k = 0; rf.cg && k < passes; ++k) {
        rf.cg_iters[k] = 0;
        rf.cg_residual[k] = rf.step[k] = 0.0;
    }
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
    const auto w_max = work.add<unsigned long long>((size_t)passes + 1);  // per sweep, or per round
    const auto w_stop = work.add<int32_t>((size_t)passes + 1);
    const auto w_deep = work.add<int32_t>(1);
    // the CG refit: G lanes per node and the grids as position averaging's path 2 sizes them
    const int G = pa_group_lanes(2 * E, N, false);
    const int32_t nb_group = pa_blocks((int64_t)N * G, RA_THREADS), nb_node = pa_blocks(N, RA_THREADS);
    const size_t v3 = rf.cg ? 3 * (size_t)N : 0, npart = rf.cg ? (size_t)nb_group : 0;
    const auto w_aw = work.add<double>(rf.cg ? E : 0), w_g = work.add<double>(rf.cg ? 3 * E : 0);
    const auto w_x = work.add<double>(v3), w_r = work.add<double>(v3), w_z = work.add<double>(v3);
    const auto w_q = work.add<double>(v3), w_p0 = work.add<double>(v3), w_p1 = work.add<double>(v3);
    const auto w_D = work.add<double>(v3 / 3);
    const auto w_bb = work.add<double>(npart), w_rz = work.add<double>(npart), w_rr = work.add<double>(npart);
    const auto w_pq = work.add<double>(npart);
    const auto w_it = work.add<int32_t>(rf.cg ? passes : 0);
    const auto w_res = work.add<double>(rf.cg ? passes : 0);
    const auto w_state = work.add<RcState>(rf.cg ? 1 : 0);
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
    if (rf.cg) {
        if (passes > 0) {
            SFM_HIP(hipMemsetAsync(work.ptr(w_it), 0, w_it.bytes(), s));
            SFM_HIP(hipMemsetAsync(work.ptr(w_res), 0, w_res.bytes(), s));
        }
        SFM_HIP(hipMemsetAsync(work.ptr(w_state), 0, sizeof(RcState), s));
    }
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
    if (!rf.cg && !list[3].empty()) {
        const dim3 g_list((unsigned)ceil_div((int64_t)list[3].size(), RA_THREADS));
        std::vector<int32_t> stopped((size_t)passes + 1, 0);
        for (int32_t it = 0; it < passes;) {
            const int32_t it_end = std::min(it + RA_REFIT_BATCH, passes);
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
    // stage 3, the Gauss-Newton CG refit: per round the set-up, two launches per CG iteration with the stop word
    // looked at every RC_CG_BATCH iterations, the retraction; the round's step is read after it
    double cg_ms = 0.0;
    if (rf.cg && passes > 0) {
        const RcBufs b{in.ptr(i_ij), weight ? in.ptr(i_w) : (const double *)nullptr, out.ptr(o_level), work.ptr(w_aw),
                       work.ptr(w_g), work.ptr(w_x), work.ptr(w_r), work.ptr(w_z), work.ptr(w_q),
                       {work.ptr(w_p0), work.ptr(w_p1)}, work.ptr(w_D), work.ptr(w_bb), work.ptr(w_rz),
                       work.ptr(w_rr), work.ptr(w_pq), work.ptr(w_state), work.ptr(w_it), work.ptr(w_res),
                       work.ptr(w_max), N, G, E, nb_group, nb_node};
        const dim3 g_group((unsigned)nb_group), g_edge((unsigned)ceil_div(E, RA_THREADS));
        for (int32_t round = 0; round < passes; ++round) {
            hipLaunchKernelGGL(k_rc_edges, g_edge, T, 0, s, b, in.ptr(i_rel), buf[cur], tau);
            hipLaunchKernelGGL(k_rc_gather, g_group, T, 0, s, g, b);
            SFM_HIP(hipGetLastError());
            RcState st{};
            // iteration cg_max_iters is the apply launch alone: it ends the solve if nothing did before
            // (k is 64 bits wide on the host: cg_max_iters + 1 must not wrap at INT32_MAX)
            for (int64_t k = 0; k <= rf.cg_max_iters && !st.stopped;) {
                const int64_t k_end = std::min<int64_t>(k + RC_CG_BATCH, (int64_t)rf.cg_max_iters + 1);
                if (timed) SFM_HIP(hipEventRecord(c->ev[5], s));
                for (; k < k_end; ++k) {
                    hipLaunchKernelGGL(k_rc_apply, g_group, T, 0, s, g, b, rf.cg_tol, rf.cg_max_iters, round, (int32_t)k);
                    if (k < rf.cg_max_iters) hipLaunchKernelGGL(k_rc_update, g_nodes, T, 0, s, b, round, (int32_t)k);
                    SFM_HIP(hipGetLastError());
                }
                if (timed) SFM_HIP(hipEventRecord(c->ev[6], s));
                SFM_TRY(work.download(&st, w_state, s));
                SFM_HIP(hipStreamSynchronize(s));
                if (timed) {
                    float t = 0;
                    (void)hipEventElapsedTime(&t, c->ev[5], c->ev[6]);
                    cg_ms += t;
                }
            }
            hipLaunchKernelGGL(k_rc_retract, g_nodes, T, 0, s, b, buf[cur], round);
            SFM_HIP(hipGetLastError());
            unsigned long long bits = 0;
            SFM_TRY(work.download(&bits, w_max, (size_t)round, 1, s));
            SFM_HIP(hipStreamSynchronize(s));
            std::memcpy(&rf.step[round], &bits, sizeof(double));
            ++n_run;
            if (tol > 0.0 && rf.step[round] <= tol) break;
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
    if (rf.cg && passes > 0) {
        SFM_TRY(work.download(rf.cg_iters, w_it, s));
        SFM_TRY(work.download(rf.cg_residual, w_res, s));
    }
    SFM_TRY(tm.finish(s));
    if (timed) {  // [3]: the consensus kernels alone, or the CG launches alone
        float t[4] = {0, 0, 0, 0};
        for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&t[k], c->ev[k], c->ev[k + 1]);
        if (!rf.cg) (void)hipEventElapsedTime(&t[3], c->ev[5], c->ev[6]);
        const double t4[4] = {t[0], t[1], t[2], rf.cg ? cg_ms : t[3]};
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

}  // namespace

extern "C" int sfm_average_rotations(int32_t n_images, const int32_t *pair_ij, const double *R_rel,
                                     const double *weight, int64_t n_edges, uint64_t seed, double threshold,
                                     int32_t consensus_sweeps, int32_t max_sweeps, double tol, double *R,
                                     double *edge_angle, uint8_t *edge_inlier, int32_t *n_inlier_edges, int32_t *group,
                                     int32_t *info, int32_t *level, int32_t *sweeps, int device) {
    const RaRefit rf{false, max_sweeps, tol, 0.0, 0, nullptr, nullptr, nullptr};
    return ra_run(n_images, pair_ij, R_rel, weight, n_edges, seed, threshold, consensus_sweeps, rf, R, edge_angle,
                  edge_inlier, n_inlier_edges, group, info, level, sweeps, device);
}

extern "C" int sfm_average_rotations_cg(int32_t n_images, const int32_t *pair_ij, const double *R_rel,
                                        const double *weight, int64_t n_edges, uint64_t seed, double threshold,
                                        int32_t consensus_sweeps, int32_t rounds, double tol, double cg_tol,
                                        int32_t cg_max_iters, double *R, double *edge_angle, uint8_t *edge_inlier,
                                        int32_t *n_inlier_edges, int32_t *group, int32_t *info, int32_t *level,
                                        int32_t *sweeps, int32_t *cg_iters, double *cg_residual, double *step,
                                        int device) {
    const RaRefit rf{true, rounds, tol, cg_tol, cg_max_iters, cg_iters, cg_residual, step};
    return ra_run(n_images, pair_ij, R_rel, weight, n_edges, seed, threshold, consensus_sweeps, rf, R, edge_angle,
                  edge_inlier, n_inlier_edges, group, info, level, sweeps, device);
}
