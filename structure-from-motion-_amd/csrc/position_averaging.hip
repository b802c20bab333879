// Global position averaging: every camera's centre from the world-frame
// directions of the verified pairs, in one call (sfm_average_positions; the
// definitions are in include/sfmcore.h).  The reference has no counterpart.
//
// Host: argument checks, the CSR adjacency, leaf pruning, components by
// union-find, the largest one renumbered to local nodes and edges, the root.
//
// A round is one preconditioned conjugate-gradient solve of a 3 (M - 1) system
// applied matrix-free from the adjacency, the normalisation by c and the new
// edge weights and target lengths.  A node's entries are walked by a group of
// G lanes (G a power of two <= 64 chosen on the host from the size of the
// graph, position_plan.hpp): lane g takes the entries g, g + G, .. in their order and the group's
// partial sums meet in a shuffle tree, so a node of any degree is a loop, never
// a lane per entry.  Every sum over nodes or edges (the two CG dot products,
// |r|, |rhs|, the two sums of c) is a per-thread sum in index order, a shuffle
// tree over the wave, one word per wave and the words added in wave order: no
// float atomic, the same bits on every run of one path.
//
//   path 1  k_pa_persistent: one workgroup of 512 threads, one launch for all
//           rounds.  x, r, p, z, q and the six entries of every D^-1 live in
//           LDS (168 bytes a node, dynamic LDS: PA_MAX_NODES = 512 nodes are
//           86,208 bytes with the wave words); the edge records (direction,
//           weight, target, neighbour) stream from global memory in every
//           iteration.  Reweighting and normalisation run between the solves of
//           the same launch; w and s are written to global memory and read back
//           behind a workgroup barrier.
//   path 2  any size, 256-thread workgroups, no grid-wide barrier: per round
//           k_pa_setup, then two launches per CG iteration -- k_pa_apply (every
//           workgroup re-sums the partials of the launch before in their order,
//           tests the stop, forms p = z + beta p_old for its nodes and, on the
//           fly, for their neighbours, applies the operator and leaves partials
//           of p.q) and k_pa_update (alpha from the partials; x, r, z; partials
//           of r.z and |r|^2) -- then k_pa_proj, k_pa_normalise, k_pa_reweight.
//           The stop lives in a device word; launches past it return at once
//           and the host looks every PA_CG_BATCH iterations.
//
// The two paths add in different orders and agree to tolerance, not bitwise.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fixed_sums.hpp"
#include "position_plan.hpp"
#include "staging.hpp"
#include "view_graph.hpp"

namespace sfm {

static_assert(PA_MAX_NODES == SFM_POSITIONS_PATH1_MAX_NODES, "position_plan.hpp and sfmcore.h name one bound");
constexpr int PA_CG_BATCH = 8;   // path 2: CG iterations launched between two looks at the stop word
constexpr double PA_FLOOR = 1e-3;  // the least target length and the least |v| of a weight

struct PaGraph {
    const int64_t *adj_start;  // M + 1
    const int32_t *ent_code;   // 2 e + (0: the node is the edge's i, 1: its j)
    const int32_t *ent_nbr;
    const int32_t *ij;         // E x 2, local nodes
    const double *dir;         // E x 3, unit
    const double *weight;      // E, the caller's (ones where it gave none)
    double *w, *s;             // E: the round's weights and target lengths
    int32_t n_nodes, root;
    int32_t n_edges;
    int32_t G;                 // lanes per node
};

struct PaParams {
    double mu, sigma, threshold, cg_tol;
    int32_t rounds, cg_max_iters;
};

struct PaEdgeOut {
    double *angle, *length;
    uint8_t *inlier;
};

// path 2's words that cross launches
struct PaState {
    double rho[2];  // r.z of iteration k in slot k & 1
    int32_t stopped, error;
};

// path 2: has an error or (where asked) the stop ended this launch's work?  One read per workgroup, so that all its
// waves agree.  A word set during this very launch was set by a workgroup that drew, from the same sums, the
// conclusion that a workgroup reading 0 draws itself a few lines later.
__device__ __forceinline__ bool pa_halted(const PaState *st, bool test_stopped) {
    __shared__ int32_t halt;
    if (threadIdx.x == 0) halt = st->error | (test_stopped ? st->stopped : 0);
    __syncthreads();
    return halt != 0;
}

// lane g's share of q_n = sum over n's entries of w (u - (1 - mu) d (d.u)), u = pn - p_nbr;
// nbr_p(nbr, out) gives the neighbour's p
template <class F>
__device__ __forceinline__ void pa_apply_share(const PaGraph &gr, int32_t n, int g, double mu1, const double (&pn)[3],
                                               F nbr_p, double (&q)[3]) {
    q[0] = q[1] = q[2] = 0.0;
    const int64_t k1 = gr.adj_start[n + 1];
    for (int64_t k = gr.adj_start[n] + g; k < k1; k += gr.G) {
        const int32_t e = gr.ent_code[k] >> 1;
        const double w = gr.w[e];
        const double d0 = gr.dir[3 * (int64_t)e], d1 = gr.dir[3 * (int64_t)e + 1], d2 = gr.dir[3 * (int64_t)e + 2];
        double pb[3];
        nbr_p(gr.ent_nbr[k], pb);
        const double u0 = pn[0] - pb[0], u1 = pn[1] - pb[1], u2 = pn[2] - pb[2];
        const double t = mu1 * (d0 * u0 + d1 * u1 + d2 * u2);
        q[0] += w * (u0 - t * d0);
        q[1] += w * (u1 - t * d1);
        q[2] += w * (u2 - t * d2);
    }
}

// lane g's share of a node's set-up sums: a[0..6) the entries xx xy xz yy yz zz of D_n,
// a[6..9) the right-hand side, a[9..12) (A x)_n
__device__ __forceinline__ void pa_setup_share(const PaGraph &gr, int32_t n, int g, double mu, const double *x,
                                               double (&a)[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = 0.0;
    const double mu1 = 1.0 - mu;
    const double x0 = x[3 * (int64_t)n], x1 = x[3 * (int64_t)n + 1], x2 = x[3 * (int64_t)n + 2];
    const int64_t k1 = gr.adj_start[n + 1];
    for (int64_t k = gr.adj_start[n] + g; k < k1; k += gr.G) {
        const int32_t code = gr.ent_code[k], e = code >> 1;
        const int64_t nb = gr.ent_nbr[k];
        const double w = gr.w[e];
        const double d0 = gr.dir[3 * (int64_t)e], d1 = gr.dir[3 * (int64_t)e + 1], d2 = gr.dir[3 * (int64_t)e + 2];
        a[0] += w * (1.0 - mu1 * d0 * d0);
        a[1] -= w * (mu1 * d0 * d1);
        a[2] -= w * (mu1 * d0 * d2);
        a[3] += w * (1.0 - mu1 * d1 * d1);
        a[4] -= w * (mu1 * d1 * d2);
        a[5] += w * (1.0 - mu1 * d2 * d2);
        const double b = (code & 1 ? mu : -mu) * w * gr.s[e];  // the node is the edge's j: + mu w s d
        a[6] += b * d0;
        a[7] += b * d1;
        a[8] += b * d2;
        const double u0 = x0 - x[3 * nb], u1 = x1 - x[3 * nb + 1], u2 = x2 - x[3 * nb + 2];
        const double t = mu1 * (d0 * u0 + d1 * u1 + d2 * u2);
        a[9] += w * (u0 - t * d0);
        a[10] += w * (u1 - t * d1);
        a[11] += w * (u2 - t * d2);
    }
}

// the inverse of the symmetric D (xx xy xz yy yz zz) by cofactors, in the same layout
__device__ __forceinline__ void pa_invert(const double *D, double *inv) {
    const double a = D[0], b = D[1], c = D[2], d = D[3], e = D[4], f = D[5];
    const double A = d * f - e * e, B = c * e - b * f, C = b * e - c * d;
    const double det = a * A + b * B + c * C;
    inv[0] = A / det;
    inv[1] = B / det;
    inv[2] = C / det;
    inv[3] = (a * f - c * c) / det;
    inv[4] = (b * c - a * e) / det;
    inv[5] = (a * d - b * b) / det;
}

__device__ __forceinline__ void pa_sym_mul(const double *S, const double *v, double *out) {
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    out[0] = S[0] * v0 + S[1] * v1 + S[2] * v2;
    out[1] = S[1] * v0 + S[3] * v1 + S[4] * v2;
    out[2] = S[2] * v0 + S[4] * v1 + S[5] * v2;
}

// the set-up of node n from the group's sums: D^-1, r = rhs - A x, z = D^-1 r; returns |rhs|^2, r.z, |r|^2 in t
__device__ __forceinline__ void pa_setup_node(const double (&a)[12], double *Dinv, double *r, double *z, double (&t)[3]) {
    pa_invert(a, Dinv);
    r[0] = a[6] - a[9];
    r[1] = a[7] - a[10];
    r[2] = a[8] - a[11];
    pa_sym_mul(Dinv, r, z);
    t[0] += a[6] * a[6] + a[7] * a[7] + a[8] * a[8];
    t[1] += r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
    t[2] += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}

// d_e . (x_j - x_i)
__device__ __forceinline__ double pa_proj(const PaGraph &gr, int32_t e, const double *x) {
    const int64_t i = gr.ij[2 * (int64_t)e], j = gr.ij[2 * (int64_t)e + 1];
    const double *d = gr.dir + 3 * (int64_t)e;
    return d[0] * (x[3 * j] - x[3 * i]) + d[1] * (x[3 * j + 1] - x[3 * i + 1]) + d[2] * (x[3 * j + 2] - x[3 * i + 2]);
}

// the edge's angle and length on the normalised x, and its next weight and target
__device__ __forceinline__ void pa_reweight_edge(const PaGraph &gr, const PaParams &pr, const PaEdgeOut &eo, int32_t e,
                                                 const double *x) {
    const int64_t i = gr.ij[2 * (int64_t)e], j = gr.ij[2 * (int64_t)e + 1];
    const double *d = gr.dir + 3 * (int64_t)e;
    const double v0 = x[3 * j] - x[3 * i], v1 = x[3 * j + 1] - x[3 * i + 1], v2 = x[3 * j + 2] - x[3 * i + 2];
    const double proj = d[0] * v0 + d[1] * v1 + d[2] * v2;
    const double c0 = d[1] * v2 - d[2] * v1, c1 = d[2] * v0 - d[0] * v2, c2 = d[0] * v1 - d[1] * v0;
    const double theta = atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), proj);
    const double len = fmax(sqrt(v0 * v0 + v1 * v1 + v2 * v2), PA_FLOOR);
    const double ts = theta / pr.sigma;
    gr.s[e] = fmax(proj, PA_FLOOR);
    gr.w[e] = gr.weight[e] / ((1.0 + ts * ts) * (len * len));
    eo.angle[e] = theta;
    eo.length[e] = proj;
    eo.inlier[e] = theta <= pr.threshold ? 1 : 0;
}

// ------------------------------------------------------------------ path 1
__global__ __launch_bounds__(PA_T1) void k_pa_persistent(PaGraph gr, PaParams pr, PaEdgeOut eo, double *C,
                                                         int32_t *cg_iters, double *cg_residual, int32_t *error,
                                                         long long *cg_ticks) {
    extern __shared__ __attribute__((aligned(16))) char pa_smem[];
    const int tid = threadIdx.x, M = gr.n_nodes, G = gr.G, E = gr.n_edges;
    double *x = reinterpret_cast<double *>(pa_smem), *r = x + 3 * M, *p = r + 3 * M, *z = p + 3 * M, *q = z + 3 * M;
    double *Dinv = q + 3 * M, *words = Dinv + 6 * M;  // 3 * (PA_T1 / 64) words
    const int per_pass = PA_T1 / G, n_pass = (M + per_pass - 1) / per_pass, g = tid & (G - 1);
    const double mu1 = 1.0 - pr.mu;
    long long ticks = 0;

    for (int k = tid; k < 3 * M; k += PA_T1) x[k] = 0.0;
    __syncthreads();
    for (int32_t round = 0; round < pr.rounds; ++round) {
        // set-up: D^-1, r = rhs - A x, z, p
        double t3[3] = {0.0, 0.0, 0.0};
        for (int pass = 0; pass < n_pass; ++pass) {
            const int32_t n = pass * per_pass + tid / G;
            const bool live = n < M && n != gr.root;
            double a[12];
            if (live) {
                pa_setup_share(gr, n, g, pr.mu, x, a);
            } else {
#pragma unroll
                for (int i = 0; i < 12; ++i) a[i] = 0.0;
            }
            pa_group_sum<12>(a, G);
            if (g == 0 && n < M) {
                if (live) {
                    pa_setup_node(a, Dinv + 6 * n, r + 3 * n, z + 3 * n, t3);
                    for (int i = 0; i < 3; ++i) p[3 * n + i] = z[3 * n + i];
                } else {
                    for (int i = 0; i < 3; ++i) r[3 * n + i] = z[3 * n + i] = p[3 * n + i] = q[3 * n + i] = 0.0;
                    for (int i = 0; i < 6; ++i) Dinv[6 * n + i] = 0.0;
                }
            }
        }
        pa_block_sum<3>(t3, words);
        const double bn = sqrt(t3[0]);
        double rho = t3[1], rn = sqrt(t3[2]);
        int32_t k = 0;
        const long long t_start = wall_clock64();
        while (k < pr.cg_max_iters && rn > pr.cg_tol * bn) {
            double pq[1] = {0.0};
            for (int pass = 0; pass < n_pass; ++pass) {
                const int32_t n = pass * per_pass + tid / G;
                const bool live = n < M && n != gr.root;
                double qs[3] = {0.0, 0.0, 0.0}, pn[3] = {0.0, 0.0, 0.0};
                if (live) {
                    for (int i = 0; i < 3; ++i) pn[i] = p[3 * n + i];
                    pa_apply_share(gr, n, g, mu1, pn,
                                   [&](int32_t nb, double (&pb)[3]) {
                                       for (int i = 0; i < 3; ++i) pb[i] = p[3 * nb + i];
                                   },
                                   qs);
                }
                pa_group_sum<3>(qs, G);
                if (g == 0 && live) {
                    for (int i = 0; i < 3; ++i) q[3 * n + i] = qs[i];
                    pq[0] += pn[0] * qs[0] + pn[1] * qs[1] + pn[2] * qs[2];
                }
            }
            pa_block_sum<1>(pq, words);
            const double alpha = rho / pq[0];
            double t2[2] = {0.0, 0.0};
            for (int32_t n = tid; n < M; n += PA_T1) {
                if (n == gr.root) continue;
                for (int i = 0; i < 3; ++i) {
                    x[3 * n + i] += alpha * p[3 * n + i];
                    r[3 * n + i] -= alpha * q[3 * n + i];
                }
                pa_sym_mul(Dinv + 6 * n, r + 3 * n, z + 3 * n);
                t2[0] += r[3 * n] * z[3 * n] + r[3 * n + 1] * z[3 * n + 1] + r[3 * n + 2] * z[3 * n + 2];
                t2[1] += r[3 * n] * r[3 * n] + r[3 * n + 1] * r[3 * n + 1] + r[3 * n + 2] * r[3 * n + 2];
            }
            pa_block_sum<2>(t2, words);
            const double beta = t2[0] / rho;
            rho = t2[0];
            rn = sqrt(t2[1]);
            for (int32_t n = tid; n < M; n += PA_T1)
                for (int i = 0; i < 3; ++i) p[3 * n + i] = z[3 * n + i] + beta * p[3 * n + i];
            __syncthreads();
            ++k;
        }
        ticks += wall_clock64() - t_start;
        if (tid == 0) {
            cg_iters[round] = k;
            cg_residual[round] = bn > 0.0 ? rn / bn : 0.0;
        }
        // c = sum w (d.v) / sum w, on the round's weights
        double cs[2] = {0.0, 0.0};
        for (int32_t e = tid; e < E; e += PA_T1) {
            const double w = gr.w[e];
            cs[0] += w * pa_proj(gr, e, x);
            cs[1] += w;
        }
        pa_block_sum<2>(cs, words);
        const double c = cs[0] / cs[1];
        if (!(c > 0.0) || isinf(c)) {  // the same value in every thread
            if (tid == 0) *error = 1;
            return;
        }
        for (int k3 = tid; k3 < 3 * M; k3 += PA_T1) x[k3] = x[k3] / c;
        __syncthreads();
        for (int32_t e = tid; e < E; e += PA_T1) pa_reweight_edge(gr, pr, eo, e, x);
        __syncthreads();  // w and s: global stores of this workgroup, read by it after the barrier
    }
    for (int k = tid; k < 3 * M; k += PA_T1) C[k] = x[k];
    if (tid == 0) *cg_ticks = ticks;
}

// ------------------------------------------------------------------ path 2
struct PaBufs {
    double *x, *r, *z, *q, *p[2], *Dinv;
    double *part_bb, *part_rz, *part_rr, *part_pq, *part_a, *part_b;
    PaState *st;
    int32_t *cg_iters;
    double *cg_residual;
    int32_t nb_group, nb_node, nb_edge;  // the grids: groups of G lanes per node, a thread per node, a thread per edge
};

__global__ __launch_bounds__(PA_T2) void k_pa_setup(PaGraph gr, PaParams pr, PaBufs b) {
    __shared__ double words[3 * (PA_T2 / 64)];
    if (pa_halted(b.st, false)) return;
    const int tid = threadIdx.x, G = gr.G, g = tid & (G - 1);
    const int32_t n = (int32_t)(((int64_t)blockIdx.x * PA_T2 + tid) / G);
    const bool live = n < gr.n_nodes && n != gr.root;
    double a[12], t3[3] = {0.0, 0.0, 0.0};
    if (live) {
        pa_setup_share(gr, n, g, pr.mu, b.x, a);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) a[i] = 0.0;
    }
    pa_group_sum<12>(a, G);
    if (g == 0 && n < gr.n_nodes) {
        if (live) {
            pa_setup_node(a, b.Dinv + 6 * (int64_t)n, b.r + 3 * (int64_t)n, b.z + 3 * (int64_t)n, t3);
        } else {
            for (int i = 0; i < 3; ++i) b.r[3 * n + i] = b.z[3 * n + i] = b.q[3 * n + i] = b.p[0][3 * n + i] = b.p[1][3 * n + i] = 0.0;
            for (int i = 0; i < 6; ++i) b.Dinv[6 * n + i] = 0.0;
        }
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
__global__ __launch_bounds__(PA_T2) void k_pa_apply(PaGraph gr, PaParams pr, PaBufs b, int32_t round, int32_t k) {
    __shared__ double words[3 * (PA_T2 / 64)];
    if (pa_halted(b.st, true)) return;
    const int tid = threadIdx.x, G = gr.G, g = tid & (G - 1);
    // |rhs|^2 from the set-up's grid; r.z and |r|^2 from it at k = 0, then from k_pa_update's
    double t1[1], t2[2];
    const double *const p1[1] = {b.part_bb};
    const double *const p2[2] = {b.part_rz, b.part_rr};
    pa_resum<1>(t1, p1, b.nb_group, words);
    pa_resum<2>(t2, p2, k == 0 ? b.nb_group : b.nb_node, words);
    const double bn = sqrt(t1[0]), rho = t2[0], rn = sqrt(t2[1]);
    if (k >= pr.cg_max_iters || !(rn > pr.cg_tol * bn)) {
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
    const int32_t n = (int32_t)(((int64_t)blockIdx.x * PA_T2 + tid) / G);
    const bool live = n < gr.n_nodes && n != gr.root;
    auto new_p = [&](int32_t m, double (&out)[3]) {
        for (int i = 0; i < 3; ++i)
            out[i] = first ? zz[3 * (int64_t)m + i] : zz[3 * (int64_t)m + i] + beta * p_old[3 * (int64_t)m + i];
    };
    double qs[3] = {0.0, 0.0, 0.0}, pn[3] = {0.0, 0.0, 0.0}, pq[1] = {0.0};
    if (live) {
        new_p(n, pn);
        pa_apply_share(gr, n, g, 1.0 - pr.mu, pn, new_p, qs);
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
__global__ __launch_bounds__(PA_T2) void k_pa_update(PaGraph gr, PaBufs b, int32_t k) {
    __shared__ double words[2 * (PA_T2 / 64)];
    if (pa_halted(b.st, true)) return;
    const int tid = threadIdx.x;
    double pq[1];
    const double *const p1[1] = {b.part_pq};
    pa_resum<1>(pq, p1, b.nb_group, words);
    const double alpha = b.st->rho[k & 1] / pq[0];
    const double *p = b.p[k & 1];
    const int64_t n = (int64_t)blockIdx.x * PA_T2 + tid;
    double t2[2] = {0.0, 0.0};
    if (n < gr.n_nodes && n != gr.root) {
        double r[3], z[3];
        for (int i = 0; i < 3; ++i) {
            b.x[3 * n + i] += alpha * p[3 * n + i];
            r[i] = b.r[3 * n + i] - alpha * b.q[3 * n + i];
            b.r[3 * n + i] = r[i];
        }
        pa_sym_mul(b.Dinv + 6 * n, r, z);
        for (int i = 0; i < 3; ++i) b.z[3 * n + i] = z[i];
        t2[0] = r[0] * z[0] + r[1] * z[1] + r[2] * z[2];
        t2[1] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    }
    pa_block_sum<2>(t2, words);
    if (tid == 0) {
        b.part_rz[blockIdx.x] = t2[0];
        b.part_rr[blockIdx.x] = t2[1];
    }
}

__global__ __launch_bounds__(PA_T2) void k_pa_proj(PaGraph gr, PaBufs b) {
    __shared__ double words[2 * (PA_T2 / 64)];
    if (pa_halted(b.st, false)) return;
    const int64_t e = (int64_t)blockIdx.x * PA_T2 + threadIdx.x;
    double cs[2] = {0.0, 0.0};
    if (e < gr.n_edges) {
        const double w = gr.w[e];
        cs[0] = w * pa_proj(gr, (int32_t)e, b.x);
        cs[1] = w;
    }
    pa_block_sum<2>(cs, words);
    if (threadIdx.x == 0) {
        b.part_a[blockIdx.x] = cs[0];
        b.part_b[blockIdx.x] = cs[1];
    }
}

__global__ __launch_bounds__(PA_T2) void k_pa_normalise(PaGraph gr, PaBufs b) {
    __shared__ double words[2 * (PA_T2 / 64)];
    if (pa_halted(b.st, false)) return;
    double cs[2];
    const double *const p2[2] = {b.part_a, b.part_b};
    pa_resum<2>(cs, p2, b.nb_edge, words);
    const double c = cs[0] / cs[1];
    if (!(c > 0.0) || isinf(c)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) b.st->error = 1;
        return;
    }
    const int64_t n = (int64_t)blockIdx.x * PA_T2 + threadIdx.x;
    if (n < gr.n_nodes)
        for (int i = 0; i < 3; ++i) b.x[3 * n + i] = b.x[3 * n + i] / c;
}

__global__ __launch_bounds__(PA_T2) void k_pa_reweight(PaGraph gr, PaParams pr, PaEdgeOut eo, PaBufs b) {
    if (pa_halted(b.st, false)) return;
    const int64_t e = (int64_t)blockIdx.x * PA_T2 + threadIdx.x;
    if (e < gr.n_edges) pa_reweight_edge(gr, pr, eo, (int32_t)e, b.x);
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_average_positions(int32_t n_images, const int32_t *pair_ij, const double *dir, const double *weight,
                                     int64_t n_edges, double mu, double sigma, double threshold, int32_t rounds,
                                     double cg_tol, int32_t cg_max_iters, int32_t path, double *C, double *edge_angle,
                                     uint8_t *edge_inlier, double *edge_length, int32_t *info, int32_t *cg_iters,
                                     double *cg_residual, int32_t *n_solved, int32_t *path_used, int device) {
    const int32_t N = n_images;
    const int64_t E = n_edges;
    SFM_CHECK_ARG(N >= 0 && E >= 0, "n_images < 0 or n_edges < 0");
    SFM_CHECK_ARG(E <= (int64_t)1 << 30, "more than 2^30 edges");
    SFM_CHECK_ARG(mu > 0.0 && mu <= 1.0, "mu must lie in (0, 1]");
    SFM_CHECK_ARG(std::isfinite(sigma) && sigma > 0.0, "sigma must be finite and > 0");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0 && threshold < M_PI, "threshold must lie in (0, pi)");
    SFM_CHECK_ARG(rounds >= 1, "rounds must be >= 1");
    SFM_CHECK_ARG(std::isfinite(cg_tol) && cg_tol >= 0.0, "cg_tol must be finite and >= 0");
    SFM_CHECK_ARG(cg_max_iters >= 1, "cg_max_iters must be >= 1");
    SFM_CHECK_ARG(path >= 0 && path <= 2, "path must be 0, 1 or 2");
    SFM_CHECK_ARG(E == 0 || (pair_ij && dir), "null pointer");
    SFM_CHECK_ARG(cg_iters && cg_residual && n_solved && path_used && (N == 0 || (C && info)) &&
                      (E == 0 || (edge_angle && edge_inlier && edge_length)),
                  "null pointer");
    std::vector<double> unit((size_t)(3 * E));
    for (int64_t e = 0; e < E; ++e) {
        const int32_t i = pair_ij[2 * e], j = pair_ij[2 * e + 1];
        SFM_CHECK_ARG(i >= 0 && i < N && j >= 0 && j < N, "a pair image outside [0, n_images)");
        SFM_CHECK_ARG(i != j, "a pair of an image with itself");
        const double *d = dir + 3 * e;
        SFM_CHECK_ARG(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]), "a direction is not finite");
        // scaled by the largest component first, so that no finite direction overflows or vanishes
        const double m = std::max(std::fabs(d[0]), std::max(std::fabs(d[1]), std::fabs(d[2])));
        SFM_CHECK_ARG(m > 0.0, "a direction is zero");
        const double a = d[0] / m, b = d[1] / m, c = d[2] / m, len = std::sqrt(a * a + b * b + c * c);
        unit[3 * e] = a / len;
        unit[3 * e + 1] = b / len;
        unit[3 * e + 2] = c / len;
        SFM_CHECK_ARG(!weight || (std::isfinite(weight[e]) && weight[e] > 0.0), "a weight is not finite and positive");
    }

    // the graph to solve: adjacency, leaf pruning, the largest component, its root
    std::vector<int32_t> solved;             // the solved nodes, ascending
    std::vector<int32_t> local((size_t)N, -1);
    std::vector<int64_t> edges;              // the edges between solved nodes, ascending
    int32_t root = -1;
    if (N > 0 && E > 0) {
        std::vector<int64_t> adj_start;
        std::vector<int32_t> ent_code, ent_nbr;
        build_adjacency(N, pair_ij, E, adj_start, ent_code, ent_nbr);
        // distinct neighbours; a node with fewer than two goes, which may expose the next
        std::vector<int32_t> stamp((size_t)N, -1), distinct((size_t)N, 0), queue;
        std::vector<uint8_t> alive((size_t)N, 1);
        for (int32_t n = 0; n < N; ++n) {
            for (int64_t k = adj_start[n]; k < adj_start[(size_t)n + 1]; ++k)
                if (stamp[ent_nbr[k]] != n) {
                    stamp[ent_nbr[k]] = n;
                    ++distinct[n];
                }
            if (distinct[n] < 2) {
                alive[n] = 0;
                queue.push_back(n);
            }
        }
        std::fill(stamp.begin(), stamp.end(), -1);
        for (size_t h = 0; h < queue.size(); ++h) {
            const int32_t n = queue[h];
            for (int64_t k = adj_start[n]; k < adj_start[(size_t)n + 1]; ++k) {
                const int32_t m = ent_nbr[k];
                if (!alive[m] || stamp[m] == n) continue;
                stamp[m] = n;
                if (--distinct[m] < 2) {
                    alive[m] = 0;
                    queue.push_back(m);
                }
            }
        }
        NodeSets sets(N);
        for (int64_t e = 0; e < E; ++e)
            if (alive[pair_ij[2 * e]] && alive[pair_ij[2 * e + 1]]) sets.join(pair_ij[2 * e], pair_ij[2 * e + 1]);
        std::vector<int32_t> size((size_t)N, 0);
        int32_t best = -1;
        for (int32_t n = 0; n < N; ++n)
            if (alive[n]) ++size[sets.find(n)];
        for (int32_t n = 0; n < N; ++n)  // the largest, the lowest label on ties
            if (size[n] > 0 && (best < 0 || size[n] > size[best])) best = n;
        if (best >= 0) {
            for (int32_t n = 0; n < N; ++n)
                if (alive[n] && sets.find(n) == best) {
                    local[n] = (int32_t)solved.size();
                    solved.push_back(n);
                }
            for (int64_t e = 0; e < E; ++e)
                if (local[pair_ij[2 * e]] >= 0 && local[pair_ij[2 * e + 1]] >= 0) edges.push_back(e);
        }
    }
    const int32_t M = (int32_t)solved.size();
    const int64_t El = (int64_t)edges.size();
    const PaPlan plan = pa_plan(M, El, path);  // position_plan.hpp
    const int use_path = plan.path;
    SFM_CHECK_ARG(plan.fits, "path 1 takes at most 512 solved nodes");

    // from here on the outputs are written
    for (int32_t n = 0; n < N; ++n) {
        C[3 * (size_t)n] = C[3 * (size_t)n + 1] = C[3 * (size_t)n + 2] = 0.0;
        info[n] = -1;
    }
    for (int64_t e = 0; e < E; ++e) {
        edge_angle[e] = edge_length[e] = 0.0;
        edge_inlier[e] = 0;
    }
    for (int32_t k = 0; k < rounds; ++k) {
        cg_iters[k] = 0;
        cg_residual[k] = 0.0;
    }
    *n_solved = M;
    *path_used = use_path;
    if (M == 0) return 0;

    // the local graph; the root: most entries, the lowest node on ties
    std::vector<int32_t> l_ij((size_t)(2 * El));
    std::vector<double> l_dir((size_t)(3 * El)), l_w((size_t)El), l_s((size_t)El, 1.0);
    for (int64_t k = 0; k < El; ++k) {
        const int64_t e = edges[k];
        l_ij[2 * k] = local[pair_ij[2 * e]];
        l_ij[2 * k + 1] = local[pair_ij[2 * e + 1]];
        for (int t = 0; t < 3; ++t) l_dir[3 * k + t] = unit[3 * e + t];
        l_w[k] = weight ? weight[e] : 1.0;
    }
    std::vector<int64_t> adj_start;
    std::vector<int32_t> ent_code, ent_nbr;
    build_adjacency(M, l_ij.data(), El, adj_start, ent_code, ent_nbr);
    root = 0;
    for (int32_t n = 1; n < M; ++n)
        if (adj_start[(size_t)n + 1] - adj_start[n] > adj_start[(size_t)root + 1] - adj_start[root]) root = n;
    const int G = plan.G;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_adj = in.add<int64_t>((size_t)M + 1);
    const auto i_code = in.add<int32_t>(2 * El), i_nbr = in.add<int32_t>(2 * El), i_ij = in.add<int32_t>(2 * El);
    const auto i_dir = in.add<double>(3 * El), i_weight = in.add<double>(El);
    const auto o_C = out.add<double>(3 * (size_t)M), o_ang = out.add<double>(El), o_len = out.add<double>(El);
    const auto o_inl = out.add<uint8_t>(El);
    const auto o_it = out.add<int32_t>(rounds), o_err = out.add<int32_t>(1);
    const auto o_res = out.add<double>(rounds);
    const auto o_ticks = out.add<long long>(1);
    const auto o_state = out.add<PaState>(1);
    const auto w_w = work.add<double>(El), w_s = work.add<double>(El);
    const int32_t nb_group = plan.nb_group, nb_node = plan.nb_node, nb_edge = plan.nb_edge;
    const size_t v3 = use_path == 2 ? 3 * (size_t)M : 0;
    const auto w_r = work.add<double>(v3), w_z = work.add<double>(v3), w_q = work.add<double>(v3);
    const auto w_p0 = work.add<double>(v3), w_p1 = work.add<double>(v3), w_D = work.add<double>(2 * v3);
    const size_t npart = use_path == 2 ? (size_t)nb_group : 0;
    const auto w_bb = work.add<double>(npart), w_rz = work.add<double>(npart), w_rr = work.add<double>(npart);
    const auto w_pq = work.add<double>(npart);
    const auto w_a = work.add<double>(use_path == 2 ? nb_edge : 0), w_b = work.add<double>(use_path == 2 ? nb_edge : 0);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    const size_t lds = plan.lds_bytes;
    if (use_path == 1)
        SFM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pa_persistent),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const bool timed = call_timing();
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_adj, adj_start.data(), s));
    SFM_TRY(in.upload(i_code, ent_code.data(), s));
    SFM_TRY(in.upload(i_nbr, ent_nbr.data(), s));
    SFM_TRY(in.upload(i_ij, l_ij.data(), s));
    SFM_TRY(in.upload(i_dir, l_dir.data(), s));
    SFM_TRY(in.upload(i_weight, l_w.data(), s));
    SFM_TRY(work.upload(w_w, l_w.data(), s));
    SFM_TRY(work.upload(w_s, l_s.data(), s));
    // the iteration counts, the error word, the residuals, the ticks and path 2's state: contiguous slots, zeroed
    SFM_HIP(hipMemsetAsync(out.ptr(o_it), 0, (o_state.off + sizeof(PaState)) - o_it.off, s));
    if (use_path == 2) SFM_HIP(hipMemsetAsync(out.ptr(o_C), 0, o_C.bytes(), s));  // round 0 starts from zero
    SFM_TRY(tm.mark(s));

    const PaGraph gr{in.ptr(i_adj), in.ptr(i_code), in.ptr(i_nbr), in.ptr(i_ij), in.ptr(i_dir), in.ptr(i_weight),
                     work.ptr(w_w), work.ptr(w_s), M, root, (int32_t)El, G};
    const PaParams pr{mu, sigma, threshold, cg_tol, rounds, cg_max_iters};
    const PaEdgeOut eo{out.ptr(o_ang), out.ptr(o_len), out.ptr(o_inl)};
    double cg_ms = 0.0;
    if (use_path == 1) {
        hipLaunchKernelGGL(k_pa_persistent, dim3(1), dim3(PA_T1), lds, s, gr, pr, eo, out.ptr(o_C), out.ptr(o_it),
                           out.ptr(o_res), out.ptr(o_err), out.ptr(o_ticks));
        SFM_HIP(hipGetLastError());
    } else {
        const PaBufs b{out.ptr(o_C), work.ptr(w_r), work.ptr(w_z), work.ptr(w_q), {work.ptr(w_p0), work.ptr(w_p1)},
                       work.ptr(w_D), work.ptr(w_bb), work.ptr(w_rz), work.ptr(w_rr), work.ptr(w_pq), work.ptr(w_a),
                       work.ptr(w_b), out.ptr(o_state), out.ptr(o_it), out.ptr(o_res), nb_group, nb_node, nb_edge};
        const dim3 T(PA_T2), g_group((unsigned)nb_group), g_node((unsigned)nb_node), g_edge((unsigned)nb_edge);
        PaState st{};
        for (int32_t round = 0; round < rounds && !st.error; ++round) {
            hipLaunchKernelGGL(k_pa_setup, g_group, T, 0, s, gr, pr, b);
            SFM_HIP(hipGetLastError());
            st.stopped = 0;
            // iteration cg_max_iters is the apply launch alone: it ends the solve if nothing did before
            for (int32_t k = 0; k <= cg_max_iters && !st.stopped && !st.error;) {
                const int32_t k_end = (int32_t)std::min<int64_t>((int64_t)k + PA_CG_BATCH, (int64_t)cg_max_iters + 1);
                if (timed) SFM_HIP(hipEventRecord(c->ev[5], s));
                for (; k < k_end; ++k) {
                    hipLaunchKernelGGL(k_pa_apply, g_group, T, 0, s, gr, pr, b, round, k);
                    if (k < cg_max_iters) hipLaunchKernelGGL(k_pa_update, g_node, T, 0, s, gr, b, k);
                    SFM_HIP(hipGetLastError());
                }
                if (timed) SFM_HIP(hipEventRecord(c->ev[6], s));
                SFM_TRY(out.download(&st, o_state, s));
                SFM_HIP(hipStreamSynchronize(s));
                if (timed) {
                    float t = 0;
                    (void)hipEventElapsedTime(&t, c->ev[5], c->ev[6]);
                    cg_ms += t;
                }
            }
            hipLaunchKernelGGL(k_pa_proj, g_edge, T, 0, s, gr, b);
            hipLaunchKernelGGL(k_pa_normalise, g_node, T, 0, s, gr, b);
            hipLaunchKernelGGL(k_pa_reweight, g_edge, T, 0, s, gr, pr, eo, b);
            SFM_HIP(hipGetLastError());
        }
    }
    SFM_TRY(tm.mark(s));

    std::vector<double> h_C(3 * (size_t)M), h_ang((size_t)El), h_len((size_t)El), h_res((size_t)rounds);
    std::vector<uint8_t> h_inl((size_t)El);
    std::vector<int32_t> h_it((size_t)rounds);
    int32_t h_err = 0;
    long long h_ticks = 0;
    PaState h_state{};
    SFM_TRY(out.download(h_C.data(), o_C, s));
    SFM_TRY(out.download(h_ang.data(), o_ang, s));
    SFM_TRY(out.download(h_len.data(), o_len, s));
    SFM_TRY(out.download(h_inl.data(), o_inl, s));
    SFM_TRY(out.download(h_it.data(), o_it, s));
    SFM_TRY(out.download(h_res.data(), o_res, s));
    SFM_TRY(out.download(&h_err, o_err, s));
    SFM_TRY(out.download(&h_ticks, o_ticks, s));
    SFM_TRY(out.download(&h_state, o_state, s));
    SFM_TRY(tm.finish(s));
    if (timed) {  // [3]: the CG iterations alone (path 1: the device's wall clock around the loops of its one launch)
        float t[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&t[k], c->ev[k], c->ev[k + 1]);
        if (use_path == 1) {
            int khz = 0;
            (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device);
            cg_ms = khz > 0 ? (double)h_ticks / khz : 0.0;
        }
        const double t4[4] = {t[0], t[1], t[2], cg_ms};
        set_timings(t4, 4);
    }
    if (h_err || h_state.error) {
        set_error("numeric: the mean baseline c of a round is not finite and positive");
        return SFM_ERR_NUMERIC;
    }
    for (int32_t k = 0; k < M; ++k) {
        for (int t = 0; t < 3; ++t) C[3 * (size_t)solved[k] + t] = h_C[3 * (size_t)k + t];
        info[solved[k]] = k == root ? 1 : 0;
    }
    for (int64_t k = 0; k < El; ++k) {
        edge_angle[edges[k]] = h_ang[k];
        edge_length[edges[k]] = h_len[k];
        edge_inlier[edges[k]] = h_inl[k];
    }
    for (int32_t k = 0; k < rounds; ++k) {
        cg_iters[k] = h_it[k];
        cg_residual[k] = h_res[k];
    }
    return 0;
}
