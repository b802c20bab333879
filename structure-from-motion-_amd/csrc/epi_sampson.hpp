// The fundamental matrix of batched pair verification (verify_pairs.hip): one
// convention from the design row to the score, x2^T F x1 = 0, a model of unit
// Frobenius norm and the squared Sampson distance as the inlier rule.  The
// drop-ins keep the reference's arithmetic (sfm_geom.hpp: f8_points*, f8_finish,
// epi_inlier), whose design row solves x1^T F x2 = 0 while its denormalisation
// and score assume x2^T F x1 = 0; nothing of that is touched here, these
// functions stand beside it.
#pragma once
#include "hyp_batch.hpp"
#include "sfm_geom.hpp"

namespace sfm {

// Design row of x2^T F x1 = 0 for F row-major: (a, b) the normalised first
// point, (c, d) the second.
__device__ __forceinline__ void vp_row(double a, double b, double c, double d, double (&r)[9]) {
#pragma clang fp contract(off)
    r[0] = c * a; r[1] = c * b; r[2] = c;
    r[3] = d * a; r[4] = d * b; r[5] = d;
    r[6] = a; r[7] = b; r[8] = 1.0;
}

// G / |G|_F with the sign that makes the entry of largest magnitude (the first
// such in row-major order) positive.  G = 0 or not finite gives NaNs.
__device__ __forceinline__ void vp_unit(const double (&G)[9], double (&F)[9]) {
#pragma clang fp contract(off)
    double n2 = 0.0, big = -1.0, at = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        n2 += G[k] * G[k];
        const double m = fabs(G[k]);
        if (m > big) { big = m; at = G[k]; }
    }
    const double nrm = at < 0.0 ? -sqrt(n2) : sqrt(n2);
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = G[k] / nrm;
}

// f: the normalised null vector, row-major 3 x 3.  Rank 2 as f8_finish forms it
// (F - (F v3) v3^T, or Jacobi where F is nearly rank 1), F = T2^T F2 T1, then
// vp_unit: no division by F[2,2], which may be 0.
__device__ __forceinline__ void vp_finish(const double (&f)[9], const Hartley &h1, const Hartley &h2,
                                          double (&F)[9]) {
#pragma clang fp contract(off)
    double F2[3][3];
    double v3[3];
    if (smallest_right_sv(f, v3)) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double fv = f[r * 3] * v3[0] + f[r * 3 + 1] * v3[1] + f[r * 3 + 2] * v3[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) F2[r][c] = f[r * 3 + c] - fv * v3[c];
        }
    } else {
        double b[3][3], W[3][3];  // b[col][row]
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) b[c][r] = f[r * 3 + c];
        jacobi_onesided<3, 3, 24>(b, W);
        const int z = weakest_column<3, 3>(b);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k != z) acc += b[k][r] * W[c][k];
                F2[r][c] = acc;
            }
    }
    // T = [[s, 0, ox], [0, s, oy], [0, 0, 1]]: the rows of T2^T F2, then its
    // columns times T1, with the zeros of T left out
    double tmp[3][3], G[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        tmp[0][c] = h2.s * F2[0][c];
        tmp[1][c] = h2.s * F2[1][c];
        tmp[2][c] = (h2.ox * F2[0][c] + h2.oy * F2[1][c]) + F2[2][c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = tmp[r][0] * h1.s;
        G[3 * r + 1] = tmp[r][1] * h1.s;
        G[3 * r + 2] = (tmp[r][0] * h1.ox + tmp[r][1] * h1.oy) + tmp[r][2];
    }
    vp_unit(G, F);
}

// The 8-point hypothesis on a group of 8 consecutive lanes, lane i holding
// sample point i (p in the first image, q in the second): hartley8_group, one
// design row per lane, the Householder LQ of f8_points_group8 (reflector k and
// its tau broadcast from row k's lane, the back-substitution on every lane's
// own copy of n), then vp_finish on every lane (the same bits).  F to every lane.
__device__ __forceinline__ void vp_fit_group8(double px, double py, double qx, double qy, double (&F)[9]) {
#pragma clang fp contract(off)
    const int i = threadIdx.x & 7;
    const Hartley h1 = hartley8_group(px, py), h2 = hartley8_group(qx, qy);
    double A[9];
    vp_row(h1.s * px + h1.ox, h1.s * py + h1.oy, h2.s * qx + h2.ox, h2.s * qy + h2.oy, A);
    double tau = 0;  // this lane's reflector (row i)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (i == k) {
            double nrm2 = 0;
#pragma unroll
            for (int j = k; j < 9; ++j) nrm2 += A[j] * A[j];
            const double nrm = sqrt(nrm2);
            const double alpha = A[k] > 0 ? -nrm : nrm;
            A[k] -= alpha;
            double vtv = 0;
#pragma unroll
            for (int j = k; j < 9; ++j) vtv += A[j] * A[j];
            tau = nrm2 > 0 ? 2.0 / vtv : 0.0;
        }
        double v[9];
#pragma unroll
        for (int j = k; j < 9; ++j) v[j] = __shfl(A[j], k, 8);
        const double tk = __shfl(tau, k, 8);
        if (i > k) {
            double d = 0;
#pragma unroll
            for (int j = k; j < 9; ++j) d += A[j] * v[j];
            d *= tk;
#pragma unroll
            for (int j = k; j < 9; ++j) A[j] -= d * v[j];
        }
    }
    double n[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) n[j] = (j == 8) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        double v[9];
#pragma unroll
        for (int j = k; j < 9; ++j) v[j] = __shfl(A[j], k, 8);
        const double tk = __shfl(tau, k, 8);
        double d = 0;
#pragma unroll
        for (int j = k; j < 9; ++j) d += v[j] * n[j];
        d *= tk;
#pragma unroll
        for (int j = k; j < 9; ++j) n[j] -= d * v[j];
    }
    vp_finish(n, h1, h2, F);
}

// The inlier rule: e = x2^T F x1, den = (F x1)_0^2 + (F x1)_1^2 + (F^T x2)_0^2 +
// (F^T x2)_1^2; an inlier where den > 0 and e^2 < thr2 den -- the squared
// Sampson distance e^2 / den against the squared threshold, without a division
// or a square root.  False for anything not finite.
__device__ __forceinline__ bool vp_inlier(const double *F, double x, double y, double u, double v, double thr2,
                                          double &e2, double &den) {
#pragma clang fp contract(off)
    const double l0 = (F[0] * x + F[1] * y) + F[2];
    const double l1 = (F[3] * x + F[4] * y) + F[5];
    const double l2 = (F[6] * x + F[7] * y) + F[8];
    const double m0 = (F[0] * u + F[3] * v) + F[6];
    const double m1 = (F[1] * u + F[4] * v) + F[7];
    const double e = (u * l0 + v * l1) + l2;
    den = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1);
    e2 = e * e;
    return den > 0.0 && e2 < thr2 * den;
}

struct EpiPair {
    const double2 *x1, *x2;  // the pair's first correspondence
    int n;
};

// mask[i] = the inlier rule under F for the pair's correspondence i; count and
// the inliers' squared Sampson distances summed over a workgroup of NT threads
// (thread t owns i = t, t + NT, ...).  red: NT / 64 x NV, NV >= 2.
template <int NT, int NV>
__device__ __forceinline__ void epi_mask(const EpiPair &w, const double *F, double thr2, uint8_t *mask, int &count,
                                         double &cost, double (*red)[NV]) {
#pragma clang fp contract(off)
    double acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;
    for (int i = threadIdx.x; i < w.n; i += NT) {
        const double2 p = w.x1[i], q = w.x2[i];
        double e2, den;
        const bool in = vp_inlier(F, p.x, p.y, q.x, q.y, thr2, e2, den);
        mask[i] = in ? 1 : 0;
        if (in) {
            acc[0] += 1.0;
            acc[1] += e2 / den;
        }
    }
    wg_sum<NT / 64, NV>(acc, red);
    count = (int)acc[0];
    cost = acc[1];
}

enum EpiStop { EPI_ROUNDS, EPI_UNCHANGED, EPI_WORSE, EPI_DECLINED };  // how epi_refit_rounds ended

// The refit rounds of a pair's winner, from the state (F, n_inl, cost, mask) that
// epi_mask left.  A round: propose(mask, n_inl, Fn) fits a model to the current
// inliers, or returns false, which ends the rounds; Fn is scored into trial
// and replaces the state only if it is not worse -- then accept() lets the
// caller keep what else it holds of the proposal -- and an unchanged mask ends
// the rounds.  mask: the pair's part of the output mask; trial: as many bytes
// of scratch.
template <int NT, int NV, class Propose, class Accept>
__device__ __forceinline__ EpiStop epi_refit_rounds(const EpiPair &w, double thr2, double (&F)[9], int &n_inl,
                                                    double &cost, uint8_t *mask, uint8_t *trial, int rounds,
                                                    double (*red)[NV], Propose propose, Accept accept) {
    for (int round = 0; round < rounds; ++round) {
        double Fn[9], cost2;
        int n2;
        if (!propose(mask, n_inl, Fn)) return EPI_DECLINED;
        epi_mask<NT>(w, Fn, thr2, trial, n2, cost2, red);
        if (!not_worse(n2, cost2, n_inl, cost)) return EPI_WORSE;
        const int changed = adopt_trial<NT>(mask, trial, w.n);
#pragma unroll
        for (int j = 0; j < 9; ++j) F[j] = Fn[j];
        n_inl = n2;
        cost = cost2;
        accept();
        if (!changed) return EPI_UNCHANGED;
    }
    return EPI_ROUNDS;
}

// The end of a refit kernel for pair p: without a winner (hyp < 0) the mask is
// cleared; thread 0 stores the pair's scalars.
template <int NT>
__device__ __forceinline__ void epi_store_pair(int64_t p, int n, uint8_t *mask, int32_t hyp, int32_t count,
                                               double cost, int n_inl, int info, double *cost_out, int32_t *n_inl_out,
                                               int32_t *hyp_out, int32_t *count_out, int32_t *info_out) {
    if (hyp < 0)
        for (int i = threadIdx.x; i < n; i += NT) mask[i] = 0;
    if (threadIdx.x == 0) {
        cost_out[p] = cost;
        n_inl_out[p] = n_inl;
        hyp_out[p] = hyp;
        count_out[p] = hyp < 0 ? 0 : count;
        info_out[p] = info;
    }
}

}  // namespace sfm
