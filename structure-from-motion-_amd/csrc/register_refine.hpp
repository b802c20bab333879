// What the two view-registration entry points share (register_views.hip:
// 6-point DLT hypotheses; register_p3p.hip: calibrated 3-point hypotheses),
// which is everything but the fit of a hypothesis: the inlier rule and its
// division-free prefilter, the score loop of the fit-and-score kernels
// (rv_score), the winner-and-refit kernel (k_rv_refine) -- the winner's rule,
// then rounds of Levenberg-Marquardt on the 6 pose parameters over the current
// inliers, a re-score of the whole view and the not-worse test -- and the host
// driver of a call (rv_run).  The kernel takes the kind of hypothesis as a
// policy type, the driver as an RvSpec.  The fixed-order sums are the
// scaffold's (hyp_batch.hpp).
#pragma once
#include <cmath>
#include <cstring>

#include "hyp_batch.hpp"
#include "lm_small.hpp"
#include "pnp_model.hpp"
#include "select.hpp"
#include "sfm_geom.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int RV_THREADS = 256;
constexpr int RV_WAVES = RV_THREADS / 64;
constexpr int RV_TILE = 1024;                      // correspondences per LDS tile

// h = P [X; 1]
__device__ __forceinline__ void rv_h(const double *P, double X, double Y, double Z, double &h0, double &h1,
                                     double &h2) {
    h0 = (P[0] * X + P[2] * Z) + (P[1] * Y + P[3]);
    h1 = (P[4] * X + P[6] * Z) + (P[5] * Y + P[7]);
    h2 = (P[8] * X + P[10] * Z) + (P[9] * Y + P[11]);
}

// The inlier rule: h2 > 0, not |h2| < 1e-8 and (u - h0/h2)^2 + (v - h1/h2)^2 <
// thr2; e2 is the squared error (meaningful where the depth test holds).
__device__ __forceinline__ bool rv_exact(double h0, double h1, double h2, double u, double v, double thr2,
                                         double &e2) {
    e2 = 0.0;
    if (!(h2 > 0.0) || fabs(h2) < 1e-8) return false;
    const double ru = u - h0 / h2, rv = v - h1 / h2;
    e2 = ru * ru + rv * rv;
    return e2 < thr2;
}

// The same decision without the two divisions where it is not close: the
// distance scaled by |h2|, sqrt((u h2 - h0)^2 + (v h2 - h1)^2), differs from
// |h2| times the distance rv_exact forms by rounding alone -- a few 1e-16 of
// |h0| + |u h2| + |h1| + |v h2| and a few 1e-16 relative -- so a threshold
// narrowed / widened by 3e-12 of that sum and 1e-9 relative decides for
// rv_exact with four orders to spare; the band between, and anything not
// finite, takes rv_exact itself.
__device__ __forceinline__ bool rv_inlier(const double *P, double X, double Y, double Z, double u, double v,
                                          double thr, double thr2) {
    double h0, h1, h2;
    rv_h(P, X, Y, Z, h0, h1, h2);
    if (!(h2 > 0.0) || fabs(h2) < 1e-8) return false;
    const double a = fma(u, h2, -h0), b = fma(v, h2, -h1);
    const double s2 = a * a + b * b;
    const double E = ((fabs(h0) + fabs(u) * h2) + (fabs(h1) + fabs(v) * h2)) * 3e-12;
    const double lo = thr * (1.0 - 1e-9) * h2 - E, hi = thr * (1.0 + 1e-9) * h2 + E;
    if (lo > 0.0 && s2 < lo * lo) return true;
    if (s2 > hi * hi) return false;
    double e2;
    return rv_exact(h0, h1, h2, u, v, thr2, e2);
}

// correspondence c (an index into pt_idx / xy) to place i of the score loop's LDS tile
__device__ __forceinline__ void rv_stage(const double *__restrict__ Xg, const int32_t *__restrict__ pt_idx,
                                         const double2 *__restrict__ xy, int64_t c, double *sX, double2 *sxy, int i) {
    const int64_t pi = pt_idx[c];
    sX[3 * i] = Xg[3 * pi];
    sX[3 * i + 1] = Xg[3 * pi + 1];
    sX[3 * i + 2] = Xg[3 * pi + 2];
    sxy[i] = xy[c];
}

// The score loop of a fit-and-score kernel: the view's n correspondences (from
// vs on) through the LDS tile sX / sxy, a wave per entry s < n_entries.
// slot(s, m) names the entry's model sP[m] and counter sCnt[m], or returns
// false for an entry that is not scored.  sCnt starts at 0 and the caller's
// barrier stands between that and this; the counts are complete at return.
template <class Slot>
__device__ __forceinline__ void rv_score(const double *__restrict__ Xg, const int32_t *__restrict__ pt_idx,
                                         const double2 *__restrict__ xy, int64_t vs, int n, double thr, int n_entries,
                                         Slot slot, const double (*sP)[12], int32_t *sCnt, double *sX, double2 *sxy) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double thr2 = thr * thr;
    for_each_tile<RV_THREADS, RV_TILE>(
        n, [&](int i, int c) { rv_stage(Xg, pt_idx, xy, vs + c, sX, sxy, i); },
        [&](int nt) {
            for (int s = wave; s < n_entries; s += RV_WAVES) {
                int m;
                if (!slot(s, m)) continue;
                double P[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) P[j] = sP[m][j];
                const int cnt = wave_count(nt, [&](int i) {
                    const double2 q = sxy[i];
                    return rv_inlier(P, sX[3 * i], sX[3 * i + 1], sX[3 * i + 2], q.x, q.y, thr, thr2);
                });
                if (lane == 0) sCnt[m] += cnt;  // this wave alone owns entry s
            }
        });
}

struct RvView {
    const double *X;
    const int32_t *pt;
    const double2 *xy;  // pt, xy: the view's first correspondence
    int n;
};

// mask[i] = the inlier rule under P for the view's correspondence i; count and
// the inliers' squared errors summed (thread t owns i = t, t + 256, ...)
__device__ __forceinline__ void rv_mask(const RvView &w, const double *P, double thr2, uint8_t *mask, int &count,
                                        double &cost, double (*red)[2]) {
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < w.n; i += RV_THREADS) {
        const int64_t pi = w.pt[i];
        const double2 q = w.xy[i];
        double h0, h1, h2, e2;
        rv_h(P, w.X[3 * pi], w.X[3 * pi + 1], w.X[3 * pi + 2], h0, h1, h2);
        const bool in = rv_exact(h0, h1, h2, q.x, q.y, thr2, e2);
        mask[i] = in ? 1 : 0;
        if (in) {
            acc[0] += 1.0;
            acc[1] += e2;
        }
    }
    wg_sum<RV_WAVES, 2>(acc, red);
    count = (int)acc[0];
    cost = acc[1];
}

constexpr int RV_NV = 29;  // J^T J (21, upper, row-major packed) | J^T r (6) | cost | bad

// Residuals r = (u - h0/h2, v - h1/h2), h = K R (X - C), over the masked
// correspondences, with the Jacobian of the left-multiplied rotation increment
// w (R <- exp([w]x) R, d Xc / d w = -[Xc]x) and of C (d Xc / d C = -R).  A
// correspondence that fails the depth test at this pose makes the cost +inf,
// so that a trial step which pushes an inlier behind the camera is refused.
__device__ __forceinline__ void rv_eval(const RvView &w, const Cam3 &K, const double (&R)[9], const double (&C)[3],
                                        const uint8_t *mask, double (&A)[21], double (&g)[6], double &cost,
                                        double (*red)[RV_NV]) {
    double s[RV_NV];
#pragma unroll
    for (int j = 0; j < RV_NV; ++j) s[j] = 0.0;
    for (int i = threadIdx.x; i < w.n; i += RV_THREADS) {
        if (!mask[i]) continue;
        const int64_t pi = w.pt[i];
        const double2 q = w.xy[i];
        const double d0 = w.X[3 * pi] - C[0], d1 = w.X[3 * pi + 1] - C[1], d2 = w.X[3 * pi + 2] - C[2];
        double xc[3], h[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) xc[r] = (R[3 * r] * d0 + R[3 * r + 2] * d2) + R[3 * r + 1] * d1;
#pragma unroll
        for (int r = 0; r < 3; ++r) h[r] = (K.k[3 * r] * xc[0] + K.k[3 * r + 2] * xc[2]) + K.k[3 * r + 1] * xc[1];
        if (!(h[2] > 0.0) || fabs(h[2]) < 1e-8) {
            s[28] += 1.0;
            continue;
        }
        const double inv = 1.0 / h[2];
        const double pu = h[0] * inv, pv = h[1] * inv;
        const double ru = q.x - pu, rv = q.y - pv;
        s[27] += ru * ru + rv * rv;
        // d Xc per parameter: e_j x Xc for the rotation, -R[:, j] for C
        const double dx[6][3] = {{0.0, -xc[2], xc[1]}, {xc[2], 0.0, -xc[0]}, {-xc[1], xc[0], 0.0},
                                 {-R[0], -R[3], -R[6]}, {-R[1], -R[4], -R[7]}, {-R[2], -R[5], -R[8]}};
        double ju[6], jv[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double e0 = (K.k[0] * dx[j][0] + K.k[2] * dx[j][2]) + K.k[1] * dx[j][1];
            const double e1 = (K.k[3] * dx[j][0] + K.k[5] * dx[j][2]) + K.k[4] * dx[j][1];
            const double e2 = (K.k[6] * dx[j][0] + K.k[8] * dx[j][2]) + K.k[7] * dx[j][1];
            ju[j] = (pu * e2 - e0) * inv;
            jv[j] = (pv * e2 - e1) * inv;
            s[21 + j] += ju[j] * ru + jv[j] * rv;
        }
        int u = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) s[u++] += ju[a] * ju[b] + jv[a] * jv[b];
    }
    wg_sum<RV_WAVES, RV_NV>(s, red);
#pragma unroll
    for (int j = 0; j < 21; ++j) A[j] = s[j];
#pragma unroll
    for (int j = 0; j < 6; ++j) g[j] = s[21 + j];
    cost = s[28] > 0.0 ? INFINITY : s[27];
}

// (A + lam diag(A)) d = -g by Cholesky; false where the damped matrix is not
// positive definite or the step is not finite
__device__ __forceinline__ bool rv_solve6(const double (&A)[21], const double (&g)[6], double lam, double (&d)[6]) {
    double G[21];
    int u = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            G[u] = a == b ? A[u] + lam * A[u] : A[u];
            ++u;
        }
    double L[6][6];
    if (!chol6(G, L)) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {  // L^T y = -g
        double t = -g[i];
#pragma unroll
        for (int j = 0; j < i; ++j) t -= L[j][i] * y[j];
        y[i] = t / L[i][i];
    }
    bool ok = true;
#pragma unroll
    for (int i = 5; i >= 0; --i) {  // L d = y
        double t = y[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) t -= L[i][j] * d[j];
        d[i] = t / L[i][i];
        ok = ok && isfinite(d[i]);
    }
    return ok;
}

__device__ __forceinline__ double rv_diag(const double (&A)[21], int j) {
    // packed upper, row-major: row j starts at j * 6 - j (j - 1) / 2
    return A[j * 6 - j * (j - 1) / 2];
}

// Levenberg-Marquardt on (R, C) over the masked correspondences: Marquardt's
// scaling, lambda 1e-3, / 10 on an accepted step and x 10 on a rejected one, a
// step accepted only where the cost falls; MINPACK's stop tests at 1e-8 with
// mv_refine's codes (1 ftol, 2 xtol, 3 both, 4 gtol, 5 max_nfev).  The size of
// the parameter vector in the xtol test is sqrt(angle(R)^2 + |C|^2).  Every
// thread runs the same scalar code on the same sums.  -4: cost at the start
// not finite (pose kept).
__device__ int rv_lm(const RvView &w, const Cam3 &K, double (&R)[9], double (&C)[3], const uint8_t *mask,
                     int max_nfev, double (*red)[RV_NV]) {
    const double tol = 1e-8;
    double A[21], g[6], c0;
    rv_eval(w, K, R, C, mask, A, g, c0, red);
    if (!isfinite(c0)) return -4;
    int nfev = 1, info = 0;
    double lam = 1e-3;
    while (info == 0) {
        double gn = 0.0;
        if (c0 != 0.0) {
            const double fn = sqrt(c0);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double a = rv_diag(A, j);
                if (a > 0.0) gn = fmax(gn, fabs(g[j]) / (sqrt(a) * fn));
            }
        }
        if (gn <= tol) {
            info = 4;
            break;
        }
        bool accepted = false;
        while (!accepted && info == 0) {
            if (nfev >= max_nfev) {
                info = 5;
                break;
            }
            ++nfev;
            double d[6];
            if (!rv_solve6(A, g, lam, d)) {
                lam *= 10.0;
                continue;
            }
            double dR[9], Rt[9], Ct[3] = {C[0] + d[3], C[1] + d[4], C[2] + d[5]};
            rotvec_to_R(d[0], d[1], d[2], dR);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Rt[3 * r + c] = (dR[3 * r] * R[c] + dR[3 * r + 2] * R[6 + c]) + dR[3 * r + 1] * R[3 + c];
            double A1[21], g1[6], c1;
            rv_eval(w, K, Rt, Ct, mask, A1, g1, c1, red);
            // the linear model's reduction |r|^2 - |r + J d|^2
            double gd = 0.0, dAd = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                gd += g[a] * d[a];
                double Ad = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) Ad += A[a <= b ? a * 6 - a * (a - 1) / 2 + (b - a) : b * 6 - b * (b - 1) / 2 + (a - b)] * d[b];
                dAd += d[a] * Ad;
            }
            const double prered = -(2.0 * gd + dAd) / c0;
            const double actred = 1.0 - c1 / c0;
            double pn = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) pn += d[a] * d[a];
            const double pnorm = sqrt(pn);
            if (c1 < c0) {
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = Rt[j];
#pragma unroll
                for (int j = 0; j < 3; ++j) C[j] = Ct[j];
                c0 = c1;
#pragma unroll
                for (int j = 0; j < 21; ++j) A[j] = A1[j];
#pragma unroll
                for (int j = 0; j < 6; ++j) g[j] = g1[j];
                lam = fmax(lam * 0.1, 1e-15);
                accepted = true;
            } else {
                lam *= 10.0;
            }
            const double sx = R[7] - R[5], sy = R[2] - R[6], sz = R[3] - R[1];
            const double ang = atan2(0.5 * sqrt(sx * sx + sy * sy + sz * sz), 0.5 * ((R[0] + R[4] + R[8]) - 1.0));
            const double xnorm = sqrt(ang * ang + (C[0] * C[0] + C[1] * C[1] + C[2] * C[2]));
            const bool fhit = fabs(actred) <= tol && prered <= tol && 0.5 * actred <= prered;
            const bool xhit = pnorm <= tol * xnorm;
            if (fhit) info = 1;
            if (xhit) info = fhit ? 3 : 2;
        }
    }
    return info;
}

// The winner's mask under its projection P, then -- where its count bc reaches
// min_inliers -- up to refit_rounds rounds from its pose (R, C).  mask: the
// view's part of the output mask; trial: as many bytes of scratch.  Returns
// info (-3, -4, 0 or the last refit's stop code); R, C, cost, n_inl are the
// state that is kept.
__device__ __forceinline__ int rv_refit(const RvView &w, const Cam3 &K, const double *P, double thr2, int32_t bc,
                                        int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, double (&R)[9],
                                        double (&C)[3], double &cost, int &n_inl, uint8_t *mask, uint8_t *trial,
                                        double (*red)[RV_NV], double (*red2)[2]) {
    rv_mask(w, P, thr2, mask, n_inl, cost, red2);
    int info = -3;
    if (bc >= min_inliers) {
        info = 0;
        for (int round = 0; round < refit_rounds; ++round) {
            double Rn[9], Cn[3];
#pragma unroll
            for (int j = 0; j < 9; ++j) Rn[j] = R[j];
#pragma unroll
            for (int j = 0; j < 3; ++j) Cn[j] = C[j];
            info = rv_lm(w, K, Rn, Cn, mask, max_nfev, red);
            if (info < 0) break;
            double Pn[12], cost2;
            int n2;
            pnp_projection(K, Cn, Rn, Pn);
            rv_mask(w, Pn, thr2, trial, n2, cost2, red2);
            if (!not_worse(n2, cost2, n_inl, cost)) break;
            const int changed = adopt_trial<RV_THREADS>(mask, trial, w.n);
#pragma unroll
            for (int j = 0; j < 9; ++j) R[j] = Rn[j];
#pragma unroll
            for (int j = 0; j < 3; ++j) C[j] = Cn[j];
            n_inl = n2;
            cost = cost2;
            if (!changed) break;
        }
    }
    return info;
}

// One workgroup per view: the winner over the view's H x SLOTS_PER_HYP slots,
// its mask and the refit from its pose.  modelsP / modelsCR (12 words a slot)
// and counts are the fit-and-score kernel's; mask2: scratch of n_corr bytes.
// Views below Hyp::MIN_N are the host's (info -1): nothing of them is read.
// Most inliers win; Hyp says what follows:
//   SLOTS_PER_HYP   models a hypothesis brings (best_hyp is the hypothesis, not the slot)
//   MIN_N           correspondences of a live view
//   COST_TIE_BREAK  among slots of equal count the smaller sum of the inliers'
//                   squared errors wins (rv_mask's, one pass over the view per
//                   tying slot), then the earlier slot; without it the earlier
//                   slot at once
//   usable(modelsP, modelsCR, n_sol, g)  with every count 0: whether hypothesis
//                   g = v H + h of the call may win; its first slot then does,
//                   for the earliest such h.  n_sol is Hyp's to read or not.
template <class Hyp>
__global__ void __launch_bounds__(RV_THREADS)
k_rv_refine(const double *__restrict__ Xg, const int64_t *__restrict__ view_start,
            const int32_t *__restrict__ pt_idx, const double2 *__restrict__ xy, int32_t H, Cam3 K, double thr,
            int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, const double *__restrict__ modelsP,
            const double *__restrict__ modelsCR, const int32_t *__restrict__ counts, uint8_t *mask2,
            double *__restrict__ C_out, double *__restrict__ R_out, double *__restrict__ cost_out,
            int32_t *__restrict__ n_inl_out, int32_t *__restrict__ hyp_out, int32_t *__restrict__ count_out,
            int32_t *__restrict__ info_out, uint8_t *inlier, const int32_t *__restrict__ n_sol) {
    constexpr int NS = Hyp::SLOTS_PER_HYP;
    __shared__ int32_t sc[RV_WAVES];
    __shared__ int64_t sh[RV_WAVES];
    __shared__ int32_t sFirst;
    __shared__ double red[RV_WAVES][RV_NV];
    __shared__ double red2[RV_WAVES][2];
    const int tid = threadIdx.x;
    const int64_t v = blockIdx.x;
    const int64_t vs = view_start[v];
    const int n = (int)(view_start[v + 1] - vs);
    if (n < Hyp::MIN_N) return;
    const RvView w{Xg, pt_idx + vs, xy + vs, n};
    uint8_t *mask = inlier + vs, *trial = mask2 + vs;
    const double thr2 = thr * thr;
    const int32_t S = H * NS;  // the view's slots
    const int32_t *cnt = counts + v * S;
    const double *mP = modelsP + v * S * 12, *mCR = modelsCR + v * S * 12;

    int32_t bc;
    int64_t bh;
    if (tid == 0) sFirst = S;
    wg_select_best<RV_THREADS>(cnt, S, sc, sh, bc, bh);  // holds a barrier
    if (bh < 0) {  // every count is 0: the earliest usable hypothesis, if any
        for (int32_t h = tid; h < H; h += RV_THREADS)
            if (Hyp::usable(modelsP, modelsCR, n_sol, v * H + h)) {
                atomicMin(&sFirst, h * NS);
                break;
            }
        __syncthreads();
        bh = sFirst < S ? sFirst : -1;
        bc = 0;
    } else if constexpr (Hyp::COST_TIE_BREAK) {
        // the slots that tie on the count, in order
        double P[12], best, c;
        int k;
#pragma unroll
        for (int j = 0; j < 12; ++j) P[j] = mP[bh * 12 + j];
        rv_mask(w, P, thr2, trial, k, best, red2);
        int32_t cur = (int32_t)bh;
        while (true) {
            __syncthreads();
            if (tid == 0) sFirst = S;
            __syncthreads();
            for (int32_t i = cur + 1 + tid; i < S; i += RV_THREADS)
                if (cnt[i] == bc) {
                    atomicMin(&sFirst, i);
                    break;
                }
            __syncthreads();
            cur = sFirst;
            if (cur >= S) break;
#pragma unroll
            for (int j = 0; j < 12; ++j) P[j] = mP[(int64_t)cur * 12 + j];
            rv_mask(w, P, thr2, trial, k, c, red2);
            if (c < best) {
                best = c;
                bh = cur;
            }
        }
    }
    double C[3] = {0.0, 0.0, 0.0}, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, cost = 0.0;
    int info = -2, n_inl = 0;
    if (bh < 0) {
        for (int i = tid; i < n; i += RV_THREADS) mask[i] = 0;
    } else {
        double P[12];
        const double *m = mP + bh * 12, *mc = mCR + bh * 12;
#pragma unroll
        for (int j = 0; j < 12; ++j) P[j] = m[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) C[j] = mc[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = mc[3 + j];
        info = rv_refit(w, K, P, thr2, bc, min_inliers, refit_rounds, max_nfev, R, C, cost, n_inl, mask, trial, red,
                        red2);
    }
    if (tid == 0) {
        for (int j = 0; j < 3; ++j) C_out[3 * v + j] = C[j];
        for (int j = 0; j < 9; ++j) R_out[9 * v + j] = R[j];
        cost_out[v] = cost;
        n_inl_out[v] = n_inl;
        hyp_out[v] = bh < 0 ? -1 : (int32_t)(bh / NS);
        count_out[v] = bh < 0 ? 0 : bc;
        info_out[v] = info;
    }
}

// What an entry point is, to the driver.  Both fit-and-score kernels have one
// signature; Ki and n_sol are the calibrated one's (zeros and null otherwise).
using RvFitScore = void (*)(const double *Xg, const int64_t *view_start, const int32_t *pt_idx, const double2 *xy,
                            const int32_t *samples, int32_t H, Cam3 K, Cam3 Ki, const int32_t *blk_start,
                            const int32_t *tab, int32_t n_live, double thr, double *modelsP, double *modelsCR,
                            int32_t *counts, int32_t *n_sol);
using RvRefine = decltype(&k_rv_refine<void>);  // the signature does not depend on Hyp
struct RvSpec {
    int k;           // correspondences of a sample
    int min_n;       // ... of a live view, and the least min_inliers
    int slots;       // models per hypothesis
    int ht;          // most hypotheses per workgroup of fit_score
    bool calibrated; // hypotheses from the bearings K^-1 [x; 1], with an n_sol table
    RvFitScore fit_score;
    RvRefine refine;
    const char *min_inliers_msg, *too_large_msg;
};

// A call of either entry point, from the argument checks to the downloads.  The
// arguments are sfm_register_views_p3p's (include/sfmcore.h); n_sol is null
// for an entry point that is not calibrated.
inline int rv_run(const RvSpec &sp, const double *K, const double *X, int64_t n_pts, const int64_t *view_start,
                  int64_t V, const int32_t *pt_idx, const double *xy, int64_t n_corr, const int32_t *samples, int64_t H,
                  double threshold, int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, double *C, double *R,
                  double *cost, int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                  uint8_t *inlier, int32_t *n_sol, int32_t *counts, double *models, int device) {
    const int64_t NS = sp.slots;
    SFM_CHECK_ARG(V >= 0 && n_corr >= 0 && n_pts >= 0, "V < 0, n_corr < 0 or n_pts < 0");
    SFM_CHECK_ARG(H >= 1 && H <= (int64_t)1 << 20, "H must lie in [1, 2^20]");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0, "threshold must be finite and positive");
    SFM_CHECK_ARG(min_inliers >= sp.min_n, sp.min_inliers_msg);
    SFM_CHECK_ARG(refit_rounds >= 0, "refit_rounds < 0");
    SFM_CHECK_ARG(max_nfev > 0, "max_nfev must be positive");
    SFM_CHECK_ARG(V < (int64_t)0x7fffffff / (NS * H), sp.too_large_msg);
    SFM_CHECK_ARG(view_start && K, "null pointer");
    SFM_TRY(check_csr(view_start, V, n_corr, "view_start", "correspondence", 0x7fffffff,
                      "a view has too many correspondences"));
    const int64_t n_live = count_live(view_start, V, sp.min_n);
    SFM_CHECK_ARG(n_corr == 0 || (pt_idx && xy && X), "null pointer");
    SFM_TRY(check_index(pt_idx, n_corr, n_pts, "point index outside [0, n_pts)"));
    SFM_CHECK_ARG(n_live == 0 || samples, "null pointer");
    SFM_TRY(check_samples(view_start, V, samples, H, sp.k, sp.min_n, "sample outside [0, n_v)"));
    if (V == 0) return 0;
    SFM_CHECK_ARG(C && R && cost && n_inliers && best_hyp && best_count && info && (inlier || n_corr == 0),
                  "null pointer");
    // info -1: a view below the minimum.  Also what the live views start from.
    for (int64_t v = 0; v < V; ++v) {
        if (view_start[v + 1] - view_start[v] >= sp.min_n) continue;
        for (int j = 0; j < 3; ++j) C[3 * v + j] = 0.0;
        for (int j = 0; j < 9; ++j) R[9 * v + j] = j % 4 == 0 ? 1.0 : 0.0;
        cost[v] = 0.0;
        n_inliers[v] = 0;
        best_hyp[v] = -1;
        best_count[v] = 0;
        info[v] = -1;
        for (int64_t k = view_start[v]; k < view_start[v + 1]; ++k) inlier[k] = 0;
        if (n_sol) std::memset(n_sol + v * H, 0, (size_t)H * sizeof(int32_t));
        if (counts) std::memset(counts + v * H * NS, 0, (size_t)(H * NS) * sizeof(int32_t));
        if (models) std::memset(models + v * H * NS * 12, 0, (size_t)(H * NS * 12) * sizeof(double));
    }
    if (n_live == 0) return 0;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    TileTable tt;
    SFM_TRY(tt.build(c->pinned, n_live, view_start, V, sp.min_n, H, sp.ht, RV_TILE));

    const size_t VH = (size_t)V * (size_t)H;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_vs = in.add<int64_t>(V + 1);
    const auto i_xy = in.add<double2>(n_corr);
    const auto i_X = in.add<double>(3 * n_pts);
    const auto i_pt = in.add<int32_t>(n_corr), i_s = in.add<int32_t>(sp.k * VH);
    const auto i_t = in.add<int32_t>(tt.words());  // the block table
    const auto o_C = out.add<double>(3 * V), o_R = out.add<double>(9 * V), o_cost = out.add<double>(V);
    const auto o_info = out.add<int32_t>(V), o_ninl = out.add<int32_t>(V);
    const auto o_hyp = out.add<int32_t>(V), o_bc = out.add<int32_t>(V);
    const auto o_ns = out.add<int32_t>(sp.calibrated ? VH : 0), o_cnt = out.add<int32_t>(NS * VH);
    const auto o_mP = out.add<double>(12 * NS * VH), o_mCR = out.add<double>(12 * NS * VH);
    const auto o_mask = out.add<uint8_t>(n_corr), o_m2 = out.add<uint8_t>(n_corr);  // o_m2: the refits' trial mask
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    Cam3 cam, cam_inv{};
    std::memcpy(cam.k, K, sizeof cam.k);
    // a singular K gives bearings that are not finite, and with them hypotheses without solutions
    if (sp.calibrated) (void)inv3_adjugate(K, cam_inv.k);
    hipStream_t s = c->stream;
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_vs, view_start, s));
    SFM_TRY(in.upload(i_xy, xy, s));
    SFM_TRY(in.upload(i_X, X, s));
    SFM_TRY(in.upload(i_pt, pt_idx, s));
    SFM_TRY(in.upload(i_s, samples, s));
    SFM_TRY(in.upload(i_t, tt.blk, s));
    SFM_TRY(tm.mark(s));
    int32_t *d_ns = sp.calibrated ? out.ptr(o_ns) : nullptr;
    hipLaunchKernelGGL(sp.fit_score, dim3((unsigned)tt.blocks), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs),
                       in.ptr(i_pt), in.ptr(i_xy), in.ptr(i_s), (int32_t)H, cam, cam_inv, in.ptr(i_t),
                       in.ptr(i_t, n_live + 1), (int32_t)n_live, threshold, out.ptr(o_mP), out.ptr(o_mCR),
                       out.ptr(o_cnt), d_ns);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.split(s));  // [3]: the fit-and-score kernel alone
    hipLaunchKernelGGL(sp.refine, dim3((unsigned)V), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs), in.ptr(i_pt),
                       in.ptr(i_xy), (int32_t)H, cam, threshold, min_inliers, refit_rounds, max_nfev, out.ptr(o_mP),
                       out.ptr(o_mCR), out.ptr(o_cnt), out.ptr(o_m2), out.ptr(o_C), out.ptr(o_R), out.ptr(o_cost),
                       out.ptr(o_ninl), out.ptr(o_hyp), out.ptr(o_bc), out.ptr(o_info), out.ptr(o_mask), d_ns);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    SFM_TRY(for_each_live_run(view_start, V, sp.min_n, [&](int64_t v0, int64_t v1, int64_t k0, int64_t k1) -> int {
        SFM_TRY(out.download_rows(C, o_C, 3, v0, v1, s));
        SFM_TRY(out.download_rows(R, o_R, 9, v0, v1, s));
        SFM_TRY(out.download_rows(cost, o_cost, 1, v0, v1, s));
        SFM_TRY(out.download_rows(info, o_info, 1, v0, v1, s));
        SFM_TRY(out.download_rows(n_inliers, o_ninl, 1, v0, v1, s));
        SFM_TRY(out.download_rows(best_hyp, o_hyp, 1, v0, v1, s));
        SFM_TRY(out.download_rows(best_count, o_bc, 1, v0, v1, s));
        SFM_TRY(out.download_rows(inlier, o_mask, 1, k0, k1, s));
        SFM_TRY(out.download_rows(n_sol, o_ns, H, v0, v1, s));
        SFM_TRY(out.download_rows(counts, o_cnt, H * NS, v0, v1, s));
        return out.download_rows(models, o_mP, 12 * H * NS, v0, v1, s);
    }));
    return tm.finish(s);
}

}  // namespace sfm
