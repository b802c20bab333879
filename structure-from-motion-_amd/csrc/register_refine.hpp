// What the two view-registration entry points share (register_views.hip:
// 6-point DLT hypotheses; register_p3p.hip: calibrated 3-point hypotheses):
// the inlier rule and its division-free prefilter, and the refit of a winning
// pose -- rounds of Levenberg-Marquardt on the 6 pose parameters over the
// current inliers, a re-score of the whole view and the not-worse test.  The
// fixed-order sums are the scaffold's (hyp_batch.hpp).
#pragma once
#include <cmath>

#include "hyp_batch.hpp"
#include "lm_small.hpp"
#include "pnp_model.hpp"
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

}  // namespace sfm
