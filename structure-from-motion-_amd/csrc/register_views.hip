// Batched view registration: which unregistered image to add next, and with
// what pose.  Every candidate view brings its 2D-3D correspondences (CSR over
// views) and a host-drawn table of 6-point samples; one call returns, per view,
// the RANSAC winner, the pose refitted to its consensus set and the inlier mask
// of the view's observations.  The reference registers one image per call from
// 4-point samples (PnPRANSAC.py: 8 equations for 12 unknowns, so the hypothesis
// is whatever null vector LAPACK returns); six points give 12 equations for the
// 11 degrees of freedom of P, a determined model.  Differs on purpose.
//
//   k_reg_fit_score  flat grid over (view, hypothesis tile) from a host prefix
//                    table.  Fit: a hypothesis belongs to 16 lanes, lane k < 12
//                    holding row k of the 12 x 12 DLT system and row k of V;
//                    one-sided Jacobi rotates column pairs (the three column
//                    sums are 16-lane butterflies), the column of smallest
//                    norm names the null vector, rv_post / pnp_projection
//                    finish the model.  Score: the view's correspondences are
//                    staged through LDS in tiles of 1024, a wave per hypothesis,
//                    ballot popcount of the inlier rule.
//   k_reg_refine     one workgroup per view: winner (most inliers, then the
//                    earliest), its mask, then rounds of Levenberg-Marquardt on
//                    the 6 pose parameters over the current inliers, a re-score
//                    of the whole view and the not-worse test.
//
// Every sum runs in a fixed order over quantities of the view alone (strided
// per-thread partial sums, a 64-lane butterfly, four wave results added as
// (0 + 1) + (2 + 3)); counts are integers.  A view's outputs therefore do not
// depend on the batch it is in.
#include <cmath>
#include <cstring>

#include "lm_small.hpp"
#include "staging.hpp"
#include "pnp_model.hpp"
#include "select.hpp"
#include "sfm_geom.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int RV_THREADS = 256;
constexpr int RV_WAVES = RV_THREADS / 64;
constexpr int RV_GROUP = 16;                       // lanes per hypothesis in the fit
constexpr int RV_FIT = RV_THREADS / RV_GROUP;      // hypotheses fitted per pass
constexpr int RV_HT = 64;                          // most hypotheses per workgroup
constexpr int RV_TILE = 1024;                      // correspondences per LDS tile
constexpr int RV_SWEEPS = 60;

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

__device__ __forceinline__ double rv_group_sum(double x) {
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 8);
    return x;
}

// One-sided Jacobi on the 12 x 12 system whose row k is M of lane k of the
// 16-lane group (zeros in lanes 12..15); Vr is row k of the accumulated
// rotations.  Every lane of a group sees the same sums, so the control flow
// is the group's.  Returns the null vector (V's column of the smallest
// column norm of M V, the first of equals) to every lane.
__device__ __forceinline__ void rv_null12(double (&M)[12], double (&Vr)[12], double (&p)[12]) {
    for (int sweep = 0; sweep < RV_SWEEPS; ++sweep) {
        bool any = false;
#pragma unroll
        for (int a = 0; a < 11; ++a) {
#pragma unroll
            for (int b = a + 1; b < 12; ++b) {
                const double al = rv_group_sum(M[a] * M[a]);
                const double be = rv_group_sum(M[b] * M[b]);
                const double ga = rv_group_sum(M[a] * M[b]);
                // |ga| / sqrt(al be) > 1e-15, squared; false for a NaN
                const bool rot = ga != 0.0 && ga * ga > 1e-30 * (al * be);
                any = any || rot;
                const double zeta = (be - al) / (2.0 * ga);
                const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c1 = 1.0 / sqrt(1.0 + tt * tt);
                const double cs = rot ? c1 : 1.0, sn = rot ? c1 * tt : 0.0;
                const double m1 = M[a], m2 = M[b], v1 = Vr[a], v2 = Vr[b];
                M[a] = rot ? cs * m1 - sn * m2 : m1;
                M[b] = rot ? sn * m1 + cs * m2 : m2;
                Vr[a] = rot ? cs * v1 - sn * v2 : v1;
                Vr[b] = rot ? sn * v1 + cs * v2 : v2;
            }
        }
        if (!any) break;
    }
    int best = 0;
    double bn = 0.0, vb = Vr[0];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const double s = rv_group_sum(M[j] * M[j]);
        if (j == 0 || s < bn) {
            bn = s;
            best = j;
            vb = Vr[j];
        }
    }
    (void)best;
#pragma unroll
    for (int k = 0; k < 12; ++k) p[k] = __shfl(vb, k, RV_GROUP);
}

// (C, R) from the null vector p = [M | t] ~ s [R | -R C].  pnp_post cannot serve
// here: it keeps LinearPnP.py:73-81's mean of a QR diagonal whose signs LAPACK
// mixes (-s, -s, +s for a camera near the identity), so its scale is s / 3 and
// its R a reflection that the det < 0 branch repairs by rounding noise.  This
// is the factorisation those lines intend: M = L R with L lower triangular and
// a positive diagonal, by Gram-Schmidt on M's rows after the sign that makes
// det M > 0; the third row is the cross product, so det R = +1; scale is the
// mean of L's diagonal.  B = [M | t] / scale with that sign.
__device__ __forceinline__ void rv_post(const double (&p)[12], double (&C)[3], double (&R)[9], double (&B)[12]) {
    double M[9] = {p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]};
    double t[3] = {p[3], p[7], p[11]};
    if (det3_d(M) < 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = -M[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = -t[k];
    }
    const double l00 = sqrt(M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) R[k] = M[k] / l00;
    const double l10 = M[3] * R[0] + M[4] * R[1] + M[5] * R[2];
    double b[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = M[3 + k] - l10 * R[k];
    const double l11 = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) R[3 + k] = b[k] / l11;
    R[6] = R[1] * R[5] - R[2] * R[4];
    R[7] = R[2] * R[3] - R[0] * R[5];
    R[8] = R[0] * R[4] - R[1] * R[3];
    const double l22 = M[6] * R[6] + M[7] * R[7] + M[8] * R[8];
    const double scale = ((l00 + l11) + l22) / 3.0;
    const double tn[3] = {t[0] / scale, t[1] / scale, t[2] / scale};
#pragma unroll
    for (int i = 0; i < 3; ++i) C[i] = -((R[i] * tn[0] + R[6 + i] * tn[2]) + R[3 + i] * tn[1]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) B[4 * r + c] = M[3 * r + c] / scale;
        B[4 * r + 3] = tn[r];
    }
}

// blk_start (n_live + 1): the first block of each live view (n_v >= 6);
// tab (n_live x 2): the view and the hypotheses per block chosen for it.
// modelsP (V x H x 12) the hypothesis projections, modelsCR (V x H x 12) their
// C | R; counts (V x H), 0 for a model that is not finite.
__global__ void __launch_bounds__(RV_THREADS)
k_reg_fit_score(const double *__restrict__ Xg, const int64_t *__restrict__ view_start,
                const int32_t *__restrict__ pt_idx, const double2 *__restrict__ xy,
                const int32_t *__restrict__ samples, int32_t H, Cam3 K, const int32_t *__restrict__ blk_start,
                const int32_t *__restrict__ tab, int32_t n_live, double thr, double *__restrict__ modelsP,
                double *__restrict__ modelsCR, int32_t *__restrict__ counts) {
    __shared__ double sP[RV_HT][12];
    __shared__ double sX[RV_TILE * 3];
    __shared__ double2 sxy[RV_TILE];
    __shared__ int32_t sFin[RV_HT], sCnt[RV_HT];
    const int tid = threadIdx.x;
    // the live view of this block: the last j with blk_start[j] <= blockIdx.x
    int lo = 0, hi = n_live - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk_start[mid] <= (int32_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int32_t v = tab[2 * lo], ht = tab[2 * lo + 1];
    const int32_t hb = ((int32_t)blockIdx.x - blk_start[lo]) * ht;
    const int nh = min(ht, H - hb);
    const int64_t vs = view_start[v];
    const int n = (int)(view_start[v + 1] - vs);
    const int64_t row0 = (int64_t)v * H + hb;

    // ---- fit: 16 hypotheses a pass, 16 lanes each
    const int k = tid & (RV_GROUP - 1);
    for (int pass = 0; pass * RV_FIT < nh; ++pass) {
        const int hl = pass * RV_FIT + (tid >> 4);
        const bool valid = hl < nh;
        double M[12], Vr[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) { M[j] = 0.0; Vr[j] = j == k ? 1.0 : 0.0; }
        if (valid && k < 12) {
            const int32_t s = samples[(row0 + hl) * 6 + (k >> 1)];
            const int64_t c = vs + s;
            const int64_t pi = pt_idx[c];
            const double2 q = xy[c];
            double xn, yn, r0[12], r1[12];
            pnp_xn(K, q.x, q.y, xn, yn);
            pnp_rows(Xg[3 * pi], Xg[3 * pi + 1], Xg[3 * pi + 2], xn, yn, r0, r1);
#pragma unroll
            for (int j = 0; j < 12; ++j) M[j] = (k & 1) ? r1[j] : r0[j];
        }
        // the hypothesis is scored under its own projection K [M | t] / scale,
        // the DLT's 11-parameter fit of its six points; (C, R) is the pose the
        // refit starts from
        double p[12], C[3], R[9], B[12], P[12];
        rv_null12(M, Vr, p);
        rv_post(p, C, R, B);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                P[r * 4 + c] = fma(K.k[r * 3 + 2], B[8 + c], fma(K.k[r * 3 + 1], B[4 + c], K.k[r * 3] * B[c]));
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 12; ++j) fin = fin && isfinite(P[j]);
#pragma unroll
        for (int j = 0; j < 3; ++j) fin = fin && isfinite(C[j]);
        if (valid && k == 0) {
            double *mp = modelsP + (row0 + hl) * 12, *mc = modelsCR + (row0 + hl) * 12;
#pragma unroll
            for (int j = 0; j < 12; ++j) { sP[hl][j] = P[j]; mp[j] = P[j]; }
#pragma unroll
            for (int j = 0; j < 3; ++j) mc[j] = C[j];
#pragma unroll
            for (int j = 0; j < 9; ++j) mc[3 + j] = R[j];
            sFin[hl] = fin ? 1 : 0;
            sCnt[hl] = 0;
        }
    }
    __syncthreads();

    // ---- score: a wave per hypothesis, the view's tile shared by all of them
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double thr2 = thr * thr;
    for (int base = 0; base < n; base += RV_TILE) {
        const int nt = min(RV_TILE, n - base);
        for (int i = tid; i < nt; i += RV_THREADS) {
            const int64_t c = vs + base + i;
            const int64_t pi = pt_idx[c];
            sX[3 * i] = Xg[3 * pi];
            sX[3 * i + 1] = Xg[3 * pi + 1];
            sX[3 * i + 2] = Xg[3 * pi + 2];
            sxy[i] = xy[c];
        }
        __syncthreads();
        for (int hl = wave; hl < nh; hl += RV_WAVES) {
            if (!sFin[hl]) continue;
            double P[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) P[j] = sP[hl][j];
            int cnt = 0;
            for (int j = 0; j < nt; j += 64) {
                const int i = j + lane;
                bool in = false;
                if (i < nt) {
                    const double2 q = sxy[i];
                    in = rv_inlier(P, sX[3 * i], sX[3 * i + 1], sX[3 * i + 2], q.x, q.y, thr, thr2);
                }
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) sCnt[hl] += cnt;  // this wave alone owns hl
        }
        __syncthreads();
    }
    if (tid < nh) counts[row0 + tid] = sFin[tid] ? sCnt[tid] : 0;
}

// ------------------------------------------------------------------ phase 2
// Fixed-order sum of NV values over the workgroup: a 64-lane butterfly (both
// partners add the same pair, so every lane holds the same bits), then the
// four wave results as (0 + 1) + (2 + 3).  red: RV_WAVES x NV.
template <int NV>
__device__ __forceinline__ void rv_wg_sum(double (&x)[NV], double (*red)[NV]) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1)
#pragma unroll
        for (int j = 0; j < NV; ++j) x[j] += __shfl_xor(x[j], w);
    __syncthreads();  // the last use of red is over
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) red[threadIdx.x >> 6][j] = x[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) x[j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
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
    rv_wg_sum<2>(acc, red);
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
    rv_wg_sum<RV_NV>(s, red);
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

// One workgroup per view.  mask2: scratch of n_corr bytes.  Views of fewer
// than six correspondences are the host's (info -1): nothing of them is read.
__global__ void __launch_bounds__(RV_THREADS)
k_reg_refine(const double *__restrict__ Xg, const int64_t *__restrict__ view_start,
             const int32_t *__restrict__ pt_idx, const double2 *__restrict__ xy, int32_t H, Cam3 K, double thr,
             int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, const double *__restrict__ modelsP,
             const double *__restrict__ modelsCR, const int32_t *__restrict__ counts, uint8_t *mask2,
             double *__restrict__ C_out, double *__restrict__ R_out, double *__restrict__ cost_out,
             int32_t *__restrict__ n_inl_out, int32_t *__restrict__ hyp_out, int32_t *__restrict__ count_out,
             int32_t *__restrict__ info_out, uint8_t *inlier) {
    __shared__ int32_t sc[RV_WAVES];
    __shared__ int64_t sh[RV_WAVES];
    __shared__ int32_t sFirst;
    __shared__ double red[RV_WAVES][RV_NV];
    __shared__ double red2[RV_WAVES][2];
    const int tid = threadIdx.x;
    const int64_t v = blockIdx.x;
    const int64_t vs = view_start[v];
    const int n = (int)(view_start[v + 1] - vs);
    if (n < 6) return;
    const RvView w{Xg, pt_idx + vs, xy + vs, n};
    uint8_t *mask = inlier + vs, *trial = mask2 + vs;
    const double thr2 = thr * thr;

    int32_t bc;
    int64_t bh;
    if (tid == 0) sFirst = H;
    wg_select_best<RV_THREADS>(counts + v * H, H, sc, sh, bc, bh);  // holds a barrier
    if (bh < 0) {  // every count is 0: the earliest finite hypothesis, if any
        for (int32_t h = tid; h < H; h += RV_THREADS) {
            const double *m = modelsP + (v * H + h) * 12, *mc = modelsCR + (v * H + h) * 12;
            bool fin = true;
            for (int j = 0; j < 12; ++j) fin = fin && isfinite(m[j]);
            for (int j = 0; j < 3; ++j) fin = fin && isfinite(mc[j]);
            if (fin) {
                atomicMin(&sFirst, h);
                break;
            }
        }
        __syncthreads();
        bh = sFirst < H ? sFirst : -1;
        bc = 0;
    }
    double C[3] = {0.0, 0.0, 0.0}, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, cost = 0.0;
    int info = -2, n_inl = 0;
    if (bh < 0) {
        for (int i = tid; i < n; i += RV_THREADS) mask[i] = 0;
    } else {
        double P[12];
        const double *m = modelsP + (v * H + bh) * 12, *mc = modelsCR + (v * H + bh) * 12;
#pragma unroll
        for (int j = 0; j < 12; ++j) P[j] = m[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) C[j] = mc[j];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = mc[3 + j];
        rv_mask(w, P, thr2, mask, n_inl, cost, red2);
        info = -3;
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
                // the refitted state replaces the current one only if it is not worse
                if (!(n2 > n_inl || (n2 == n_inl && cost2 <= cost))) break;
                int changed = 0;
                for (int i = tid; i < n; i += RV_THREADS) {
                    changed |= mask[i] != trial[i];
                    mask[i] = trial[i];
                }
                changed = __syncthreads_or(changed);
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = Rn[j];
#pragma unroll
                for (int j = 0; j < 3; ++j) C[j] = Cn[j];
                n_inl = n2;
                cost = cost2;
                if (!changed) break;
            }
        }
    }
    if (tid == 0) {
        for (int j = 0; j < 3; ++j) C_out[3 * v + j] = C[j];
        for (int j = 0; j < 9; ++j) R_out[9 * v + j] = R[j];
        cost_out[v] = cost;
        n_inl_out[v] = n_inl;
        hyp_out[v] = (int32_t)bh;
        count_out[v] = bh < 0 ? 0 : bc;
        info_out[v] = info;
    }
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_register_views(const double *K, const double *X, int64_t n_pts, const int64_t *view_start,
                                  int64_t V, const int32_t *pt_idx, const double *xy, int64_t n_corr,
                                  const int32_t *samples, int64_t H, double threshold, int32_t min_inliers,
                                  int32_t refit_rounds, int32_t max_nfev, double *C, double *R, double *cost,
                                  int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                                  uint8_t *inlier, int32_t *counts, double *models, int device) {
    SFM_CHECK_ARG(V >= 0 && n_corr >= 0 && n_pts >= 0, "V < 0, n_corr < 0 or n_pts < 0");
    SFM_CHECK_ARG(H >= 1 && H <= (int64_t)1 << 20, "H must lie in [1, 2^20]");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0, "threshold must be finite and positive");
    SFM_CHECK_ARG(min_inliers >= 6, "min_inliers must be at least 6");
    SFM_CHECK_ARG(refit_rounds >= 0, "refit_rounds < 0");
    SFM_CHECK_ARG(max_nfev > 0, "max_nfev must be positive");
    SFM_CHECK_ARG(V < (int64_t)0x7fffffff / H, "V x H too large for one call");
    SFM_CHECK_ARG(view_start && K, "null pointer");
    SFM_TRY(check_csr(view_start, V, n_corr, "view_start", "correspondence", 0x7fffffff,
                      "a view has too many correspondences"));
    int64_t n_live = 0;
    for (int64_t v = 0; v < V; ++v) n_live += view_start[v + 1] - view_start[v] >= 6;
    SFM_CHECK_ARG(n_corr == 0 || (pt_idx && xy && X), "null pointer");
    SFM_TRY(check_index(pt_idx, n_corr, n_pts, "point index outside [0, n_pts)"));
    SFM_CHECK_ARG(n_live == 0 || samples, "null pointer");
    for (int64_t v = 0; v < V; ++v) {
        const int64_t n = view_start[v + 1] - view_start[v];
        if (n < 6) continue;
        const int32_t *sv = samples + v * H * 6;
        for (int64_t h = 0; h < H; ++h) {
            const int32_t *s = sv + h * 6;
            for (int a = 0; a < 6; ++a) {
                SFM_CHECK_ARG(s[a] >= 0 && s[a] < n, "sample outside [0, n_v)");
                for (int b = 0; b < a; ++b) SFM_CHECK_ARG(s[a] != s[b], "a hypothesis repeats a sample");
            }
        }
    }
    if (V == 0) return 0;
    SFM_CHECK_ARG(C && R && cost && n_inliers && best_hyp && best_count && info && (inlier || n_corr == 0),
                  "null pointer");
    // info -1: fewer than six correspondences.  Also what the live views start from.
    for (int64_t v = 0; v < V; ++v) {
        if (view_start[v + 1] - view_start[v] >= 6) continue;
        for (int j = 0; j < 3; ++j) C[3 * v + j] = 0.0;
        for (int j = 0; j < 9; ++j) R[9 * v + j] = j % 4 == 0 ? 1.0 : 0.0;
        cost[v] = 0.0;
        n_inliers[v] = 0;
        best_hyp[v] = -1;
        best_count[v] = 0;
        info[v] = -1;
        for (int64_t k = view_start[v]; k < view_start[v + 1]; ++k) inlier[k] = 0;
        if (counts) std::memset(counts + v * H, 0, (size_t)H * sizeof(int32_t));
        if (models) std::memset(models + v * H * 12, 0, (size_t)H * 12 * sizeof(double));
    }
    if (n_live == 0) return 0;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    int rc;
    // block table: a view of many correspondences gets fewer hypotheses per
    // block, so that its score loop is spread over more of them
    if ((rc = c->pinned.reserve((size_t)(3 * n_live + 1) * sizeof(int32_t)))) return rc;
    int32_t *blk = c->pinned.as<int32_t>(), *tab = blk + (n_live + 1);
    int64_t blocks = 0, j = 0;
    for (int64_t v = 0; v < V; ++v) {
        const int64_t n = view_start[v + 1] - view_start[v];
        if (n < 6) continue;
        const int32_t ht = n >= 4 * RV_TILE ? RV_FIT : (n >= RV_TILE ? 2 * RV_FIT : RV_HT);
        blk[j] = (int32_t)blocks;
        tab[2 * j] = (int32_t)v;
        tab[2 * j + 1] = ht;
        blocks += (H + ht - 1) / ht;
        SFM_CHECK_ARG(blocks <= (int64_t)0x7fffffff, "too many hypothesis tiles for one launch");
        ++j;
    }
    blk[n_live] = (int32_t)blocks;

    const size_t VH = (size_t)V * (size_t)H;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_vs = in.add<int64_t>(V + 1);
    const auto i_xy = in.add<double2>(n_corr);
    const auto i_X = in.add<double>(3 * n_pts);
    const auto i_pt = in.add<int32_t>(n_corr), i_s = in.add<int32_t>(6 * VH);
    const auto i_t = in.add<int32_t>(3 * n_live + 1);  // the block table
    const auto o_C = out.add<double>(3 * V), o_R = out.add<double>(9 * V), o_cost = out.add<double>(V);
    const auto o_info = out.add<int32_t>(V), o_ninl = out.add<int32_t>(V);
    const auto o_hyp = out.add<int32_t>(V), o_bc = out.add<int32_t>(V), o_cnt = out.add<int32_t>(VH);
    const auto o_mP = out.add<double>(12 * VH), o_mCR = out.add<double>(12 * VH);
    const auto o_mask = out.add<uint8_t>(n_corr), o_m2 = out.add<uint8_t>(n_corr);  // o_m2: the refits' trial mask
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    Cam3 cam;
    std::memcpy(cam.k, K, sizeof cam.k);
    hipStream_t s = c->stream;
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_vs, view_start, s));
    SFM_TRY(in.upload(i_xy, xy, s));
    SFM_TRY(in.upload(i_X, X, s));
    SFM_TRY(in.upload(i_pt, pt_idx, s));
    SFM_TRY(in.upload(i_s, samples, s));
    SFM_TRY(in.upload(i_t, blk, s));
    SFM_TRY(tm.mark(s));
    hipLaunchKernelGGL(k_reg_fit_score, dim3((unsigned)blocks), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs),
                       in.ptr(i_pt), in.ptr(i_xy), in.ptr(i_s), (int32_t)H, cam, in.ptr(i_t),
                       in.ptr(i_t, n_live + 1), (int32_t)n_live, threshold, out.ptr(o_mP), out.ptr(o_mCR),
                       out.ptr(o_cnt));
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.split(s));  // [3]: the fit-and-score kernel alone
    hipLaunchKernelGGL(k_reg_refine, dim3((unsigned)V), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs),
                       in.ptr(i_pt), in.ptr(i_xy), (int32_t)H, cam, threshold, min_inliers, refit_rounds, max_nfev,
                       out.ptr(o_mP), out.ptr(o_mCR), out.ptr(o_cnt), out.ptr(o_m2), out.ptr(o_C), out.ptr(o_R),
                       out.ptr(o_cost), out.ptr(o_ninl), out.ptr(o_hyp), out.ptr(o_bc), out.ptr(o_info),
                       out.ptr(o_mask));
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    // live views are copied out one run of consecutive views at a time, so that
    // what the host wrote for the views of info -1 stays
    for (int64_t v0 = 0; v0 < V;) {
        if (view_start[v0 + 1] - view_start[v0] < 6) {
            ++v0;
            continue;
        }
        int64_t v1 = v0;
        while (v1 < V && view_start[v1 + 1] - view_start[v1] >= 6) ++v1;
        const size_t nv = (size_t)(v1 - v0);
        SFM_TRY(out.download(C + 3 * v0, o_C, 3 * v0, 3 * nv, s));
        SFM_TRY(out.download(R + 9 * v0, o_R, 9 * v0, 9 * nv, s));
        SFM_TRY(out.download(cost + v0, o_cost, v0, nv, s));
        SFM_TRY(out.download(info + v0, o_info, v0, nv, s));
        SFM_TRY(out.download(n_inliers + v0, o_ninl, v0, nv, s));
        SFM_TRY(out.download(best_hyp + v0, o_hyp, v0, nv, s));
        SFM_TRY(out.download(best_count + v0, o_bc, v0, nv, s));
        const int64_t k0 = view_start[v0], k1 = view_start[v1];
        SFM_TRY(out.download(inlier + k0, o_mask, k0, k1 - k0, s));
        if (counts) SFM_TRY(out.download(counts + v0 * H, o_cnt, v0 * H, nv * H, s));
        if (models) SFM_TRY(out.download(models + v0 * H * 12, o_mP, v0 * H * 12, nv * H * 12, s));
        v0 = v1;
    }
    return tm.finish(s);
}
