// The per-track bodies shared by k_triangulate_tracks (multiview.hip) and
// k_triangulate_tracks_robust (robust_tracks.hip): the streamed Givens DLT,
// the cost / normal-equation stream and the Levenberg-Marquardt on it.  Every
// stream takes a predicate keep(k) on the observation's index; an observation
// it rejects is skipped as if the track did not hold it, so a track streamed
// under a mask returns the bits of the same track with those rows removed.
//
// Include after triangulate_point.hpp and lm_small.hpp (see multiview.hip).
#pragma once
#include "sfm_common.hpp"
#include "sfm_geom.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int MV_LDS_CAMS = SFM_TRACKS_LDS_CAMS;
// LDS row stride in doubles.  A lane reads its camera's row with six
// ds_read_b128; that instruction serves 16 lanes per cycle over 64 banks of
// 4 B.  With 14 doubles (112 B = 28 banks) a row starts on bank 28 c mod 64,
// a multiple of 4 that takes 16 values: the 16-B reads of any 16 consecutive
// cameras fall on disjoint banks, cameras 16 apart share them, and lanes on
// the same camera broadcast.  The dense stride 12 (24 banks) repeats after 8.
constexpr int MV_ROW = 14;

template <bool LDS>
__device__ __forceinline__ const double *mv_row(const double *base, int cam) {
    return LDS ? base + cam * MV_ROW : base + (int64_t)cam * 12;
}

// keep every observation of the track
struct MvAll {
    __device__ __forceinline__ bool operator()(int64_t) const { return true; }
};

// keep the observations whose byte in a per-observation mask is set
struct MvMask {
    const uint8_t *m;
    __device__ __forceinline__ bool operator()(int64_t k) const { return m[k] != 0; }
};

// One Givens step of the streamed QR: row a (4 entries) is rotated into the
// upper triangle r = (r00 r01 r02 r03 | r11 r12 r13 | r22 r23 | r33).
__device__ __forceinline__ void givens_row(double (&r)[10], double (&a)[4]) {
    constexpr int D[4] = {0, 4, 7, 9};  // index of r_ii
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (a[i] != 0.0) {
            const double rii = r[D[i]];
            const double h = sqrt(rii * rii + a[i] * a[i]);
            const double c = rii / h, s = a[i] / h;
            r[D[i]] = h;
#pragma unroll
            for (int j = i + 1; j < 4; ++j) {
                const double rij = r[D[i] + j - i], aj = a[j];
                r[D[i] + j - i] = c * rij + s * aj;
                a[j] = c * aj - s * rij;
            }
        }
    }
}

// The N-view DLT of the kept observations: two rows per view streamed
// through Givens rotations into a 4 x 4 triangle, one-sided Jacobi on it, the
// weakest column's right singular vector, dehomogenised where |h3| > 1e-8.
template <bool LDS, class Keep>
__device__ __forceinline__ void mv_dlt(const double *Pb, const int32_t *__restrict__ cam,
                                       const double2 *__restrict__ xy, int64_t s, int64_t e, const Keep &keep,
                                       double (&x)[3]) {
    double r[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) r[k] = 0.0;
    for (int64_t k = s; k < e; ++k) {
        if (!keep(k)) continue;
        const double *P = mv_row<LDS>(Pb, cam[k]);
        const double2 o = xy[k];
        double a[4], b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = o.y * P[8 + c] - P[4 + c];
            b[c] = P[c] - o.x * P[8 + c];
        }
        givens_row(r, a);
        givens_row(r, b);
    }
    double a[4][4], V[4][4];  // a[col][row]
    a[0][0] = r[0]; a[0][1] = 0.0;  a[0][2] = 0.0;  a[0][3] = 0.0;
    a[1][0] = r[1]; a[1][1] = r[4]; a[1][2] = 0.0;  a[1][3] = 0.0;
    a[2][0] = r[2]; a[2][1] = r[5]; a[2][2] = r[7]; a[2][3] = 0.0;
    a[3][0] = r[3]; a[3][1] = r[6]; a[3][2] = r[8]; a[3][3] = r[9];
    jacobi_onesided<4, 4, 40>(a, V);
    const int j = weakest_column<4, 4>(a);
    const double h0 = V[0][j], h1 = V[1][j], h2 = V[2][j], h3 = V[3][j];
    if (fabs(h3) > 1e-8) {
        x[0] = h0 / h3; x[1] = h1 / h3; x[2] = h2 / h3;
    } else {
        x[0] = h0; x[1] = h1; x[2] = h2;
    }
}

// The kept observations' cost at X (sum of squared residuals u - h0/h2,
// v - h1/h2; a view with |h2| < 1e-8 contributes none), whether X lies in
// front of every kept camera (h2 > 0), and with JAC the normal equations:
// A = J^T J as (00 01 02 11 12 22), g = J^T r.  h is summed as NlTriLoss sums
// it.  The cost is the same sequence of IEEE operations with and without JAC.
template <bool LDS, bool JAC, class Keep>
__device__ __forceinline__ void mv_stream(const double *Pb, const int32_t *__restrict__ cam,
                                          const double2 *__restrict__ xy, int64_t s, int64_t e, const Keep &keep,
                                          const double (&X)[3], double &cost, bool &front, double (&A)[6],
                                          double (&g)[3]) {
    cost = 0.0;
    front = true;
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = 0.0;
        g[0] = g[1] = g[2] = 0.0;
    }
    for (int64_t k = s; k < e; ++k) {
        if (!keep(k)) continue;
        const double *P = mv_row<LDS>(Pb, cam[k]);
        const double2 o = xy[k];
        const double h0 = (P[0] * X[0] + P[2] * X[2]) + (P[1] * X[1] + P[3]);
        const double h1 = (P[4] * X[0] + P[6] * X[2]) + (P[5] * X[1] + P[7]);
        const double h2 = (P[8] * X[0] + P[10] * X[2]) + (P[9] * X[1] + P[11]);
        front = front && h2 > 0.0;
        if (!(fabs(h2) < 1e-8)) {
            const double px = h0 / h2, py = h1 / h2;
            const double ru = o.x - px, rv = o.y - py;
            cost += ru * ru + rv * rv;
            if (JAC) {
                const double inv = 1.0 / h2;
                double ju[3], jv[3];  // d ru / dX, d rv / dX
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    ju[j] = (px * P[8 + j] - P[j]) * inv;
                    jv[j] = (py * P[8 + j] - P[4 + j]) * inv;
                    g[j] += ju[j] * ru + jv[j] * rv;
                }
                A[0] += ju[0] * ju[0] + jv[0] * jv[0];
                A[1] += ju[0] * ju[1] + jv[0] * jv[1];
                A[2] += ju[0] * ju[2] + jv[0] * jv[2];
                A[3] += ju[1] * ju[1] + jv[1] * jv[1];
                A[4] += ju[1] * ju[2] + jv[1] * jv[2];
                A[5] += ju[2] * ju[2] + jv[2] * jv[2];
            }
        }
    }
}

// (A + lam diag(A)) d = -g by LDL^T in registers; false where the damped
// matrix is not positive definite (or holds a NaN).
__device__ __forceinline__ bool mv_solve3(const double (&A)[6], const double (&g)[3], double lam, double (&d)[3]) {
    const double m00 = A[0] + lam * A[0], m11 = A[3] + lam * A[3], m22 = A[5] + lam * A[5];
    const double d0 = m00;
    if (!(d0 > 0.0)) return false;
    const double l10 = A[1] / d0, l20 = A[2] / d0;
    const double d1 = m11 - l10 * A[1];
    if (!(d1 > 0.0)) return false;
    const double t = A[4] - l20 * A[1];
    const double l21 = t / d1;
    const double d2 = m22 - l20 * A[2] - l21 * t;
    if (!(d2 > 0.0)) return false;
    const double y0 = -g[0];
    const double y1 = -g[1] - l10 * y0;
    const double y2 = -g[2] - l20 * y0 - l21 * y1;
    d[2] = y2 / d2;
    d[1] = y1 / d1 - l21 * d[2];
    d[0] = y0 / d0 - l10 * d[1] - l20 * d[2];
    return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

// Levenberg-Marquardt over all 2n residuals of three or more kept views
// (Marquardt's scaling, lambda 1e-3, /10 on an accepted step, x10 on a
// rejected one).  A step is accepted only where it lowers the cost.  The stop
// tests are MINPACK's with the reference's ftol = xtol = gtol = 1e-8 on this
// iteration's own quantities, and so are the codes: 1 the actual and the
// predicted relative reductions are both at most ftol, 2 the step is at most
// xtol |x|, 3 both, 4 the cosine between the residual and every Jacobian
// column is at most gtol, 5 max_nfev cost evaluations.  Returns -1 (x kept)
// where the cost at x is not finite.
template <bool LDS, class Keep>
__device__ __forceinline__ int mv_refine(const double *Pb, const int32_t *__restrict__ cam,
                                         const double2 *__restrict__ xy, int64_t s, int64_t e, const Keep &keep,
                                         double (&x)[3], int max_nfev, double &cost, bool &front) {
    const double tol = 1e-8;
    double A[6], g[3], c0;
    bool fr;
    mv_stream<LDS, true>(Pb, cam, xy, s, e, keep, x, c0, fr, A, g);
    cost = c0;
    front = fr;
    if (!isfinite(c0)) return -1;
    int nfev = 1, info = 0;
    double lam = 1e-3;
    while (info == 0) {
        double gn = 0.0;
        if (c0 != 0.0) {
            const double fn = sqrt(c0);
            if (A[0] > 0.0) gn = fmax(gn, fabs(g[0]) / (sqrt(A[0]) * fn));
            if (A[3] > 0.0) gn = fmax(gn, fabs(g[1]) / (sqrt(A[3]) * fn));
            if (A[5] > 0.0) gn = fmax(gn, fabs(g[2]) / (sqrt(A[5]) * fn));
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
            double d[3];
            if (!mv_solve3(A, g, lam, d)) {
                lam *= 10.0;
                continue;
            }
            double xt[3] = {x[0] + d[0], x[1] + d[1], x[2] + d[2]};
            double A1[6], g1[3], c1;
            bool fr1;
            mv_stream<LDS, true>(Pb, cam, xy, s, e, keep, xt, c1, fr1, A1, g1);
            // the linear model's reduction |r|^2 - |r + J d|^2
            const double Ad0 = A[0] * d[0] + A[1] * d[1] + A[2] * d[2];
            const double Ad1 = A[1] * d[0] + A[3] * d[1] + A[4] * d[2];
            const double Ad2 = A[2] * d[0] + A[4] * d[1] + A[5] * d[2];
            const double prered =
                -(2.0 * (g[0] * d[0] + g[1] * d[1] + g[2] * d[2]) + (d[0] * Ad0 + d[1] * Ad1 + d[2] * Ad2)) / c0;
            const double actred = 1.0 - c1 / c0;
            const double pnorm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (c1 < c0) {
                x[0] = xt[0]; x[1] = xt[1]; x[2] = xt[2];
                c0 = c1;
                fr = fr1;
#pragma unroll
                for (int k = 0; k < 6; ++k) A[k] = A1[k];
                g[0] = g1[0]; g[1] = g1[1]; g[2] = g1[2];
                lam = fmax(lam * 0.1, 1e-15);
                accepted = true;
            } else {
                lam *= 10.0;
            }
            const double xnorm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            const bool fhit = fabs(actred) <= tol && prered <= tol && 0.5 * actred <= prered;
            const bool xhit = pnorm <= tol * xnorm;
            if (fhit) info = 1;
            if (xhit) info = fhit ? 3 : 2;
        }
    }
    cost = c0;
    front = fr;
    return info;
}

}  // namespace sfm
