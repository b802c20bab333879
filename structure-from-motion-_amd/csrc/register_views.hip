// Batched view registration: which unregistered image to add next, and with
// what pose.  Every candidate view brings its 2D-3D correspondences (CSR over
// views) and a host-drawn table of 6-point samples; one call returns, per view,
// the RANSAC winner, the pose refitted to its consensus set and the inlier mask
// of the view's observations.  The reference registers one image per call from
// 4-point samples (PnPRANSAC.py: 8 equations for 12 unknowns, so the hypothesis
// is whatever null vector LAPACK returns); six points give 12 equations for the
// 11 degrees of freedom of P, a determined model.  Differs on purpose.
//
// The grid, the block table, the tile loop and the fixed-order sums are the
// scaffold's (hyp_batch.hpp).
//
//   k_reg_fit_score  Fit: a hypothesis belongs to 16 lanes, lane k < 12 holding
//                    row k of the 12 x 12 DLT system and row k of V; one-sided
//                    Jacobi rotates column pairs (the three column sums are
//                    16-lane butterflies), the column of smallest norm names
//                    the null vector, rv_post / pnp_projection finish the
//                    model.  Score: a wave per hypothesis, the inlier rule over
//                    tiles of 1024.
//   k_rv_refine<RvDlt6>  register_refine.hpp's: one workgroup per view, the
//                    winner (most inliers, then the earliest hypothesis), its
//                    mask and the refit from its pose.
//
// The inlier rule, the score loop, that kernel and the host driver of a call
// are register_refine.hpp's, shared with the calibrated 3-point entry point
// (register_p3p.hip); what is here is the fit.
#include "register_refine.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int RV_GROUP = 16;                       // lanes per hypothesis in the fit
constexpr int RV_FIT = RV_THREADS / RV_GROUP;      // hypotheses fitted per pass
constexpr int RV_HT = 64;                          // most hypotheses per workgroup
static_assert(RV_HT == 4 * RV_FIT, "a block of a long view takes one fit pass, RV_HT / 4");
constexpr int RV_SWEEPS = 60;

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

// Live views: n_v >= 6.  modelsP (V x H x 12) the hypothesis projections, modelsCR (V x H x 12) their
// C | R; counts (V x H), 0 for a model that is not finite.
__global__ void __launch_bounds__(RV_THREADS)
k_reg_fit_score(const double *__restrict__ Xg, const int64_t *__restrict__ view_start,
                const int32_t *__restrict__ pt_idx, const double2 *__restrict__ xy,
                const int32_t *__restrict__ samples, int32_t H, Cam3 K, Cam3, const int32_t *__restrict__ blk_start,
                const int32_t *__restrict__ tab, int32_t n_live, double thr, double *__restrict__ modelsP,
                double *__restrict__ modelsCR, int32_t *__restrict__ counts, int32_t *) {
    __shared__ double sP[RV_HT][12];
    __shared__ double sX[RV_TILE * 3];
    __shared__ double2 sxy[RV_TILE];
    __shared__ int32_t sFin[RV_HT], sCnt[RV_HT];
    const int tid = threadIdx.x;
    const HypTile t = tile_of_block(blk_start, tab, n_live, H);
    const int nh = t.nh;
    const int64_t vs = view_start[t.row];
    const int n = (int)(view_start[t.row + 1] - vs);
    const int64_t row0 = (int64_t)t.row * H + t.hb;

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

    // ---- score: a wave per finite hypothesis, the view's tile shared by all of them
    rv_score(Xg, pt_idx, xy, vs, n, thr, nh, [&](int hl, int &m) { return sFin[m = hl] != 0; }, sP, sCnt, sX, sxy);
    if (tid < nh) counts[row0 + tid] = sFin[tid] ? sCnt[tid] : 0;
}

// k_rv_refine's policy: one model a hypothesis, the earliest of equal counts;
// with every count 0, the earliest hypothesis whose P and C are finite.
struct RvDlt6 {
    static constexpr int SLOTS_PER_HYP = 1, MIN_N = 6;
    static constexpr bool COST_TIE_BREAK = false;
    static __device__ __forceinline__ bool usable(const double *modelsP, const double *modelsCR, const int32_t *, int64_t g) {
        const double *m = modelsP + g * 12, *mc = modelsCR + g * 12;
        bool fin = true;
        for (int j = 0; j < 12; ++j) fin &= isfinite(m[j]);
        for (int j = 0; j < 3; ++j) fin &= isfinite(mc[j]);
        return fin;
    }
};

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_register_views(const double *K, const double *X, int64_t n_pts, const int64_t *view_start,
                                  int64_t V, const int32_t *pt_idx, const double *xy, int64_t n_corr,
                                  const int32_t *samples, int64_t H, double threshold, int32_t min_inliers,
                                  int32_t refit_rounds, int32_t max_nfev, double *C, double *R, double *cost,
                                  int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                                  uint8_t *inlier, int32_t *counts, double *models, int device) {
    static const RvSpec spec{6, 6, 1, RV_HT, false, k_reg_fit_score, k_rv_refine<RvDlt6>,
                             "min_inliers must be at least 6", "V x H too large for one call"};
    return rv_run(spec, K, X, n_pts, view_start, V, pt_idx, xy, n_corr, samples, H, threshold, min_inliers, refit_rounds,
                  max_nfev, C, R, cost, n_inliers, best_hyp, best_count, info, inlier, nullptr, counts, models, device);
}
