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
//   k_reg_refine     one workgroup per view: winner (most inliers, then the
//                    earliest), its mask, then rounds of Levenberg-Marquardt on
//                    the 6 pose parameters over the current inliers, a re-score
//                    of the whole view and the not-worse test.
//
// The inlier rule, the fixed-order sums and the refit are register_refine.hpp's,
// shared with the calibrated 3-point entry point (register_p3p.hip).
#include <cmath>
#include <cstring>

#include "hyp_batch.hpp"
#include "register_refine.hpp"
#include "select.hpp"

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
                const int32_t *__restrict__ samples, int32_t H, Cam3 K, const int32_t *__restrict__ blk_start,
                const int32_t *__restrict__ tab, int32_t n_live, double thr, double *__restrict__ modelsP,
                double *__restrict__ modelsCR, int32_t *__restrict__ counts) {
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

    // ---- score: a wave per hypothesis, the view's tile shared by all of them
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double thr2 = thr * thr;
    for_each_tile<RV_THREADS, RV_TILE>(
        n, [&](int i, int c) { rv_stage(Xg, pt_idx, xy, vs + c, sX, sxy, i); },
        [&](int nt) {
            for (int hl = wave; hl < nh; hl += RV_WAVES) {
                if (!sFin[hl]) continue;
                double P[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) P[j] = sP[hl][j];
                const int cnt = wave_count(nt, [&](int i) {
                    const double2 q = sxy[i];
                    return rv_inlier(P, sX[3 * i], sX[3 * i + 1], sX[3 * i + 2], q.x, q.y, thr, thr2);
                });
                if (lane == 0) sCnt[hl] += cnt;  // this wave alone owns hl
            }
        });
    if (tid < nh) counts[row0 + tid] = sFin[tid] ? sCnt[tid] : 0;
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
        info = rv_refit(w, K, P, thr2, bc, min_inliers, refit_rounds, max_nfev, R, C, cost, n_inl, mask, trial, red,
                        red2);
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
    const int64_t n_live = count_live(view_start, V, 6);
    SFM_CHECK_ARG(n_corr == 0 || (pt_idx && xy && X), "null pointer");
    SFM_TRY(check_index(pt_idx, n_corr, n_pts, "point index outside [0, n_pts)"));
    SFM_CHECK_ARG(n_live == 0 || samples, "null pointer");
    SFM_TRY(check_samples(view_start, V, samples, H, 6, 6, "sample outside [0, n_v)"));
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
    TileTable tt;
    SFM_TRY(tt.build(c->pinned, n_live, view_start, V, 6, H, RV_HT, RV_TILE));

    const size_t VH = (size_t)V * (size_t)H;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_vs = in.add<int64_t>(V + 1);
    const auto i_xy = in.add<double2>(n_corr);
    const auto i_X = in.add<double>(3 * n_pts);
    const auto i_pt = in.add<int32_t>(n_corr), i_s = in.add<int32_t>(6 * VH);
    const auto i_t = in.add<int32_t>(tt.words());  // the block table
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
    SFM_TRY(in.upload(i_t, tt.blk, s));
    SFM_TRY(tm.mark(s));
    hipLaunchKernelGGL(k_reg_fit_score, dim3((unsigned)tt.blocks), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs),
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
    SFM_TRY(for_each_live_run(view_start, V, 6, [&](int64_t v0, int64_t v1, int64_t k0, int64_t k1) -> int {
        SFM_TRY(out.download_rows(C, o_C, 3, v0, v1, s));
        SFM_TRY(out.download_rows(R, o_R, 9, v0, v1, s));
        SFM_TRY(out.download_rows(cost, o_cost, 1, v0, v1, s));
        SFM_TRY(out.download_rows(info, o_info, 1, v0, v1, s));
        SFM_TRY(out.download_rows(n_inliers, o_ninl, 1, v0, v1, s));
        SFM_TRY(out.download_rows(best_hyp, o_hyp, 1, v0, v1, s));
        SFM_TRY(out.download_rows(best_count, o_bc, 1, v0, v1, s));
        SFM_TRY(out.download_rows(inlier, o_mask, 1, k0, k1, s));
        SFM_TRY(out.download_rows(counts, o_cnt, H, v0, v1, s));
        return out.download_rows(models, o_mP, 12 * H, v0, v1, s);
    }));
    return tm.finish(s);
}
