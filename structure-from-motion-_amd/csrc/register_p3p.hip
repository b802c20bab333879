// Calibrated batched view registration: sfm_register_views' question -- which
// image to add next, and with what pose -- answered with the calibration it is
// handed.  A hypothesis is a 3-point sample; p3p.hpp returns every pose (up to
// four) that puts the three points on their bearings K^-1 [x; 1], and each is
// scored as itself, P = K [R | -R C].  Three points instead of six per sample,
// a model for points on one plane (where the 12 x 12 DLT system has a
// four-dimensional null space), and no serial Jacobi.  The reference has no
// counterpart.
//
// The grid, the block table, the tile loop and the fixed-order sums are the
// scaffold's (hyp_batch.hpp).
//
//   k_p3p_fit_score  Solve: one lane per hypothesis, all of it in registers, no
//                    LDS and no shuffles; the poses go to LDS and global memory
//                    as they are found.  One thread then lists the slots that
//                    hold a solution.  Score: a wave per listed slot, the
//                    inlier rule over tiles of 1024 (rv_inlier: the fp64 band
//                    prefilter, rv_exact inside the band).  A hypothesis
//                    without solutions is never listed.
//   k_p3p_refine     one workgroup per view: the winner over (hypothesis,
//                    solution) -- most inliers, then the smaller sum of the
//                    inliers' squared errors, then the earlier slot -- and
//                    register_refine.hpp's refit from its pose.  The sums of
//                    the tie-break are rv_mask's, one pass over the view per
//                    slot that ties on the count.
#include <cmath>
#include <cstring>

#include "hyp_batch.hpp"
#include "p3p.hpp"
#include "register_refine.hpp"
#include "select.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int P3_HT = 32;               // most hypotheses per workgroup
constexpr int P3_SLOTS = P3_HT * P3P_MAX_SOL;

// Live views: n_v >= 4.  Per slot (V x H x 4): modelsP the projection (zeros past n_sol), modelsCR
// its C | R (written up to n_sol only), counts (0 past n_sol); n_sol (V x H).
__global__ void __launch_bounds__(RV_THREADS)
k_p3p_fit_score(const double *__restrict__ Xg, const int64_t *__restrict__ view_start,
                const int32_t *__restrict__ pt_idx, const double2 *__restrict__ xy,
                const int32_t *__restrict__ samples, int32_t H, Cam3 K, Cam3 Ki, const int32_t *__restrict__ blk_start,
                const int32_t *__restrict__ tab, int32_t n_live, double thr, double *__restrict__ modelsP,
                double *__restrict__ modelsCR, int32_t *__restrict__ counts, int32_t *__restrict__ n_sol) {
    __shared__ double sP[P3_SLOTS][12];
    __shared__ double sX[RV_TILE * 3];
    __shared__ double2 sxy[RV_TILE];
    __shared__ int32_t sNs[P3_HT], sCnt[P3_SLOTS], sList[P3_SLOTS], sLive;
    const int tid = threadIdx.x;
    const HypTile t = tile_of_block(blk_start, tab, n_live, H);
    const int nh = t.nh;
    const int64_t vs = view_start[t.row];
    const int n = (int)(view_start[t.row + 1] - vs);
    const int64_t row0 = (int64_t)t.row * H + t.hb;

    // ---- solve: one lane per hypothesis
    if (tid < P3_SLOTS) sCnt[tid] = 0;
    if (tid < nh) {
        double X[3][3], b[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int64_t c = vs + samples[(row0 + tid) * 3 + i];
            const int64_t pi = pt_idx[c];
            const double2 q = xy[c];
#pragma unroll
            for (int k = 0; k < 3; ++k) X[i][k] = Xg[3 * pi + k];
            const double r0 = (Ki.k[0] * q.x + Ki.k[1] * q.y) + Ki.k[2];
            const double r1 = (Ki.k[3] * q.x + Ki.k[4] * q.y) + Ki.k[5];
            const double r2 = (Ki.k[6] * q.x + Ki.k[7] * q.y) + Ki.k[8];
            const double nr = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
            b[i][0] = r0 / nr;
            b[i][1] = r1 / nr;
            b[i][2] = r2 / nr;
        }
        double *mp = modelsP + (row0 + tid) * (P3P_MAX_SOL * 12), *mc = modelsCR + (row0 + tid) * (P3P_MAX_SOL * 12);
        double(*sp)[12] = sP + tid * P3P_MAX_SOL;
        const int ns = p3p_solve(X, b, [&](int k, const double (&R)[9], const double (&C)[3]) {
            double P[12];
            pnp_projection(K, C, R, P);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                sp[k][j] = P[j];
                mp[12 * k + j] = P[j];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) mc[12 * k + j] = C[j];
#pragma unroll
            for (int j = 0; j < 9; ++j) mc[12 * k + 3 + j] = R[j];
        });
        for (int k = ns; k < P3P_MAX_SOL; ++k)
            for (int j = 0; j < 12; ++j) mp[12 * k + j] = 0.0;
        sNs[tid] = ns;
        n_sol[row0 + tid] = ns;
    }
    __syncthreads();
    if (tid == 0) {  // the slots that hold a solution, in order
        int m = 0;
        for (int hl = 0; hl < nh; ++hl)
            for (int k = 0; k < sNs[hl]; ++k) sList[m++] = hl * P3P_MAX_SOL + k;
        sLive = m;
    }
    __syncthreads();

    // ---- score: a wave per listed slot, the view's tile shared by all of them
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int live = sLive;
    const double thr2 = thr * thr;
    for_each_tile<RV_THREADS, RV_TILE>(
        n, [&](int i, int c) { rv_stage(Xg, pt_idx, xy, vs + c, sX, sxy, i); },
        [&](int nt) {
            for (int s = wave; s < live; s += RV_WAVES) {
                const int m = sList[s];
                double P[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) P[j] = sP[m][j];
                const int cnt = wave_count(nt, [&](int i) {
                    const double2 q = sxy[i];
                    return rv_inlier(P, sX[3 * i], sX[3 * i + 1], sX[3 * i + 2], q.x, q.y, thr, thr2);
                });
                if (lane == 0) sCnt[m] += cnt;  // this wave alone owns list entry s
            }
        });
    if (tid < nh * P3P_MAX_SOL) counts[row0 * P3P_MAX_SOL + tid] = sCnt[tid];
}

// One workgroup per view.  mask2: scratch of n_corr bytes.  Views of fewer
// than four correspondences are the host's (info -1): nothing of them is read.
__global__ void __launch_bounds__(RV_THREADS)
k_p3p_refine(const double *__restrict__ Xg, const int64_t *__restrict__ view_start,
             const int32_t *__restrict__ pt_idx, const double2 *__restrict__ xy, int32_t H, Cam3 K, double thr,
             int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, const double *__restrict__ modelsP,
             const double *__restrict__ modelsCR, const int32_t *__restrict__ counts,
             const int32_t *__restrict__ n_sol, uint8_t *mask2, double *__restrict__ C_out,
             double *__restrict__ R_out, double *__restrict__ cost_out, int32_t *__restrict__ n_inl_out,
             int32_t *__restrict__ hyp_out, int32_t *__restrict__ count_out, int32_t *__restrict__ info_out,
             uint8_t *inlier) {
    __shared__ int32_t sc[RV_WAVES];
    __shared__ int64_t sh[RV_WAVES];
    __shared__ int32_t sFirst;
    __shared__ double red[RV_WAVES][RV_NV];
    __shared__ double red2[RV_WAVES][2];
    const int tid = threadIdx.x;
    const int64_t v = blockIdx.x;
    const int64_t vs = view_start[v];
    const int n = (int)(view_start[v + 1] - vs);
    if (n < 4) return;
    const RvView w{Xg, pt_idx + vs, xy + vs, n};
    uint8_t *mask = inlier + vs, *trial = mask2 + vs;
    const double thr2 = thr * thr;
    const int32_t S = H * P3P_MAX_SOL;  // the view's slots
    const int32_t *cnt = counts + v * S;
    const double *mP = modelsP + v * S * 12, *mCR = modelsCR + v * S * 12;

    int32_t bc;
    int64_t bh;
    if (tid == 0) sFirst = S;
    wg_select_best<RV_THREADS>(cnt, S, sc, sh, bc, bh);  // holds a barrier
    if (bh < 0) {  // every count is 0: the earliest solution, if any
        for (int32_t h = tid; h < H; h += RV_THREADS)
            if (n_sol[v * H + h] > 0) {
                atomicMin(&sFirst, h * P3P_MAX_SOL);
                break;
            }
        __syncthreads();
        bh = sFirst < S ? sFirst : -1;
        bc = 0;
    } else {
        // the slots that tie on the count, in order: the smaller cost wins,
        // the earlier slot among equal costs
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
        hyp_out[v] = bh < 0 ? -1 : (int32_t)(bh / P3P_MAX_SOL);
        count_out[v] = bh < 0 ? 0 : bc;
        info_out[v] = info;
    }
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_register_views_p3p(const double *K, const double *X, int64_t n_pts, const int64_t *view_start,
                                      int64_t V, const int32_t *pt_idx, const double *xy, int64_t n_corr,
                                      const int32_t *samples, int64_t H, double threshold, int32_t min_inliers,
                                      int32_t refit_rounds, int32_t max_nfev, double *C, double *R, double *cost,
                                      int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                                      uint8_t *inlier, int32_t *n_sol, int32_t *counts, double *models, int device) {
    constexpr int64_t NS = P3P_MAX_SOL;
    SFM_CHECK_ARG(V >= 0 && n_corr >= 0 && n_pts >= 0, "V < 0, n_corr < 0 or n_pts < 0");
    SFM_CHECK_ARG(H >= 1 && H <= (int64_t)1 << 20, "H must lie in [1, 2^20]");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0, "threshold must be finite and positive");
    SFM_CHECK_ARG(min_inliers >= 4, "min_inliers must be at least 4");
    SFM_CHECK_ARG(refit_rounds >= 0, "refit_rounds < 0");
    SFM_CHECK_ARG(max_nfev > 0, "max_nfev must be positive");
    SFM_CHECK_ARG(V < (int64_t)0x7fffffff / (NS * H), "V x H x 4 too large for one call");
    SFM_CHECK_ARG(view_start && K, "null pointer");
    SFM_TRY(check_csr(view_start, V, n_corr, "view_start", "correspondence", 0x7fffffff,
                      "a view has too many correspondences"));
    const int64_t n_live = count_live(view_start, V, 4);
    SFM_CHECK_ARG(n_corr == 0 || (pt_idx && xy && X), "null pointer");
    SFM_TRY(check_index(pt_idx, n_corr, n_pts, "point index outside [0, n_pts)"));
    SFM_CHECK_ARG(n_live == 0 || samples, "null pointer");
    SFM_TRY(check_samples(view_start, V, samples, H, 3, 4, "sample outside [0, n_v)"));
    if (V == 0) return 0;
    SFM_CHECK_ARG(C && R && cost && n_inliers && best_hyp && best_count && info && (inlier || n_corr == 0),
                  "null pointer");
    // info -1: fewer than four correspondences.  Also what the live views start from.
    for (int64_t v = 0; v < V; ++v) {
        if (view_start[v + 1] - view_start[v] >= 4) continue;
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
    // every hypothesis brings up to four models, so a block takes a quarter to a
    // half of the hypotheses k_reg_fit_score gives it
    TileTable tt;
    SFM_TRY(tt.build(c->pinned, n_live, view_start, V, 4, H, P3_HT, RV_TILE));

    const size_t VH = (size_t)V * (size_t)H;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_vs = in.add<int64_t>(V + 1);
    const auto i_xy = in.add<double2>(n_corr);
    const auto i_X = in.add<double>(3 * n_pts);
    const auto i_pt = in.add<int32_t>(n_corr), i_s = in.add<int32_t>(3 * VH);
    const auto i_t = in.add<int32_t>(tt.words());  // the block table
    const auto o_C = out.add<double>(3 * V), o_R = out.add<double>(9 * V), o_cost = out.add<double>(V);
    const auto o_info = out.add<int32_t>(V), o_ninl = out.add<int32_t>(V);
    const auto o_hyp = out.add<int32_t>(V), o_bc = out.add<int32_t>(V), o_ns = out.add<int32_t>(VH);
    const auto o_cnt = out.add<int32_t>(NS * VH);
    const auto o_mP = out.add<double>(12 * NS * VH), o_mCR = out.add<double>(12 * NS * VH);
    const auto o_mask = out.add<uint8_t>(n_corr), o_m2 = out.add<uint8_t>(n_corr);  // o_m2: the refits' trial mask
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    Cam3 cam, cam_inv;
    std::memcpy(cam.k, K, sizeof cam.k);
    // a singular K gives bearings that are not finite, and with them hypotheses without solutions
    (void)inv3_adjugate(K, cam_inv.k);
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
    hipLaunchKernelGGL(k_p3p_fit_score, dim3((unsigned)tt.blocks), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs),
                       in.ptr(i_pt), in.ptr(i_xy), in.ptr(i_s), (int32_t)H, cam, cam_inv, in.ptr(i_t),
                       in.ptr(i_t, n_live + 1), (int32_t)n_live, threshold, out.ptr(o_mP), out.ptr(o_mCR),
                       out.ptr(o_cnt), out.ptr(o_ns));
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.split(s));  // [3]: the fit-and-score kernel alone
    hipLaunchKernelGGL(k_p3p_refine, dim3((unsigned)V), dim3(RV_THREADS), 0, s, in.ptr(i_X), in.ptr(i_vs),
                       in.ptr(i_pt), in.ptr(i_xy), (int32_t)H, cam, threshold, min_inliers, refit_rounds, max_nfev,
                       out.ptr(o_mP), out.ptr(o_mCR), out.ptr(o_cnt), out.ptr(o_ns), out.ptr(o_m2), out.ptr(o_C),
                       out.ptr(o_R), out.ptr(o_cost), out.ptr(o_ninl), out.ptr(o_hyp), out.ptr(o_bc),
                       out.ptr(o_info), out.ptr(o_mask));
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    SFM_TRY(for_each_live_run(view_start, V, 4, [&](int64_t v0, int64_t v1, int64_t k0, int64_t k1) -> int {
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
