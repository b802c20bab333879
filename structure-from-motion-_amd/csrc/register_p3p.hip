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
//   k_rv_refine<RvP3p>  register_refine.hpp's: one workgroup per view, the
//                    winner over (hypothesis, solution) -- most inliers, then
//                    the smaller sum of the inliers' squared errors, then the
//                    earlier slot -- and the refit from its pose.
//
// The inlier rule, the score loop, that kernel and the host driver of a call
// are register_refine.hpp's, shared with sfm_register_views; what is here is
// the solve.
#include "p3p.hpp"
#include "register_refine.hpp"

#pragma clang fp contract(off)

namespace sfm {

// most hypotheses per workgroup: every hypothesis brings up to four models, so a
// block takes a quarter to a half of the hypotheses k_reg_fit_score gives it
constexpr int P3_HT = 32;
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
    rv_score(Xg, pt_idx, xy, vs, n, thr, sLive, [&](int s, int &m) { return m = sList[s], true; }, sP, sCnt, sX, sxy);
    if (tid < nh * P3P_MAX_SOL) counts[row0 * P3P_MAX_SOL + tid] = sCnt[tid];
}

// k_rv_refine's policy: up to four models a hypothesis, the smaller cost among
// equal counts; with every count 0, the earliest hypothesis with a solution.
struct RvP3p {
    static constexpr int SLOTS_PER_HYP = P3P_MAX_SOL, MIN_N = 4;
    static constexpr bool COST_TIE_BREAK = true;
    static __device__ __forceinline__ bool usable(const double *, const double *, const int32_t *n_sol, int64_t g) {
        return n_sol[g] > 0;
    }
};

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_register_views_p3p(const double *K, const double *X, int64_t n_pts, const int64_t *view_start,
                                      int64_t V, const int32_t *pt_idx, const double *xy, int64_t n_corr,
                                      const int32_t *samples, int64_t H, double threshold, int32_t min_inliers,
                                      int32_t refit_rounds, int32_t max_nfev, double *C, double *R, double *cost,
                                      int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                                      uint8_t *inlier, int32_t *n_sol, int32_t *counts, double *models, int device) {
    static const RvSpec spec{3, 4, P3P_MAX_SOL, P3_HT, true, k_p3p_fit_score, k_rv_refine<RvP3p>,
                             "min_inliers must be at least 4", "V x H x 4 too large for one call"};
    return rv_run(spec, K, X, n_pts, view_start, V, pt_idx, xy, n_corr, samples, H, threshold, min_inliers, refit_rounds,
                  max_nfev, C, R, cost, n_inliers, best_hyp, best_count, info, inlier, n_sol, counts, models, device);
}
