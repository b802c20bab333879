// Batched calibrated pair verification: the essential matrix of every image
// pair of a store in one call.  The calibrated member of the family of
// verify_pairs.hip: every pair brings its correspondences (CSR over pairs) and a
// host-drawn table of 5-point samples; one call returns, per pair, the RANSAC
// winner over all (hypothesis, solution) pairs, the pose E = [t]x R refitted to
// its consensus set by Levenberg-Marquardt and the inlier mask.  E and F = K^-T E
// K^-1 come out under verify_pairs' convention (x2^T F x1 = 0, unit norm, the
// Sampson distance in pixels), so F goes straight into sfm_init_pairs.  The
// reference has no counterpart.
//
// The grid, the block table and the fixed-order sums are the scaffold's
// (hyp_batch.hpp); k_ep_fit_score keeps the scaffold's device loops written out.
// The refit's round loop (epi_sampson.hpp) and the host side of a call
// (pair_verify.hpp) are shared with verify_pairs.hip.
//
//   k_ep_fit_score  Fit: one thread per hypothesis, four lanes of every wave at
//                   a time, the 10 x 20 constraint matrix in LDS
//                   (five_point.hpp).  Score: tiles of 1024 in the fit's
//                   workspace, reused; a wave per (hypothesis, solution), the
//                   inlier rule and a fixed-order sum of the inliers' squared
//                   distances; empty solution slots are skipped wave-uniformly.
//                   Per hypothesis the best solution (count, then cost, then
//                   the earliest) is written out.
//   k_ep_refit      one workgroup per pair: the winner (count, then cost, then
//                   the earliest hypothesis), its mask, then rounds of the
//                   five-parameter fit over the current inliers (per-thread
//                   partial sums of the 5 x 5 normal equations, a fixed-order
//                   tree, the solve by every thread on the same bits), a re-score
//                   of the whole pair and the not-worse test.
//
// No float atomics anywhere.
#include <cmath>
#include <cstring>

#include "five_point.hpp"
#include "pair_verify.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int EP_THREADS = 256;                 // fit and score
constexpr int EP_WAVES = EP_THREADS / 64;
constexpr int EP_LANES = 4;                     // lanes of a wave that fit at a time
constexpr int EP_FIT = EP_WAVES * EP_LANES;     // hypotheses fitted per pass
constexpr int EP_HT = 32;                       // most hypotheses per workgroup
constexpr int EP_TILE = 1024;                   // correspondences per LDS tile (32 KiB)
constexpr int EP_SMEM = EP_FIT * EP_WS > 4 * EP_TILE ? EP_FIT * EP_WS : 4 * EP_TILE;  // doubles
constexpr int EP_RT = 256;                      // refit
constexpr int EP_RW = EP_RT / 64;

// Live pairs: n_p >= 5.  Per hypothesis: n_sol; h_count, h_cost, h_E (9) of its
// best solution (h_count -1 without one).  counts (P x H x 10) and models
// (P x H x 10 x 9) may be null.
__global__ void __launch_bounds__(EP_THREADS)
k_ep_fit_score(const int64_t *__restrict__ pair_start, const double2 *__restrict__ x1,
               const double2 *__restrict__ x2, const int32_t *__restrict__ samples, int32_t H,
               const int32_t *__restrict__ blk_start, const int32_t *__restrict__ tab, int32_t n_live, EpK K,
               double thr, int32_t *__restrict__ n_sol, int32_t *__restrict__ h_count, double *__restrict__ h_cost,
               double *__restrict__ h_E, int32_t *__restrict__ counts, double *__restrict__ models) {
    __shared__ double smem[EP_SMEM];
    __shared__ double sE[EP_HT][EP_MAX_SOL][9];
    __shared__ double sCost[EP_HT][EP_MAX_SOL];
    __shared__ int32_t sCnt[EP_HT][EP_MAX_SOL], sN[EP_HT];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // tile_of_block, for_each_tile and wave_count written out here on purpose (the scaffold): keep
    // this text in step with hyp_batch.hpp
    int lo = 0, hi = n_live - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk_start[mid] <= (int32_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int32_t p = tab[2 * lo], ht = tab[2 * lo + 1];
    const int32_t hb = ((int32_t)blockIdx.x - blk_start[lo]) * ht;
    const int nh = min(ht, H - hb);
    const int64_t ps = pair_start[p];
    const int n = (int)(pair_start[p + 1] - ps);
    const int64_t row0 = (int64_t)p * H + hb;

    // ---- fit: 16 hypotheses a pass, one thread each
    if (lane < EP_LANES) {
        const int slot = wave * EP_LANES + lane;
        const EpWs<EP_FIT> w{smem + slot};
        for (int hl = slot; hl < nh; hl += EP_FIT) {
            double a[5], b[5], c[5], d[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int64_t k = ps + samples[(row0 + hl) * 5 + i];
                const double2 q1 = x1[k], q2 = x2[k];
                ep_normalise(K, q1.x, q1.y, a[i], b[i]);
                ep_normalise(K, q2.x, q2.y, c[i], d[i]);
            }
            sN[hl] = ep_solve(a, b, c, d, w, &sE[hl][0][0]);
            for (int s = 0; s < EP_MAX_SOL; ++s) {
                sCnt[hl][s] = 0;
                sCost[hl][s] = 0.0;
            }
        }
    }
    __syncthreads();  // the workspace is free: it becomes the tiles

    // ---- score: a wave per (hypothesis, solution), the pair's tile shared by all of them
    double2 *s1 = reinterpret_cast<double2 *>(smem), *s2 = s1 + EP_TILE;
    const double thr2 = thr * thr;
    for (int base = 0; base < n; base += EP_TILE) {
        const int nt = min(EP_TILE, n - base);
        for (int i = tid; i < nt; i += EP_THREADS) {
            s1[i] = x1[ps + base + i];
            s2[i] = x2[ps + base + i];
        }
        __syncthreads();
        for (int hl = wave; hl < nh; hl += EP_WAVES) {
            const int ns = __builtin_amdgcn_readfirstlane(sN[hl]);
            for (int s = 0; s < ns; ++s) {
                double E[9], F[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) E[j] = sE[hl][s][j];
                ep_F(K, E, F);
                int cnt = 0;
                double acc = 0.0;
                for (int j = 0; j < nt; j += 64) {
                    const int i = j + lane;
                    bool in = false;
                    if (i < nt) {
                        const double2 q1 = s1[i], q2 = s2[i];
                        double e2, den;
                        in = vp_inlier(F, q1.x, q1.y, q2.x, q2.y, thr2, e2, den);
                        if (in) acc += e2 / den;
                    }
                    cnt += __popcll(__ballot(in));
                }
                acc = wave_sum(acc);
                if (lane == 0) {  // this wave alone owns hl
                    sCnt[hl][s] += cnt;
                    sCost[hl][s] += acc;
                }
            }
        }
        __syncthreads();
    }

    // ---- the best solution of each hypothesis
    if (tid < nh) {
        const int ns = sN[tid];
        int bs = 0, bc = -1;
        double bcost = 0.0;
        for (int s = 0; s < ns; ++s) {
            const int c = sCnt[tid][s];
            const double co = sCost[tid][s];
            if (c > bc || (c == bc && co < bcost)) { bc = c; bcost = co; bs = s; }
        }
        n_sol[row0 + tid] = ns;
        h_count[row0 + tid] = bc;
        h_cost[row0 + tid] = bcost;
        for (int j = 0; j < 9; ++j) h_E[(row0 + tid) * 9 + j] = ns > 0 ? sE[tid][bs][j] : 0.0;
        if (counts)
            for (int s = 0; s < EP_MAX_SOL; ++s) counts[(row0 + tid) * EP_MAX_SOL + s] = s < ns ? sCnt[tid][s] : 0;
        if (models)
            for (int s = 0; s < EP_MAX_SOL; ++s)
                for (int j = 0; j < 9; ++j)
                    models[((row0 + tid) * EP_MAX_SOL + s) * 9 + j] = s < ns ? sE[tid][s][j] : 0.0;
    }
}

// ------------------------------------------------------------------ phase 2
// (count, cost, hypothesis): more inliers, then the smaller cost, then the earlier
__device__ __forceinline__ void ep_merge(int32_t &c1, double &s1, int32_t &h1, int32_t c2, double s2, int32_t h2) {
    if (c2 > c1 || (c2 == c1 && (s2 < s1 || (s2 == s1 && h2 < h1)))) {
        c1 = c2;
        s1 = s2;
        h1 = h2;
    }
}

// One workgroup per pair.  mask2: scratch of n_corr bytes.  Pairs of fewer than
// five correspondences are the host's (info -1): nothing of them is read.
__global__ void __launch_bounds__(EP_RT)
k_ep_refit(const int64_t *__restrict__ pair_start, const double2 *__restrict__ x1, const double2 *__restrict__ x2,
           int32_t H, EpK K, double thr, int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev,
           const int32_t *__restrict__ h_count, const double *__restrict__ h_cost, const double *__restrict__ h_E,
           uint8_t *mask2, double *__restrict__ E_out, double *__restrict__ F_out, double *__restrict__ cost_out,
           int32_t *__restrict__ n_inl_out, int32_t *__restrict__ hyp_out, int32_t *__restrict__ count_out,
           int32_t *__restrict__ info_out, uint8_t *inlier) {
    __shared__ int32_t sc[EP_RW], sh[EP_RW];
    __shared__ double ss[EP_RW];
    __shared__ double red[EP_RW][EP_NV];
    __shared__ double red2[EP_RW][2];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int64_t ps = pair_start[p];
    const int n = (int)(pair_start[p + 1] - ps);
    if (n < 5) return;
    const EpiPair w{x1 + ps, x2 + ps, n};
    uint8_t *mask = inlier + ps, *trial = mask2 + ps;
    const double thr2 = thr * thr;

    // ---- the winner over the hypotheses' best solutions
    int32_t bc = -1, bh = 0x7fffffff;
    double bs = 0.0;
    for (int32_t h = tid; h < H; h += EP_RT) {
        const int32_t c = h_count[p * H + h];
        if (c >= 0) ep_merge(bc, bs, bh, c, h_cost[p * H + h], h);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t c2 = __shfl_xor(bc, off), h2 = __shfl_xor(bh, off);
        const double s2 = __shfl_xor(bs, off);
        ep_merge(bc, bs, bh, c2, s2, h2);
    }
    if ((tid & 63) == 0) { sc[tid >> 6] = bc; ss[tid >> 6] = bs; sh[tid >> 6] = bh; }
    __syncthreads();
    bc = sc[0]; bs = ss[0]; bh = sh[0];
#pragma unroll
    for (int k = 1; k < EP_RW; ++k) ep_merge(bc, bs, bh, sc[k], ss[k], sh[k]);

    double E[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double cost = 0.0;
    int info = -2, n_inl = 0;
    if (bc >= 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) E[j] = h_E[(p * H + bh) * 9 + j];
        ep_F(K, E, F);
        epi_mask<EP_RT>(w, F, thr2, mask, n_inl, cost, red2);
        info = -3;
        if (bc >= min_inliers) {
            info = 0;
            // the sums of the normal equations over the current inliers; every thread gets the same bits
            const auto eval = [&](const double (&R)[9], const double (&t)[3], double (&A)[15], double (&g)[5],
                                  double &c) {
                EpModel m;
                ep_model(K, R, t, m);
                double s[EP_NV];
#pragma unroll
                for (int j = 0; j < EP_NV; ++j) s[j] = 0.0;
                for (int i = tid; i < n; i += EP_RT) {
                    if (!mask[i]) continue;
                    const double2 q1 = w.x1[i], q2 = w.x2[i];
                    ep_accum(m, q1.x, q1.y, q2.x, q2.y, s);
                }
                wg_sum<EP_RW, EP_NV>(s, red);
#pragma unroll
                for (int j = 0; j < 15; ++j) A[j] = s[j];
#pragma unroll
                for (int j = 0; j < 5; ++j) g[j] = s[15 + j];
                c = s[21] > 0.0 ? INFINITY : s[20];
            };
            // a round: E = [t]x R from Levenberg-Marquardt on the factors of the current E; info is its
            // last code, or -4 where E does not factor
            double En[9];
            epi_refit_rounds<EP_RT>(
                w, thr2, F, n_inl, cost, mask, trial, refit_rounds, red2,
                [&](const uint8_t *, int, double (&Fn)[9]) {
                    double R[9], t[3], G[9];
                    if (!ep_factor(E, R, t)) {
                        info = -4;
                        return false;
                    }
                    info = ep_lm(eval, R, t, max_nfev);
                    if (info < 0) return false;
                    ep_cross_mat(t, R, G);
                    vp_unit(G, En);
                    ep_F(K, En, Fn);
                    return true;
                },
                [&] {
#pragma unroll
                    for (int j = 0; j < 9; ++j) E[j] = En[j];
                });
        }
    }
    if (tid == 0)
        for (int j = 0; j < 9; ++j) {
            E_out[9 * p + j] = E[j];
            F_out[9 * p + j] = F[j];
        }
    epi_store_pair<EP_RT>(p, n, mask, bc < 0 ? -1 : bh, bc, cost, n_inl, info, cost_out, n_inl_out, hyp_out, count_out,
                          info_out);
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_essential_pairs(const double *K, const int64_t *pair_start, int64_t P, const double *x1,
                                   const double *x2, int64_t n_corr, const int32_t *samples, int64_t H,
                                   double threshold, int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev,
                                   double *E, double *F, double *cost, int32_t *n_inliers, int32_t *best_hyp,
                                   int32_t *best_count, int32_t *info, uint8_t *inlier, int32_t *n_sol,
                                   int32_t *counts, double *models, int device) {
    static const PairSpec spec{5, 5, EP_MAX_SOL, EP_HT, EP_TILE, true, "min_inliers must be at least 5"};
    Slot<int32_t> o_ns, o_hc, o_cnt;
    Slot<double> o_hs, o_hE, o_m;
    EpK Ki{};
    if (K) (void)inv3_adjugate(K, Ki.ki);  // pair_run checks K and this inverse before a kernel reads it
    return pair_run(
        spec, K, pair_start, P, x1, x2, n_corr, samples, H, threshold, min_inliers, refit_rounds, max_nfev, E, F, cost,
        n_inliers, best_hyp, best_count, info, inlier, n_sol, counts, models, device,
        [&](Pack &out, size_t PH) {
            o_ns = out.add<int32_t>(PH), o_hc = out.add<int32_t>(PH);
            o_hs = out.add<double>(PH), o_hE = out.add<double>(9 * PH);
            // the per-solution tables exist on the device only when they are asked for
            o_cnt = out.add<int32_t>(counts ? EP_MAX_SOL * PH : 0);
            o_m = out.add<double>(models ? 9 * EP_MAX_SOL * PH : 0);
        },
        [&](const PairCall &c, int refit) {
            if (!refit)
                hipLaunchKernelGGL(k_ep_fit_score, dim3((unsigned)c.blocks), dim3(EP_THREADS), 0, c.s, c.ps, c.x1, c.x2,
                                   c.samples, (int32_t)c.H, c.blk_start, c.tab, (int32_t)c.n_live, Ki, c.threshold,
                                   c.out.ptr(o_ns), c.out.ptr(o_hc), c.out.ptr(o_hs), c.out.ptr(o_hE),
                                   counts ? c.out.ptr(o_cnt) : nullptr, models ? c.out.ptr(o_m) : nullptr);
            else
                hipLaunchKernelGGL(k_ep_refit, dim3((unsigned)c.P), dim3(EP_RT), 0, c.s, c.ps, c.x1, c.x2, (int32_t)c.H,
                                   Ki, c.threshold, c.min_inliers, c.refit_rounds, c.max_nfev, c.out.ptr(o_hc),
                                   c.out.ptr(o_hs), c.out.ptr(o_hE), c.mask2, c.E, c.F, c.cost, c.n_inl, c.hyp, c.count,
                                   c.info, c.mask);
        },
        [&](const PairCall &c, int64_t p0, int64_t p1) -> int {
            const size_t S = (size_t)c.H * EP_MAX_SOL;
            SFM_TRY(c.out.download_rows(n_sol, o_ns, c.H, p0, p1, c.s));
            SFM_TRY(c.out.download_rows(counts, o_cnt, S, p0, p1, c.s));
            return c.out.download_rows(models, o_m, 9 * S, p0, p1, c.s);
        });
}
