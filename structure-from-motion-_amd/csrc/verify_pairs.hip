// Batched pair verification: the epipolar geometry of every image pair of a
// store in one call.  Every pair brings its correspondences (CSR over pairs)
// and a host-drawn table of 8-point samples; one call returns, per pair, the
// RANSAC winner, the fundamental matrix refitted to its consensus set and the
// inlier mask of the pair's correspondences -- the flags every later stage of
// the pipeline reads.  The reference verifies one pair per call
// (Wrapper_dev.py:69-123) with a design row for x1^T F x2 = 0 under a
// denormalisation and a score for x2^T F x1 = 0; the drop-ins keep that bit for
// bit.  This entry point uses x2^T F x1 = 0 throughout, a unit-norm model and
// the Sampson distance (epi_sampson.hpp).  Differs on purpose.
//
// The grid, the block table, the tile loop and the fixed-order sums are the
// scaffold's (hyp_batch.hpp), the refit's round loop epi_sampson.hpp's and the
// host side of a call pair_verify.hpp's, both shared with essential_pairs.hip.
//
//   k_vp_fit_score  Fit: a hypothesis belongs to 8 lanes, one design row each
//                   (vp_fit_group8).  Score: a wave per hypothesis, the inlier
//                   rule over tiles of 1024.
//   k_vp_refit      one workgroup per pair: winner (most inliers, then the
//                   earliest), its mask, then rounds of the normalised
//                   least-squares fit over the current inliers (Hartley sums,
//                   per-thread Givens QR of the N x 9 design, a tree merge of
//                   the 9 x 9 factors in LDS, one lane's 9-column Jacobi), a
//                   re-score of the whole pair and the not-worse test.
//
// The factors merge along a fixed tree, so a pair's outputs do not depend on
// the batch it is in.
#include <cmath>
#include <cstring>

#include "dlt_general.hpp"
#include "epi_sampson.hpp"
#include "pair_verify.hpp"
#include "select.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int VP_THREADS = 256;                // fit and score
constexpr int VP_WAVES = VP_THREADS / 64;
constexpr int VP_FIT = VP_THREADS / 8;         // hypotheses fitted per pass
constexpr int VP_HT = 64;                      // most hypotheses per workgroup
constexpr int VP_TILE = 1024;                  // correspondences per LDS tile (32 KiB)
constexpr int VP_RT = FG_THREADS;              // refit: 128 threads of 45 doubles, 45 KiB of LDS
constexpr int VP_RW = VP_RT / 64;

// Live pairs: n_p >= 8.  models (P x H x 9); counts (P x H), 0 for a model that
// is not finite.
__global__ void __launch_bounds__(VP_THREADS)
k_vp_fit_score(const int64_t *__restrict__ pair_start, const double2 *__restrict__ x1,
               const double2 *__restrict__ x2, const int32_t *__restrict__ samples, int32_t H,
               const int32_t *__restrict__ blk_start, const int32_t *__restrict__ tab, int32_t n_live, double thr,
               double *__restrict__ models, int32_t *__restrict__ counts) {
    __shared__ double sF[VP_HT][9];
    __shared__ double2 s1[VP_TILE];
    __shared__ double2 s2[VP_TILE];
    __shared__ int32_t sFin[VP_HT], sCnt[VP_HT];
    const int tid = threadIdx.x;
    const HypTile t = tile_of_block(blk_start, tab, n_live, H);
    const int nh = t.nh;
    const int64_t ps = pair_start[t.row];
    const int n = (int)(pair_start[t.row + 1] - ps);
    const int64_t row0 = (int64_t)t.row * H + t.hb;

    // ---- fit: 32 hypotheses a pass, 8 lanes each
    const int k = tid & 7;
    for (int pass = 0; pass * VP_FIT < nh; ++pass) {
        const int hl = pass * VP_FIT + (tid >> 3);
        const bool valid = hl < nh;  // the same for the 8 lanes of a group
        double2 a = make_double2(0.0, 0.0), b = a;
        if (valid) {
            const int64_t c = ps + samples[(row0 + hl) * 8 + k];
            a = x1[c];
            b = x2[c];
        }
        double F[9];
        vp_fit_group8(a.x, a.y, b.x, b.y, F);
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) fin = fin && isfinite(F[j]);
        if (valid) {
            double fk = F[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) fk = k == j ? F[j] : fk;
            sF[hl][k] = fk;
            models[(row0 + hl) * 9 + k] = fk;
            if (k == 0) {
                sF[hl][8] = F[8];
                models[(row0 + hl) * 9 + 8] = F[8];
                sFin[hl] = fin ? 1 : 0;
                sCnt[hl] = 0;
            }
        }
    }
    __syncthreads();

    // ---- score: a wave per hypothesis, the pair's tile shared by all of them
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double thr2 = thr * thr;
    for_each_tile<VP_THREADS, VP_TILE>(
        n, [&](int i, int c) { s1[i] = x1[ps + c], s2[i] = x2[ps + c]; },
        [&](int nt) {
            for (int hl = wave; hl < nh; hl += VP_WAVES) {
                if (!sFin[hl]) continue;
                double F[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) F[j] = sF[hl][j];
                const int cnt = wave_count(nt, [&](int i) {
                    const double2 q1 = s1[i], q2 = s2[i];
                    double e2, den;
                    return vp_inlier(F, q1.x, q1.y, q2.x, q2.y, thr2, e2, den);
                });
                if (lane == 0) sCnt[hl] += cnt;  // this wave alone owns hl
            }
        });
    if (tid < nh) counts[row0 + tid] = sFin[tid] ? sCnt[tid] : 0;
}

// ------------------------------------------------------------------ phase 2
// jacobi_onesided<9, 9, 40> and weakest_column on a matrix in LDS, for one
// lane: a[9 j + i] is column j, row i; V (9 x 9, row-major) accumulates the
// rotations.  The same rotation rule, threshold and sweep cap; held in
// registers, the two matrices alone are 324 VGPRs and the kernel spills.
// Returns the column of the smallest norm (the first of equals).
__device__ __forceinline__ int vp_jacobi9(double *a, double *V) {
    for (int i = 0; i < 81; ++i) V[i] = i % 10 == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 8; ++p) {
            double x[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) x[k] = a[9 * p + k];
            for (int q = p + 1; q < 9; ++q) {
                double y[9];
                double al = 0, be = 0, ga = 0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    y[k] = a[9 * q + k];
                    al += x[k] * x[k];
                    be += y[k] * y[k];
                    ga += x[k] * y[k];
                }
                const double r = fabs(ga) / sqrt(al * be);
                if (ga != 0.0 && r > 1e-15) {
                    off = fmax(off, r);
                    const double zeta = (be - al) / (2.0 * ga);
                    const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const double u = x[k], v = y[k];
                        x[k] = cs * u - sn * v;
                        a[9 * q + k] = sn * u + cs * v;
                    }
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const double u = V[9 * k + p], v = V[9 * k + q];
                        V[9 * k + p] = cs * u - sn * v;
                        V[9 * k + q] = sn * u + cs * v;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) a[9 * p + k] = x[k];
        }
        if (off < 1e-15) break;
    }
    int best = 0;
    double bn = 0.0;
    for (int j = 0; j < 9; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) s += a[9 * j + k] * a[9 * j + k];
        if (j == 0 || s < bn) { bn = s; best = j; }
    }
    return best;
}

// The normalised least-squares fit over the masked correspondences (n_in of
// them, at least 8): Hartley statistics of the inliers on each side, the N x 9
// design reduced to a 9 x 9 triangular factor by per-thread Givens rotations
// and the LDS tree merge of k_dlt_general, then thread 0's one-sided Jacobi
// for the right singular vector of the least singular value and vp_finish.
// F to every thread, through sFn.
__device__ __forceinline__ void vp_refit(const EpiPair &w, const uint8_t *mask, int n_in, double (*red)[4],
                                         double (*Rs)[45], double *sFn, double (&F)[9]) {
    const int t = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < w.n; i += VP_RT) {
        if (!mask[i]) continue;
        const double2 p = w.x1[i], q = w.x2[i];
        s[0] += p.x; s[1] += p.y; s[2] += q.x; s[3] += q.y;
    }
    wg_sum<VP_RW, 4>(s, red);
    const double N = (double)n_in;
    const double m1x = s[0] / N, m1y = s[1] / N, m2x = s[2] / N, m2y = s[3] / N;
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < w.n; i += VP_RT) {
        if (!mask[i]) continue;
        const double2 p = w.x1[i], q = w.x2[i];
        const double ax = p.x - m1x, ay = p.y - m1y, bx = q.x - m2x, by = q.y - m2y;
        d[0] += sqrt(ax * ax + ay * ay);
        d[1] += sqrt(bx * bx + by * by);
    }
    wg_sum<VP_RW, 4>(d, red);
    Hartley h1, h2;
    h1.s = 1.4142135623730951 / (d[0] / N + 1e-8);
    h2.s = 1.4142135623730951 / (d[1] / N + 1e-8);
    h1.ox = -h1.s * m1x; h1.oy = -h1.s * m1y; h2.ox = -h2.s * m2x; h2.oy = -h2.s * m2y;
    double R[9][9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = 0; j < 9; ++j) R[i][j] = 0.0;
    for (int i = t; i < w.n; i += VP_RT) {
        if (!mask[i]) continue;
        const double2 p = w.x1[i], q = w.x2[i];
        double row[9];
        vp_row(h1.s * p.x + h1.ox, h1.s * p.y + h1.oy, h2.s * q.x + h2.ox, h2.s * q.y + h2.oy, row);
        givens_absorb(R, row);
    }
    for (int wd = VP_RT / 2; wd > 0; wd >>= 1) {
        if (t >= wd && t < 2 * wd) {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) Rs[t][k++] = R[i][j];
        }
        __syncthreads();
        if (t < wd) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                double row[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) row[j] = 0.0;
#pragma unroll
                for (int j = i; j < 9; ++j) row[j] = Rs[t + wd][i * 9 - i * (i - 1) / 2 + (j - i)];
                givens_absorb(R, row);
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        // the merge is over: its LDS now holds the factor's columns and V
        double *a = &Rs[0][0], *V = a + 81;  // a[9 col + row], V[9 row + col]
#pragma unroll
        for (int c = 0; c < 9; ++c)
#pragma unroll
            for (int r = 0; r < 9; ++r) a[9 * c + r] = r <= c ? R[r][c] : 0.0;
        const int j = vp_jacobi9(a, V);
        double f[9], Fn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = V[9 * k + j];
        vp_finish(f, h1, h2, Fn);
#pragma unroll
        for (int k = 0; k < 9; ++k) sFn[k] = Fn[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = sFn[k];
}

// One workgroup per pair.  mask2: scratch of n_corr bytes.  Pairs of fewer than
// eight correspondences are the host's (info -1): nothing of them is read.
__global__ void __launch_bounds__(VP_RT)
k_vp_refit(const int64_t *__restrict__ pair_start, const double2 *__restrict__ x1, const double2 *__restrict__ x2,
           int32_t H, double thr, int32_t min_inliers, int32_t refit_rounds, const double *__restrict__ models,
           const int32_t *__restrict__ counts, uint8_t *mask2, double *__restrict__ F_out,
           double *__restrict__ cost_out, int32_t *__restrict__ n_inl_out, int32_t *__restrict__ hyp_out,
           int32_t *__restrict__ count_out, int32_t *__restrict__ info_out, uint8_t *inlier) {
    __shared__ int32_t sc[VP_RW];
    __shared__ int64_t sh[VP_RW];
    __shared__ int32_t sFirst;
    __shared__ double red[VP_RW][4];
    __shared__ double sFn[9];
    __shared__ double Rs[VP_RT][45];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int64_t ps = pair_start[p];
    const int n = (int)(pair_start[p + 1] - ps);
    if (n < 8) return;
    const EpiPair w{x1 + ps, x2 + ps, n};
    uint8_t *mask = inlier + ps, *trial = mask2 + ps;
    const double thr2 = thr * thr;

    int32_t bc;
    int64_t bh;
    if (tid == 0) sFirst = H;
    wg_select_best<VP_RT>(counts + p * H, H, sc, sh, bc, bh);  // holds a barrier
    if (bh < 0) {  // every count is 0: the earliest finite hypothesis, if any
        for (int32_t h = tid; h < H; h += VP_RT) {
            const double *m = models + (p * H + h) * 9;
            bool fin = true;
            for (int j = 0; j < 9; ++j) fin = fin && isfinite(m[j]);
            if (fin) {
                atomicMin(&sFirst, h);
                break;
            }
        }
        __syncthreads();
        bh = sFirst < H ? sFirst : -1;
        bc = 0;
    }
    double F[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cost = 0.0;
    int info = -2, n_inl = 0;
    if (bh >= 0) {
        const double *m = models + (p * H + bh) * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) F[j] = m[j];
        epi_mask<VP_RT>(w, F, thr2, mask, n_inl, cost, red);
        info = -3;
        if (bc >= min_inliers) {
            // a round: the least-squares fit over the inliers, while there are eight of them
            const EpiStop stop = epi_refit_rounds<VP_RT>(
                w, thr2, F, n_inl, cost, mask, trial, refit_rounds, red,
                [&](const uint8_t *cur, int n_cur, double (&Fn)[9]) {
                    if (n_cur < 8) return false;
                    vp_refit(w, cur, n_cur, red, Rs, sFn, Fn);
                    return true;
                },
                [] {});
            info = stop == EPI_UNCHANGED ? 1 : refit_rounds > 0 ? 2 : 0;
        }
    }
    if (tid == 0)
        for (int j = 0; j < 9; ++j) F_out[9 * p + j] = F[j];
    epi_store_pair<VP_RT>(p, n, mask, (int32_t)bh, bc, cost, n_inl, info, cost_out, n_inl_out, hyp_out, count_out,
                          info_out);
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_verify_pairs(const int64_t *pair_start, int64_t P, const double *x1, const double *x2,
                                int64_t n_corr, const int32_t *samples, int64_t H, double threshold,
                                int32_t min_inliers, int32_t refit_rounds, double *F, double *cost,
                                int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                                uint8_t *inlier, int32_t *counts, double *models, int device) {
    static const PairSpec spec{8, 8, 1, VP_HT, VP_TILE, false, "min_inliers must be at least 8"};
    Slot<int32_t> o_cnt;
    Slot<double> o_m;
    return pair_run(
        spec, nullptr, pair_start, P, x1, x2, n_corr, samples, H, threshold, min_inliers, refit_rounds, 0, nullptr, F,
        cost, n_inliers, best_hyp, best_count, info, inlier, nullptr, counts, models, device,
        [&](Pack &out, size_t PH) { o_cnt = out.add<int32_t>(PH), o_m = out.add<double>(9 * PH); },
        [&](const PairCall &c, int refit) {
            if (!refit)
                hipLaunchKernelGGL(k_vp_fit_score, dim3((unsigned)c.blocks), dim3(VP_THREADS), 0, c.s, c.ps, c.x1, c.x2,
                                   c.samples, (int32_t)c.H, c.blk_start, c.tab, (int32_t)c.n_live, c.threshold,
                                   c.out.ptr(o_m), c.out.ptr(o_cnt));
            else
                hipLaunchKernelGGL(k_vp_refit, dim3((unsigned)c.P), dim3(VP_RT), 0, c.s, c.ps, c.x1, c.x2, (int32_t)c.H,
                                   c.threshold, c.min_inliers, c.refit_rounds, c.out.ptr(o_m), c.out.ptr(o_cnt),
                                   c.mask2, c.F, c.cost, c.n_inl, c.hyp, c.count, c.info, c.mask);
        },
        [&](const PairCall &c, int64_t p0, int64_t p1) -> int {
            SFM_TRY(c.out.download_rows(counts, o_cnt, c.H, p0, p1, c.s));
            return c.out.download_rows(models, o_m, 9 * c.H, p0, p1, c.s);
        });
}
