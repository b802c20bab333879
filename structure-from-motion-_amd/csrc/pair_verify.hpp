// The host driver of a call of the two pair-verification entry points
// (verify_pairs.hip: 8-point F; essential_pairs.hip: calibrated 5-point E), from
// the argument checks to the downloads.  What differs -- the tables a hypothesis
// leaves on the device and the two kernels -- comes in as a PairSpec and three
// callables.  Host code only; the refit rounds are epi_sampson.hpp's.
#pragma once
#include <cmath>
#include <cstring>

#include "hyp_batch.hpp"

namespace sfm {

struct PairSpec {
    int k;            // correspondences of a sample
    int min_n;        // ... of a live pair, and the least min_inliers
    int slots;        // models per hypothesis
    int ht, tile;     // most hypotheses per workgroup of the fit-and-score kernel, correspondences per LDS tile
    bool calibrated;  // takes K, max_nfev and returns E
    const char *min_inliers_msg;
};

// What the callables see of a call: the scalars, then device addresses.
struct PairCall {
    int64_t P, H, n_live, blocks;
    double threshold;
    int32_t min_inliers, refit_rounds, max_nfev;
    hipStream_t s;
    const Pack &out;  // for the slots the stage added
    const int64_t *ps;
    const double2 *x1, *x2;
    const int32_t *samples, *blk_start, *tab;
    double *E, *F, *cost;  // E: null unless calibrated
    int32_t *n_inl, *hyp, *count, *info;
    uint8_t *mask, *mask2;  // mask2: the refits' trial mask
};

// The arguments are sfm_essential_pairs' (include/sfmcore.h); K, E and n_sol
// are null and max_nfev is not read for a spec that is not calibrated, counts
// and models have sp.slots entries a hypothesis.
//   add(out, PH)            the stage's device tables for PH = P x H hypotheses, in the Pack's order
//   launch(call, 0 or 1)    the fit-and-score kernel, the winner-and-refit kernel
//   download(call, p0, p1)  the stage's optional tables of the live pairs [p0, p1), as an int
template <class Add, class Launch, class Download>
int pair_run(const PairSpec &sp, const double *K, const int64_t *pair_start, int64_t P, const double *x1,
             const double *x2, int64_t n_corr, const int32_t *samples, int64_t H, double threshold,
             int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, double *E, double *F, double *cost,
             int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info, uint8_t *inlier,
             int32_t *n_sol, int32_t *counts, double *models, int device, Add add, Launch launch,
             Download download) {
    const int64_t NS = sp.slots;
    SFM_CHECK_ARG(P >= 0 && n_corr >= 0, "P < 0 or n_corr < 0");
    SFM_CHECK_ARG(H >= 1 && H <= (int64_t)1 << 20, "H must lie in [1, 2^20]");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0, "threshold must be finite and positive");
    SFM_CHECK_ARG(min_inliers >= sp.min_n, sp.min_inliers_msg);
    SFM_CHECK_ARG(refit_rounds >= 0, "refit_rounds < 0");
    SFM_CHECK_ARG(!sp.calibrated || max_nfev > 0, "max_nfev must be positive");
    SFM_CHECK_ARG(P < (int64_t)0x7fffffff / (H * NS), "P x H too large for one call");
    SFM_CHECK_ARG((K || !sp.calibrated) && pair_start, "null pointer");
    if (sp.calibrated) {
        for (int j = 0; j < 9; ++j) SFM_CHECK_ARG(std::isfinite(K[j]), "K is not finite");
        double ki[9];
        const double det = inv3_adjugate(K, ki);
        SFM_CHECK_ARG(std::isfinite(det) && det != 0.0, "K is singular");
        for (int j = 0; j < 9; ++j) SFM_CHECK_ARG(std::isfinite(ki[j]), "K has no finite inverse");
    }
    SFM_TRY(check_csr(pair_start, P, n_corr, "pair_start", "correspondence", 0x7fffffff,
                      "a pair has too many correspondences"));
    const int64_t n_live = count_live(pair_start, P, sp.min_n);
    SFM_CHECK_ARG(n_corr == 0 || (x1 && x2), "null pointer");
    SFM_CHECK_ARG(n_live == 0 || samples, "null pointer");
    SFM_TRY(check_samples(pair_start, P, samples, H, sp.k, sp.min_n, "sample outside [0, n_p)"));
    if (P == 0) return 0;
    SFM_CHECK_ARG((E || !sp.calibrated) && F && cost && n_inliers && best_hyp && best_count && info, "null pointer");
    SFM_CHECK_ARG(inlier || n_corr == 0, "null pointer");
    // info -1: a pair below the minimum
    for (int64_t p = 0; p < P; ++p) {
        if (pair_start[p + 1] - pair_start[p] >= sp.min_n) continue;
        for (int j = 0; j < 9; ++j) F[9 * p + j] = 0.0;
        if (E) std::memset(E + 9 * p, 0, 9 * sizeof(double));
        cost[p] = 0.0;
        n_inliers[p] = 0;
        best_hyp[p] = -1;
        best_count[p] = 0;
        info[p] = -1;
        for (int64_t k = pair_start[p]; k < pair_start[p + 1]; ++k) inlier[k] = 0;
        if (n_sol) std::memset(n_sol + p * H, 0, (size_t)H * sizeof(int32_t));
        if (counts) std::memset(counts + p * H * NS, 0, (size_t)(H * NS) * sizeof(int32_t));
        if (models) std::memset(models + p * H * NS * 9, 0, (size_t)(H * NS * 9) * sizeof(double));
    }
    if (n_live == 0) return 0;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    TileTable tt;
    SFM_TRY(tt.build(c->pinned, n_live, pair_start, P, sp.min_n, H, sp.ht, sp.tile));

    const size_t PH = (size_t)P * (size_t)H;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_ps = in.add<int64_t>(P + 1);
    const auto i_x1 = in.add<double2>(n_corr), i_x2 = in.add<double2>(n_corr);
    const auto i_s = in.add<int32_t>(sp.k * PH);
    const auto i_t = in.add<int32_t>(tt.words());  // the block table
    const auto o_E = out.add<double>(sp.calibrated ? 9 * P : 0), o_F = out.add<double>(9 * P);
    const auto o_cost = out.add<double>(P);
    const auto o_info = out.add<int32_t>(P), o_ninl = out.add<int32_t>(P), o_hyp = out.add<int32_t>(P);
    const auto o_bc = out.add<int32_t>(P);
    add(out, PH);
    const auto o_mask = out.add<uint8_t>(n_corr), o_m2 = out.add<uint8_t>(n_corr);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    hipStream_t s = c->stream;
    const PairCall call{P, H, n_live, tt.blocks, threshold, min_inliers, refit_rounds, max_nfev, s, out,
                        in.ptr(i_ps), in.ptr(i_x1), in.ptr(i_x2), in.ptr(i_s), in.ptr(i_t), in.ptr(i_t, n_live + 1),
                        sp.calibrated ? out.ptr(o_E) : nullptr, out.ptr(o_F), out.ptr(o_cost), out.ptr(o_ninl),
                        out.ptr(o_hyp), out.ptr(o_bc), out.ptr(o_info), out.ptr(o_mask), out.ptr(o_m2)};
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_ps, pair_start, s));
    SFM_TRY(in.upload(i_x1, x1, s));
    SFM_TRY(in.upload(i_x2, x2, s));
    SFM_TRY(in.upload(i_s, samples, s));
    SFM_TRY(in.upload(i_t, tt.blk, s));
    SFM_TRY(tm.mark(s));
    launch(call, 0);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.split(s));  // [3]: the fit-and-score kernel alone
    launch(call, 1);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    SFM_TRY(for_each_live_run(pair_start, P, sp.min_n, [&](int64_t p0, int64_t p1, int64_t k0, int64_t k1) -> int {
        SFM_TRY(out.download_rows(E, o_E, 9, p0, p1, s));
        SFM_TRY(out.download_rows(F, o_F, 9, p0, p1, s));
        SFM_TRY(out.download_rows(cost, o_cost, 1, p0, p1, s));
        SFM_TRY(out.download_rows(info, o_info, 1, p0, p1, s));
        SFM_TRY(out.download_rows(n_inliers, o_ninl, 1, p0, p1, s));
        SFM_TRY(out.download_rows(best_hyp, o_hyp, 1, p0, p1, s));
        SFM_TRY(out.download_rows(best_count, o_bc, 1, p0, p1, s));
        SFM_TRY(out.download_rows(inlier, o_mask, 1, k0, k1, s));
        return download(call, p0, p1);
    }));
    return tm.finish(s);
}

}  // namespace sfm
