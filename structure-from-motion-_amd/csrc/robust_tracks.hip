// Robust multi-view track triangulation: k_triangulate_tracks (multiview.hip)
// trusts every observation of a track; this kernel finds the observations
// that agree on one point, fits that point to them alone and reports the mask.
//
// Hypotheses are view pairs (i, j) of a track, positions inside it, widest
// index gap first and at most max_pairs of them.  A pair's point is the
// two-view DLT (triangulate_point); its score is the number of the track's
// observations within `threshold` pixels of the point's projection and in
// front of their camera, then the sum of those observations' squared errors,
// then the pair's place in the enumeration: a total order on quantities of the
// hypothesis alone.  The winner's inliers are refitted with the bodies of
// k_triangulate_tracks (mv_tracks.hpp) under the mask, so the result is that
// kernel's for the track with the outliers removed, bit for bit, and the mask
// is recomputed once against the refitted point.
//
// Mapping: a track belongs to a group of G lanes (a power of two inside one
// wave64; 256 / G tracks per workgroup).  Lane l scores pairs k = l, l + G,
// ... and keeps its best; the group's best is a butterfly of cross-lane
// exchanges under the order above, which every lane ends with, and the
// winner's point is read from the lane that owns it.  The refit runs on the
// group's first lane.  The scores do not depend on G, so neither do the
// results.  The mask lives in the per-observation output, never in registers:
// tracks have no length limit.
#include <cmath>

#include "staging.hpp"
// triangulate_point.hpp before lm_small.hpp, as in multiview.hip: the DLT body
// is compiled as sfm_api.hip compiles it and returns sfm_triangulate_dlt's bits.
#include "triangulate_point.hpp"
#include "lm_small.hpp"
#include "nltri_loss.hpp"
#include "mv_tracks.hpp"

#pragma clang fp contract(off)

namespace sfm {

// Counts the track's observations that are inliers of X and adds their
// squared errors in observation order: h summed as mv_stream sums it, an
// inlier where h2 > 0, not |h2| < 1e-8 and (u - h0/h2)^2 + (v - h1/h2)^2 <
// thr2.  A point that is not finite has none.  With WRITE the mask is stored.
template <bool LDS, bool WRITE>
__device__ __forceinline__ void rt_score(const double *Pb, const int32_t *__restrict__ cam,
                                         const double2 *__restrict__ xy, int64_t s, int64_t e, const double (&X)[3],
                                         double thr2, int &count, double &sse, uint8_t *mask) {
    count = 0;
    sse = 0.0;
    const bool finite = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
    for (int64_t k = s; k < e; ++k) {
        bool in = false;
        if (finite) {
            const double *P = mv_row<LDS>(Pb, cam[k]);
            const double2 o = xy[k];
            const double h0 = (P[0] * X[0] + P[2] * X[2]) + (P[1] * X[1] + P[3]);
            const double h1 = (P[4] * X[0] + P[6] * X[2]) + (P[5] * X[1] + P[7]);
            const double h2 = (P[8] * X[0] + P[10] * X[2]) + (P[9] * X[1] + P[11]);
            if (h2 > 0.0 && !(fabs(h2) < 1e-8)) {
                const double px = h0 / h2, py = h1 / h2;
                const double ru = o.x - px, rv = o.y - py;
                const double e2 = ru * ru + rv * rv;
                if (e2 < thr2) {
                    in = true;
                    ++count;
                    sse += e2;
                }
            }
        }
        if (WRITE) mask[k] = in ? 1 : 0;
    }
}

// (count, sse, pair) a beats b: more inliers, then the smaller error sum,
// then the earlier pair
__device__ __forceinline__ bool rt_better(int ca, double sa, int ka, int cb, double sb, int kb) {
    return ca > cb || (ca == cb && (sa < sb || (sa == sb && ka < kb)));
}

// The largest angle between the rays X - C_i, X - C_j over pairs of kept
// observations: the pair of smallest cosine, its angle by atan2(|a x b|, a.b).
__device__ __forceinline__ double rt_angle(const double *__restrict__ centres, const int32_t *__restrict__ cam,
                                           int64_t s, int64_t e, const uint8_t *mask, const double (&X)[3]) {
    double cmin = 2.0, best_sin = 0.0, best_dot = 1.0;
    for (int64_t a = s; a < e; ++a) {
        if (!mask[a]) continue;
        const double *Ca = centres + (int64_t)cam[a] * 3;
        const double a0 = X[0] - Ca[0], a1 = X[1] - Ca[1], a2 = X[2] - Ca[2];
        const double na = a0 * a0 + a1 * a1 + a2 * a2;
        for (int64_t b = a + 1; b < e; ++b) {
            if (!mask[b]) continue;
            const double *Cb = centres + (int64_t)cam[b] * 3;
            const double b0 = X[0] - Cb[0], b1 = X[1] - Cb[1], b2 = X[2] - Cb[2];
            const double nb = b0 * b0 + b1 * b1 + b2 * b2;
            const double dot = a0 * b0 + a1 * b1 + a2 * b2;
            const double c = dot / sqrt(na * nb);
            if (c < cmin) {
                cmin = c;
                const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
                best_sin = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
                best_dot = dot;
            }
        }
    }
    return cmin < 2.0 ? atan2(best_sin, best_dot) : 0.0;
}

// Outputs per track: X, cost (sum of the final inliers' squared errors),
// n_inliers, best_pair (the winner's place in the enumeration, -1 without
// one), best_count (its inlier count), info (>= 1 the refinement's stop code,
// -1 as k_triangulate_tracks, -2 fewer than two views: X = 0 and an empty
// mask, -3 no hypothesis with min_inliers: X the best hypothesis's point, the
// mask, count and cost its own), angle where centres are given; per
// observation the inlier mask.  LG = log2 of the lanes per track.
template <bool LDS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_triangulate_tracks_robust(const double *__restrict__ Pg, int32_t n_cams, const double *__restrict__ centres,
                            const int64_t *__restrict__ track_start, const int32_t *__restrict__ obs_cam,
                            const double2 *__restrict__ obs_xy, int64_t T, double thr2, int32_t max_pairs,
                            int32_t min_inliers, int32_t max_nfev, int32_t LG, double *__restrict__ X,
                            double *__restrict__ cost_out, int32_t *__restrict__ n_inl_out, uint8_t *inlier,
                            int32_t *__restrict__ pair_out, int32_t *__restrict__ count_out,
                            int32_t *__restrict__ info_out, double *__restrict__ angle_out) {
    __shared__ __attribute__((aligned(16))) double sP[LDS ? MV_LDS_CAMS * MV_ROW : 2];
    if (LDS) {
        for (int i = threadIdx.x; i < n_cams * 12; i += blockDim.x) sP[(i / 12) * MV_ROW + i % 12] = Pg[i];
        __syncthreads();
    }
    const double *Pb = LDS ? sP : Pg;
    const int G = 1 << LG;
    const int l = threadIdx.x & (G - 1);
    const int64_t t = (int64_t)blockIdx.x * (256 >> LG) + (threadIdx.x >> LG);
    // no lane leaves before the exchanges: a group's lanes share t, so a
    // group is whole or idle, but the exchanges are executed by every lane
    const bool live = t < T;
    const int64_t s = live ? track_start[t] : 0, e = live ? track_start[t + 1] : 0;
    const int64_t n = e - s;
    const int64_t all_pairs = n >= 2 ? (n % 2 ? n * ((n - 1) / 2) : (n / 2) * (n - 1)) : 0;
    const int npairs = (int)(all_pairs < (int64_t)max_pairs ? all_pairs : (int64_t)max_pairs);

    // this lane's hypotheses.  Level m = 1, 2, ... holds the m pairs of index
    // gap n - m, i = 0 .. m - 1; the levels before it hold m (m - 1) / 2.
    int bc = -1, bk = -1;
    double bs = 0.0, bx[3] = {0.0, 0.0, 0.0};
    int64_t m = 1;
    for (int k = l; k < npairs; k += G) {
        while (m * (m + 1) / 2 <= k) ++m;
        const int64_t i = k - m * (m - 1) / 2, j = i + (n - m);
        double x[3];
        triangulate_point(mv_row<LDS>(Pb, obs_cam[s + i]), mv_row<LDS>(Pb, obs_cam[s + j]), obs_xy[s + i],
                          obs_xy[s + j], x);
        int c;
        double sse;
        rt_score<LDS, false>(Pb, obs_cam, obs_xy, s, e, x, thr2, c, sse, nullptr);
        if (rt_better(c, sse, k, bc, bs, bk)) {
            bc = c; bs = sse; bk = k;
            bx[0] = x[0]; bx[1] = x[1]; bx[2] = x[2];
        }
    }
    // the group's winner, known to each of its lanes
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        if (w < G) {
            const int oc = __shfl_xor(bc, w), ok = __shfl_xor(bk, w);
            const double os = __shfl_xor(bs, w);
            if (rt_better(oc, os, ok, bc, bs, bk)) {
                bc = oc; bs = os; bk = ok;
            }
        }
    }
    if (G > 1) {
        const int owner = bk >= 0 ? (bk & (G - 1)) : 0;
        bx[0] = __shfl(bx[0], owner, G);
        bx[1] = __shfl(bx[1], owner, G);
        bx[2] = __shfl(bx[2], owner, G);
    }
    if (!live || l != 0) return;

    double x[3] = {0.0, 0.0, 0.0}, cost = 0.0;
    int info = -2, n_inl = 0, count = 0;
    if (n < 2) {
        for (int64_t k = s; k < e; ++k) inlier[k] = 0;
    } else {
        x[0] = bx[0]; x[1] = bx[1]; x[2] = bx[2];
        count = bc;
        rt_score<LDS, true>(Pb, obs_cam, obs_xy, s, e, x, thr2, n_inl, cost, inlier);
        info = -3;
        if (bc >= min_inliers) {
            const MvMask keep{inlier};
            if (n_inl == 2) {
                int64_t ia = s;
                while (ia + 2 < e && !inlier[ia]) ++ia;
                int64_t ib = ia + 1;
                while (ib + 1 < e && !inlier[ib]) ++ib;
                const double *Pa = mv_row<LDS>(Pb, obs_cam[ia]), *Pc = mv_row<LDS>(Pb, obs_cam[ib]);
                const double2 u = obs_xy[ia], v = obs_xy[ib];
                triangulate_point(Pa, Pc, u, v, x);
                NlTriLoss loss{Pa, Pc, u.x, u.y, v.x, v.y};
                bool ok = !(isnan(x[0]) || isnan(x[1]) || isnan(x[2]));
                if (ok) {
                    double f0[4];
                    loss(x, f0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) ok = ok && isfinite(f0[k]);
                }
                info = -1;
                if (ok) info = lm::lmdif<4, 3>(loss, x, 1e-8, 1e-8, 1e-8, max_nfev);
            } else {
                mv_dlt<LDS>(Pb, obs_cam, obs_xy, s, e, keep, x);
                info = -1;
                if (!(isnan(x[0]) || isnan(x[1]) || isnan(x[2]))) {
                    double c;
                    bool front;
                    info = mv_refine<LDS>(Pb, obs_cam, obs_xy, s, e, keep, x, max_nfev, c, front);
                }
            }
            rt_score<LDS, true>(Pb, obs_cam, obs_xy, s, e, x, thr2, n_inl, cost, inlier);
        }
    }
    X[3 * t] = x[0];
    X[3 * t + 1] = x[1];
    X[3 * t + 2] = x[2];
    cost_out[t] = cost;
    n_inl_out[t] = n_inl;
    pair_out[t] = n < 2 ? -1 : bk;
    count_out[t] = count;
    info_out[t] = info;
    if (angle_out) angle_out[t] = rt_angle(centres, obs_cam, s, e, inlier, x);
}

// Lanes per track when the caller leaves the choice open.  One lane per
// track wastes nothing (the refit runs on one lane of a group while the
// others idle), so it is the choice while the tracks alone fill the machine:
// 256 CUs x 4 SIMDs x 2 waves x 64 lanes.  Fewer tracks than that get the idle
// lanes, up to the longest track's pair count.  And where the longest track
// has many times the mean's pairs it would hold its wave that many times
// longer: its pairs are spread until a lane's share is about the mean track's.
static int auto_lanes(int64_t T, double mean_pairs, int64_t max_track_pairs) {
    const int64_t machine_lanes = 256 * 4 * 2 * 64;
    int G = 1;
    while (G < 64 && 2 * G <= max_track_pairs && T * (2 * G) <= machine_lanes) G *= 2;
    if (mean_pairs >= 1.0 && (double)max_track_pairs >= 4.0 * mean_pairs)
        while (G < 64 && (double)G * mean_pairs < (double)max_track_pairs) G *= 2;
    return G;
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_triangulate_tracks_robust(const double *P, int32_t n_cams, const double *centres,
                                             const int64_t *track_start, int64_t T, const int32_t *obs_cam,
                                             const double *obs_xy, int64_t n_obs, double threshold,
                                             int32_t max_pairs, int32_t min_inliers, int32_t max_nfev,
                                             int32_t lanes_per_track, double *X, double *cost, int32_t *n_inliers,
                                             uint8_t *inlier, int32_t *best_pair, int32_t *best_count,
                                             int32_t *info, double *angle, int device) {
    SFM_CHECK_ARG(T >= 0 && n_obs >= 0, "T < 0 or n_obs < 0");
    SFM_CHECK_ARG(n_cams >= 0, "n_cams < 0");
    SFM_CHECK_ARG(std::isfinite(threshold) && threshold > 0.0, "threshold must be finite and positive");
    SFM_CHECK_ARG(max_pairs >= 1, "max_pairs must be at least 1");
    SFM_CHECK_ARG(min_inliers >= 2, "min_inliers must be at least 2");
    SFM_CHECK_ARG(max_nfev > 0, "max_nfev must be positive");
    SFM_CHECK_ARG(lanes_per_track >= 0 && lanes_per_track <= 64 && (lanes_per_track & (lanes_per_track - 1)) == 0,
                  "lanes_per_track is 0 or a power of two up to 64");
    SFM_CHECK_ARG(centres || !angle, "angle needs centres");
    SFM_CHECK_ARG(track_start, "null pointer");
    SFM_TRY(check_csr(track_start, T, n_obs, "track_start", "observation"));
    SFM_CHECK_ARG(n_obs == 0 || (obs_cam && obs_xy && P), "null pointer");
    SFM_TRY(check_index(obs_cam, n_obs, n_cams, "camera index outside [0, n_cams)"));
    if (T == 0) return 0;
    SFM_CHECK_ARG(X && cost && n_inliers && best_pair && best_count && info && (inlier || n_obs == 0),
                  "null pointer");
    int64_t max_track_pairs = 0, long_tracks = 0;
    double sum_pairs = 0.0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t n = track_start[t + 1] - track_start[t];
        if (n < 2) continue;
        const double all = 0.5 * (double)n * (double)(n - 1);
        const int64_t p = all < (double)max_pairs ? (int64_t)all : (int64_t)max_pairs;
        max_track_pairs = p > max_track_pairs ? p : max_track_pairs;
        sum_pairs += (double)p;
        ++long_tracks;
    }
    int G = lanes_per_track ? lanes_per_track
                            : auto_lanes(T, long_tracks ? sum_pairs / (double)long_tracks : 0.0, max_track_pairs);
    while (G > 1 && (T + (256 / G) - 1) / (256 / G) > (int64_t)0x7fffffff) G /= 2;
    SFM_CHECK_ARG((T + (256 / G) - 1) / (256 / G) <= (int64_t)0x7fffffff, "too many tracks for one launch");
    int LG = 0;
    while ((1 << LG) < G) ++LG;
    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_ts = in.add<int64_t>(T + 1);
    const auto i_xy = in.add<double2>(n_obs);
    const auto i_cam = in.add<int32_t>(n_obs);
    const auto i_c = in.add<double>(3 * (size_t)n_cams), i_p = in.add<double>(12 * (size_t)n_cams);
    const auto o_x = out.add<double>(3 * T), o_cost = out.add<double>(T), o_ang = out.add<double>(T);
    const auto o_info = out.add<int32_t>(T), o_ninl = out.add<int32_t>(T);
    const auto o_pair = out.add<int32_t>(T), o_cnt = out.add<int32_t>(T);
    const auto o_mask = out.add<uint8_t>(n_obs);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    hipStream_t s = c->stream;
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_ts, track_start, s));
    SFM_TRY(in.upload(i_xy, obs_xy, s));
    SFM_TRY(in.upload(i_cam, obs_cam, s));
    SFM_TRY(in.upload(i_c, centres, s));
    SFM_TRY(in.upload(i_p, P, s));
    SFM_TRY(tm.mark(s));
    auto kernel = n_cams <= MV_LDS_CAMS ? k_triangulate_tracks_robust<true> : k_triangulate_tracks_robust<false>;
    hipLaunchKernelGGL(kernel, dim3(ceil_div(T, 256 / G)), dim3(256), 0, s, in.ptr(i_p), n_cams,
                       centres ? in.ptr(i_c) : nullptr, in.ptr(i_ts), in.ptr(i_cam), in.ptr(i_xy), T,
                       threshold * threshold, max_pairs, min_inliers, max_nfev, LG, out.ptr(o_x), out.ptr(o_cost),
                       out.ptr(o_ninl), out.ptr(o_mask), out.ptr(o_pair), out.ptr(o_cnt), out.ptr(o_info),
                       angle ? out.ptr(o_ang) : nullptr);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    SFM_TRY(out.download(X, o_x, s));
    SFM_TRY(out.download(cost, o_cost, s));
    SFM_TRY(out.download(angle, o_ang, s));
    SFM_TRY(out.download(info, o_info, s));
    SFM_TRY(out.download(n_inliers, o_ninl, s));
    SFM_TRY(out.download(best_pair, o_pair, s));
    SFM_TRY(out.download(best_count, o_cnt, s));
    SFM_TRY(out.download(inlier, o_mask, s));
    return tm.finish(s);
}
