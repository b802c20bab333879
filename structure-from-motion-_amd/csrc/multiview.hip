// Multi-view track triangulation: every track (a CSR row of observations
// (camera, x, y), cameras ascending) gets one point from ALL of its views in
// one launch -- the N-view generalisation of LinearTriangulation.py:54-90 and
// of NonLinearTriangulation.py:5-50's loss.  The reference's registration
// loop (Wrapper_dev.py:262-291) triangulates image pairs one at a time and
// keeps the last pair's point; this is the all-views answer it never forms.
//
// One thread owns one track.  Linear stage: the 2n x 4 DLT system is never
// stored; its rows stream through Givens rotations into a 4 x 4 upper
// triangle (A = QR, so R's right singular vectors are A's; no A^T A, which
// would square the condition number), then the one-sided Jacobi of
// sfm_geom.hpp.  Refinement: Levenberg-Marquardt on the three coordinates,
// one pass over the track per iteration accumulating J^T J, J^T r and the
// cost with analytic Jacobians, the damped 3 x 3 system solved in registers.
// Two-view tracks run the two-view kernels' own bodies (triangulate_point,
// lm::lmdif<4, 3> on NlTriLoss) and return their bits.
//
// The kernel is FP64-VALU / latency bound: a refined 8-view track reads
// 8 * 20 B of observations and writes 37 B, against ~10^4 flops.
#include <cstring>

#include "staging.hpp"
// triangulate_point.hpp comes before lm_small.hpp on purpose: lm_small.hpp
// turns FP contraction off for the rest of the translation unit, and the DLT
// body must be compiled as sfm_api.hip and two_view.hip compile it to return
// sfm_triangulate_dlt's bits.
#include "triangulate_point.hpp"
#include "lm_small.hpp"
#include "nltri_loss.hpp"
#include "mv_tracks.hpp"

#pragma clang fp contract(off)

namespace sfm {

enum { MV_LINEAR = SFM_TRACKS_LINEAR, MV_REFINE = SFM_TRACKS_REFINE, MV_BOTH = SFM_TRACKS_BOTH };

// Outputs per track: X, cost (sum of squared residuals at X), front (X in
// front of every camera of the track), info: >= 1 the refinement's stop code
// (MINPACK's for a two-view track), 0 linear mode, -1 as k_nltri (a NaN in
// the start, or residuals that are not finite there: X is the start), -2
// fewer than two views (X = X0 where given, else 0; cost 0, front 0).
template <bool LDS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_triangulate_tracks(const double *__restrict__ Pg, int32_t n_cams, const int64_t *__restrict__ track_start,
                     const int32_t *__restrict__ obs_cam, const double2 *__restrict__ obs_xy,
                     const double *__restrict__ X0, int64_t T, int32_t mode, int32_t max_nfev,
                     double *__restrict__ X, double *__restrict__ cost_out, uint8_t *__restrict__ front_out,
                     int32_t *__restrict__ info_out) {
    __shared__ __attribute__((aligned(16))) double sP[LDS ? MV_LDS_CAMS * MV_ROW : 2];
    if (LDS) {
        for (int i = threadIdx.x; i < n_cams * 12; i += blockDim.x) sP[(i / 12) * MV_ROW + i % 12] = Pg[i];
        __syncthreads();
    }
    const double *Pb = LDS ? sP : Pg;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int64_t s = track_start[t], e = track_start[t + 1];
    const int64_t n = e - s;
    double x[3] = {0.0, 0.0, 0.0};
    if (X0) {
        x[0] = X0[3 * t]; x[1] = X0[3 * t + 1]; x[2] = X0[3 * t + 2];
    }
    double cost = 0.0;
    bool front = false;
    int info = -2;
    if (n >= 2) {
        info = 0;
        bool done = false;  // cost and front already belong to x
        if (n == 2) {
            const double *Pa = mv_row<LDS>(Pb, obs_cam[s]), *Pc = mv_row<LDS>(Pb, obs_cam[s + 1]);
            const double2 u = obs_xy[s], v = obs_xy[s + 1];
            if (mode != MV_REFINE) triangulate_point(Pa, Pc, u, v, x);
            if (mode != MV_LINEAR) {
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
            }
        } else {
            if (mode != MV_REFINE) {
                mv_dlt<LDS>(Pb, obs_cam, obs_xy, s, e, MvAll{}, x);
            }
            if (mode != MV_LINEAR) {
                info = -1;
                if (!(isnan(x[0]) || isnan(x[1]) || isnan(x[2]))) {
                    info = mv_refine<LDS>(Pb, obs_cam, obs_xy, s, e, MvAll{}, x, max_nfev, cost, front);
                    done = true;
                }
            }
        }
        if (!done) {
            double A[6], g[3];
            mv_stream<LDS, false>(Pb, obs_cam, obs_xy, s, e, MvAll{}, x, cost, front, A, g);
        }
    }
    X[3 * t] = x[0];
    X[3 * t + 1] = x[1];
    X[3 * t + 2] = x[2];
    cost_out[t] = cost;
    front_out[t] = front ? 1 : 0;
    info_out[t] = info;
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_triangulate_tracks(const double *P, int32_t n_cams, const int64_t *track_start, int64_t T,
                                      const int32_t *obs_cam, const double *obs_xy, int64_t n_obs, const double *X0,
                                      int32_t mode, int32_t max_nfev, double *X, double *cost, uint8_t *front,
                                      int32_t *info, int device) {
    SFM_CHECK_ARG(T >= 0 && n_obs >= 0, "T < 0 or n_obs < 0");
    SFM_CHECK_ARG(n_cams >= 0, "n_cams < 0");
    SFM_CHECK_ARG(mode == MV_LINEAR || mode == MV_REFINE || mode == MV_BOTH, "mode is not 0, 1 or 2");
    SFM_CHECK_ARG(max_nfev > 0, "max_nfev must be positive");
    SFM_CHECK_ARG(mode != MV_REFINE || X0, "refine-only mode needs X0");
    SFM_CHECK_ARG(track_start, "null pointer");
    SFM_TRY(check_csr(track_start, T, n_obs, "track_start", "observation"));
    SFM_CHECK_ARG(n_obs == 0 || (obs_cam && obs_xy && P), "null pointer");
    SFM_TRY(check_index(obs_cam, n_obs, n_cams, "camera index outside [0, n_cams)"));
    if (T == 0) return 0;
    SFM_CHECK_ARG(X && cost && front && info, "null pointer");
    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_ts = in.add<int64_t>(T + 1);
    const auto i_xy = in.add<double2>(n_obs);
    const auto i_cam = in.add<int32_t>(n_obs);
    const auto i_x0 = in.add<double>(3 * T), i_p = in.add<double>(12 * (size_t)n_cams);
    const auto o_x = out.add<double>(3 * T), o_cost = out.add<double>(T);
    const auto o_info = out.add<int32_t>(T);
    const auto o_front = out.add<uint8_t>(T);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    hipStream_t s = c->stream;
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_ts, track_start, s));
    SFM_TRY(in.upload(i_xy, obs_xy, s));
    SFM_TRY(in.upload(i_cam, obs_cam, s));
    SFM_TRY(in.upload(i_x0, X0, s));
    SFM_TRY(in.upload(i_p, P, s));
    SFM_TRY(tm.mark(s));
    auto kernel = n_cams <= MV_LDS_CAMS ? k_triangulate_tracks<true> : k_triangulate_tracks<false>;
    hipLaunchKernelGGL(kernel, dim3(ceil_div(T, 256)), dim3(256), 0, s, in.ptr(i_p), n_cams, in.ptr(i_ts),
                       in.ptr(i_cam), in.ptr(i_xy), X0 ? in.ptr(i_x0) : nullptr, T, mode, max_nfev, out.ptr(o_x),
                       out.ptr(o_cost), out.ptr(o_front), out.ptr(o_info));
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    SFM_TRY(out.download(X, o_x, s));
    SFM_TRY(out.download(cost, o_cost, s));
    SFM_TRY(out.download(info, o_info, s));
    SFM_TRY(out.download(front, o_front, s));
    return tm.finish(s);
}
