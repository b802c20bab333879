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

#include "sfm_common.hpp"
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

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

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
    SFM_CHECK_ARG(track_start[0] == 0, "track_start does not start at 0");
    for (int64_t t = 0; t < T; ++t)
        SFM_CHECK_ARG(track_start[t + 1] >= track_start[t], "track_start decreases");
    SFM_CHECK_ARG(track_start[T] == n_obs, "track_start does not end at the observation count");
    SFM_CHECK_ARG(n_obs == 0 || (obs_cam && obs_xy && P), "null pointer");
    // a camera index out of range is an error here, never a device read
    for (int64_t k = 0; k < n_obs; ++k)
        SFM_CHECK_ARG(obs_cam[k] >= 0 && obs_cam[k] < n_cams, "camera index outside [0, n_cams)");
    if (T == 0) return 0;
    SFM_CHECK_ARG(X && cost && front && info, "null pointer");
    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    // buf[0]: track_start | obs_xy | obs_cam | X0 | P;  buf[1]: X | cost | info | front
    const size_t b_ts = (size_t)(T + 1) * sizeof(int64_t), b_xy = (size_t)n_obs * sizeof(double2),
                 b_cam = (size_t)n_obs * sizeof(int32_t), b_x = (size_t)T * 3 * sizeof(double),
                 b_p = (size_t)n_cams * 12 * sizeof(double);
    const size_t o_xy = up256(b_ts), o_cam = o_xy + up256(b_xy), o_x0 = o_cam + up256(b_cam),
                 o_p = o_x0 + up256(b_x), in_bytes = o_p + up256(b_p);
    const size_t o_cost = up256(b_x), o_info = o_cost + up256((size_t)T * sizeof(double)),
                 o_front = o_info + up256((size_t)T * sizeof(int32_t)), out_bytes = o_front + up256((size_t)T);
    int rc;
    if ((rc = c->buf[0].reserve(in_bytes)) || (rc = c->buf[1].reserve(out_bytes))) return rc;
    char *in = c->buf[0].as<char>(), *out = c->buf[1].as<char>();
    hipStream_t s = c->stream;
    const bool tm = call_timing();  // HIP events only when asked (each costs the stream us)
    if (tm) SFM_HIP(hipEventRecord(c->ev[0], s));
    SFM_HIP(hipMemcpyAsync(in, track_start, b_ts, hipMemcpyHostToDevice, s));
    if (n_obs) {
        SFM_HIP(hipMemcpyAsync(in + o_xy, obs_xy, b_xy, hipMemcpyHostToDevice, s));
        SFM_HIP(hipMemcpyAsync(in + o_cam, obs_cam, b_cam, hipMemcpyHostToDevice, s));
    }
    if (X0) SFM_HIP(hipMemcpyAsync(in + o_x0, X0, b_x, hipMemcpyHostToDevice, s));
    if (n_cams) SFM_HIP(hipMemcpyAsync(in + o_p, P, b_p, hipMemcpyHostToDevice, s));
    if (tm) SFM_HIP(hipEventRecord(c->ev[1], s));
    const dim3 grid(ceil_div(T, 256)), block(256);
    const double *dX0 = X0 ? reinterpret_cast<const double *>(in + o_x0) : nullptr;
    if (n_cams <= MV_LDS_CAMS)
        hipLaunchKernelGGL(k_triangulate_tracks<true>, grid, block, 0, s, reinterpret_cast<const double *>(in + o_p),
                           n_cams, reinterpret_cast<const int64_t *>(in), reinterpret_cast<const int32_t *>(in + o_cam),
                           reinterpret_cast<const double2 *>(in + o_xy), dX0, T, mode, max_nfev,
                           reinterpret_cast<double *>(out), reinterpret_cast<double *>(out + o_cost),
                           reinterpret_cast<uint8_t *>(out + o_front), reinterpret_cast<int32_t *>(out + o_info));
    else
        hipLaunchKernelGGL(k_triangulate_tracks<false>, grid, block, 0, s, reinterpret_cast<const double *>(in + o_p),
                           n_cams, reinterpret_cast<const int64_t *>(in), reinterpret_cast<const int32_t *>(in + o_cam),
                           reinterpret_cast<const double2 *>(in + o_xy), dX0, T, mode, max_nfev,
                           reinterpret_cast<double *>(out), reinterpret_cast<double *>(out + o_cost),
                           reinterpret_cast<uint8_t *>(out + o_front), reinterpret_cast<int32_t *>(out + o_info));
    SFM_HIP(hipGetLastError());
    if (tm) SFM_HIP(hipEventRecord(c->ev[2], s));
    SFM_HIP(hipMemcpyAsync(X, out, b_x, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(cost, out + o_cost, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(info, out + o_info, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(front, out + o_front, (size_t)T, hipMemcpyDeviceToHost, s));
    if (tm) SFM_HIP(hipEventRecord(c->ev[3], s));
    SFM_HIP(hipStreamSynchronize(s));
    float a = 0, b = 0, d = 0;
    if (tm) (void)hipEventElapsedTime(&a, c->ev[0], c->ev[1]);
    if (tm) (void)hipEventElapsedTime(&b, c->ev[1], c->ev[2]);
    if (tm) (void)hipEventElapsedTime(&d, c->ev[2], c->ev[3]);
    const double t4[4] = {a, b, d, b};
    set_timings(t4, 4);
    return 0;
}
