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

#pragma clang fp contract(off)

namespace sfm {

constexpr int MV_LDS_CAMS = SFM_TRACKS_LDS_CAMS;
// LDS row stride in doubles.  A lane reads its camera's row with six
// ds_read_b128; that instruction serves 16 lanes per cycle over 64 banks of
// 4 B.  With 14 doubles (112 B = 28 banks) a row starts on bank 28 c mod 64,
// a multiple of 4 that takes 16 values: the 16-B reads of any 16 consecutive
// cameras fall on disjoint banks, cameras 16 apart share them, and lanes on
// the same camera broadcast.  The dense stride 12 (24 banks) repeats after 8.
constexpr int MV_ROW = 14;

enum { MV_LINEAR = SFM_TRACKS_LINEAR, MV_REFINE = SFM_TRACKS_REFINE, MV_BOTH = SFM_TRACKS_BOTH };

template <bool LDS>
__device__ __forceinline__ const double *mv_row(const double *base, int cam) {
    return LDS ? base + cam * MV_ROW : base + (int64_t)cam * 12;
}

// One Givens step of the streamed QR: row a (4 entries) is rotated into the
// upper triangle r = (r00 r01 r02 r03 | r11 r12 r13 | r22 r23 | r33).
__device__ __forceinline__ void givens_row(double (&r)[10], double (&a)[4]) {
    constexpr int D[4] = {0, 4, 7, 9};  // index of r_ii
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (a[i] != 0.0) {
            const double rii = r[D[i]];
            const double h = sqrt(rii * rii + a[i] * a[i]);
            const double c = rii / h, s = a[i] / h;
            r[D[i]] = h;
#pragma unroll
            for (int j = i + 1; j < 4; ++j) {
                const double rij = r[D[i] + j - i], aj = a[j];
                r[D[i] + j - i] = c * rij + s * aj;
                a[j] = c * aj - s * rij;
            }
        }
    }
}

// The track's cost at X (sum of squared residuals u - h0/h2, v - h1/h2; a
// view with |h2| < 1e-8 contributes none), whether X lies in front of every
// camera (h2 > 0), and with JAC the normal equations: A = J^T J as
// (00 01 02 11 12 22), g = J^T r.  h is summed as NlTriLoss sums it.  The cost
// is the same sequence of IEEE operations with and without JAC.
template <bool LDS, bool JAC>
__device__ __forceinline__ void mv_stream(const double *Pb, const int32_t *__restrict__ cam,
                                          const double2 *__restrict__ xy, int64_t s, int64_t e,
                                          const double (&X)[3], double &cost, bool &front, double (&A)[6],
                                          double (&g)[3]) {
    cost = 0.0;
    front = true;
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = 0.0;
        g[0] = g[1] = g[2] = 0.0;
    }
    for (int64_t k = s; k < e; ++k) {
        const double *P = mv_row<LDS>(Pb, cam[k]);
        const double2 o = xy[k];
        const double h0 = (P[0] * X[0] + P[2] * X[2]) + (P[1] * X[1] + P[3]);
        const double h1 = (P[4] * X[0] + P[6] * X[2]) + (P[5] * X[1] + P[7]);
        const double h2 = (P[8] * X[0] + P[10] * X[2]) + (P[9] * X[1] + P[11]);
        front = front && h2 > 0.0;
        if (!(fabs(h2) < 1e-8)) {
            const double px = h0 / h2, py = h1 / h2;
            const double ru = o.x - px, rv = o.y - py;
            cost += ru * ru + rv * rv;
            if (JAC) {
                const double inv = 1.0 / h2;
                double ju[3], jv[3];  // d ru / dX, d rv / dX
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    ju[j] = (px * P[8 + j] - P[j]) * inv;
                    jv[j] = (py * P[8 + j] - P[4 + j]) * inv;
                    g[j] += ju[j] * ru + jv[j] * rv;
                }
                A[0] += ju[0] * ju[0] + jv[0] * jv[0];
                A[1] += ju[0] * ju[1] + jv[0] * jv[1];
                A[2] += ju[0] * ju[2] + jv[0] * jv[2];
                A[3] += ju[1] * ju[1] + jv[1] * jv[1];
                A[4] += ju[1] * ju[2] + jv[1] * jv[2];
                A[5] += ju[2] * ju[2] + jv[2] * jv[2];
            }
        }
    }
}

// (A + lam diag(A)) d = -g by LDL^T in registers; false where the damped
// matrix is not positive definite (or holds a NaN).
__device__ __forceinline__ bool mv_solve3(const double (&A)[6], const double (&g)[3], double lam, double (&d)[3]) {
    const double m00 = A[0] + lam * A[0], m11 = A[3] + lam * A[3], m22 = A[5] + lam * A[5];
    const double d0 = m00;
    if (!(d0 > 0.0)) return false;
    const double l10 = A[1] / d0, l20 = A[2] / d0;
    const double d1 = m11 - l10 * A[1];
    if (!(d1 > 0.0)) return false;
    const double t = A[4] - l20 * A[1];
    const double l21 = t / d1;
    const double d2 = m22 - l20 * A[2] - l21 * t;
    if (!(d2 > 0.0)) return false;
    const double y0 = -g[0];
    const double y1 = -g[1] - l10 * y0;
    const double y2 = -g[2] - l20 * y0 - l21 * y1;
    d[2] = y2 / d2;
    d[1] = y1 / d1 - l21 * d[2];
    d[0] = y0 / d0 - l10 * d[1] - l20 * d[2];
    return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

// Levenberg-Marquardt over all 2n residuals of a track of three or more
// views (Marquardt's scaling, lambda 1e-3, /10 on an accepted step, x10 on a
// rejected one).  A step is accepted only where it lowers the cost.  The stop
// tests are MINPACK's with the reference's ftol = xtol = gtol = 1e-8 on this
// iteration's own quantities, and so are the codes: 1 the actual and the
// predicted relative reductions are both at most ftol, 2 the step is at most
// xtol |x|, 3 both, 4 the cosine between the residual and every Jacobian
// column is at most gtol, 5 max_nfev cost evaluations.  Returns -1 (x kept)
// where the cost at x is not finite.
template <bool LDS>
__device__ __forceinline__ int mv_refine(const double *Pb, const int32_t *__restrict__ cam,
                                         const double2 *__restrict__ xy, int64_t s, int64_t e, double (&x)[3],
                                         int max_nfev, double &cost, bool &front) {
    const double tol = 1e-8;
    double A[6], g[3], c0;
    bool fr;
    mv_stream<LDS, true>(Pb, cam, xy, s, e, x, c0, fr, A, g);
    cost = c0;
    front = fr;
    if (!isfinite(c0)) return -1;
    int nfev = 1, info = 0;
    double lam = 1e-3;
    while (info == 0) {
        double gn = 0.0;
        if (c0 != 0.0) {
            const double fn = sqrt(c0);
            if (A[0] > 0.0) gn = fmax(gn, fabs(g[0]) / (sqrt(A[0]) * fn));
            if (A[3] > 0.0) gn = fmax(gn, fabs(g[1]) / (sqrt(A[3]) * fn));
            if (A[5] > 0.0) gn = fmax(gn, fabs(g[2]) / (sqrt(A[5]) * fn));
        }
        if (gn <= tol) {
            info = 4;
            break;
        }
        bool accepted = false;
        while (!accepted && info == 0) {
            if (nfev >= max_nfev) {
                info = 5;
                break;
            }
            ++nfev;
            double d[3];
            if (!mv_solve3(A, g, lam, d)) {
                lam *= 10.0;
                continue;
            }
            double xt[3] = {x[0] + d[0], x[1] + d[1], x[2] + d[2]};
            double A1[6], g1[3], c1;
            bool fr1;
            mv_stream<LDS, true>(Pb, cam, xy, s, e, xt, c1, fr1, A1, g1);
            // the linear model's reduction |r|^2 - |r + J d|^2
            const double Ad0 = A[0] * d[0] + A[1] * d[1] + A[2] * d[2];
            const double Ad1 = A[1] * d[0] + A[3] * d[1] + A[4] * d[2];
            const double Ad2 = A[2] * d[0] + A[4] * d[1] + A[5] * d[2];
            const double prered =
                -(2.0 * (g[0] * d[0] + g[1] * d[1] + g[2] * d[2]) + (d[0] * Ad0 + d[1] * Ad1 + d[2] * Ad2)) / c0;
            const double actred = 1.0 - c1 / c0;
            const double pnorm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (c1 < c0) {
                x[0] = xt[0]; x[1] = xt[1]; x[2] = xt[2];
                c0 = c1;
                fr = fr1;
#pragma unroll
                for (int k = 0; k < 6; ++k) A[k] = A1[k];
                g[0] = g1[0]; g[1] = g1[1]; g[2] = g1[2];
                lam = fmax(lam * 0.1, 1e-15);
                accepted = true;
            } else {
                lam *= 10.0;
            }
            const double xnorm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            const bool fhit = fabs(actred) <= tol && prered <= tol && 0.5 * actred <= prered;
            const bool xhit = pnorm <= tol * xnorm;
            if (fhit) info = 1;
            if (xhit) info = fhit ? 3 : 2;
        }
    }
    cost = c0;
    front = fr;
    return info;
}

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
                double r[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) r[k] = 0.0;
                for (int64_t k = s; k < e; ++k) {
                    const double *P = mv_row<LDS>(Pb, obs_cam[k]);
                    const double2 o = obs_xy[k];
                    double a[4], b[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        a[c] = o.y * P[8 + c] - P[4 + c];
                        b[c] = P[c] - o.x * P[8 + c];
                    }
                    givens_row(r, a);
                    givens_row(r, b);
                }
                double a[4][4], V[4][4];  // a[col][row]
                a[0][0] = r[0]; a[0][1] = 0.0;  a[0][2] = 0.0;  a[0][3] = 0.0;
                a[1][0] = r[1]; a[1][1] = r[4]; a[1][2] = 0.0;  a[1][3] = 0.0;
                a[2][0] = r[2]; a[2][1] = r[5]; a[2][2] = r[7]; a[2][3] = 0.0;
                a[3][0] = r[3]; a[3][1] = r[6]; a[3][2] = r[8]; a[3][3] = r[9];
                jacobi_onesided<4, 4, 40>(a, V);
                const int j = weakest_column<4, 4>(a);
                const double h0 = V[0][j], h1 = V[1][j], h2 = V[2][j], h3 = V[3][j];
                if (fabs(h3) > 1e-8) {
                    x[0] = h0 / h3; x[1] = h1 / h3; x[2] = h2 / h3;
                } else {
                    x[0] = h0; x[1] = h1; x[2] = h2;
                }
            }
            if (mode != MV_LINEAR) {
                info = -1;
                if (!(isnan(x[0]) || isnan(x[1]) || isnan(x[2]))) {
                    info = mv_refine<LDS>(Pb, obs_cam, obs_xy, s, e, x, max_nfev, cost, front);
                    done = true;
                }
            }
        }
        if (!done) {
            double A[6], g[3];
            mv_stream<LDS, false>(Pb, obs_cam, obs_xy, s, e, x, cost, front, A, g);
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
