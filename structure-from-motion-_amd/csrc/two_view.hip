// Two-view initialisation between F-RANSAC and the first triangulation
// (Wrapper_dev.py:156-179): every pose candidate of ExtractCameraPose is
// triangulated and its cheirality count (DisambiguateCameraPose.py:58-70)
// taken in one launch; the host picks the first maximum.
#include <cstring>

#include "staging.hpp"
#include "triangulate_point.hpp"

namespace sfm {

constexpr int TV_MAX = 8;  // candidates per call

// Kernel arguments: wave-uniform, read through scalar loads.  Of each rotation
// only the third row enters the depth.
struct TvCams {
    double r1[3], c1[3];
    double r2[TV_MAX][3], c2[TV_MAX][3];
};
struct TvProj {
    double p1[12];
    double p2[TV_MAX][12];
};

// The workgroup's count of one candidate: a ballot per wave, the waves' sums
// through LDS, one integer atomic per workgroup.  Integer adds commute, so the
// counts do not depend on the order the workgroups arrive in.
__device__ __forceinline__ void add_count(bool front, unsigned long long *count) {
    __shared__ unsigned int wg;
    if (threadIdx.x == 0) wg = 0;
    __syncthreads();
    const unsigned long long b = __ballot(front);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&wg, (unsigned int)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && wg) atomicAdd(count, (unsigned long long)wg);
}

// One thread per (point, candidate); blockIdx.y is the candidate, so a wave
// holds 64 points of one candidate and its projection matrices stay scalar.
__global__ void __launch_bounds__(256) k_two_view_select(TvProj P, TvCams cam, const double2 *__restrict__ x1,
                                                         const double2 *__restrict__ x2, int64_t N,
                                                         double *__restrict__ X_all,
                                                         unsigned long long *__restrict__ counts) {
    const int m = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool front = false;
    if (i < N) {
        double X[3];
        triangulate_point(P.p1, P.p2[m], x1[i], x2[i], X);
        double *o = X_all + ((int64_t)m * N + i) * 3;
        o[0] = X[0]; o[1] = X[1]; o[2] = X[2];
        front = in_front_of_both(cam.r1, cam.c1, cam.r2[m], cam.c2[m], X);
    }
    add_count(front, counts + m);
}

// The same count on points the caller triangulated: Xset is M x N x 3.
__global__ void __launch_bounds__(256) k_cheirality_count(TvCams cam, const double *__restrict__ Xset, int64_t N,
                                                          unsigned long long *__restrict__ counts) {
    const int m = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool front = false;
    if (i < N) {
        const double *p = Xset + ((int64_t)m * N + i) * 3;
        const double X[3] = {p[0], p[1], p[2]};
        front = in_front_of_both(cam.r1, cam.c1, cam.r2[m], cam.c2[m], X);
    }
    add_count(front, counts + m);
}

static void fill_cams(TvCams &cam, const double *R1, const double *C1, const double *Rs, const double *Cs, int M) {
    std::memset(&cam, 0, sizeof cam);
    std::memcpy(cam.r1, R1 + 6, sizeof cam.r1);
    std::memcpy(cam.c1, C1, sizeof cam.c1);
    for (int m = 0; m < M; ++m) {
        std::memcpy(cam.r2[m], Rs + 9 * m + 6, sizeof cam.r2[m]);
        std::memcpy(cam.c2[m], Cs + 3 * m, sizeof cam.c2[m]);
    }
}

// DisambiguateCameraPose.py:77: strict '>', so the earliest maximum wins
static int32_t first_max(const unsigned long long *dc, int M, int64_t *counts) {
    int32_t best = 0;
    for (int m = 0; m < M; ++m) {
        counts[m] = (int64_t)dc[m];
        if (dc[m] > dc[best]) best = m;
    }
    return best;
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_two_view_select(const double *P1, const double *P2s, const double *R1, const double *C1,
                                   const double *Rs, const double *Cs, int32_t M, const double *x1,
                                   const double *x2, int64_t N, int64_t *counts, int32_t *best, double *X_best,
                                   double *X_all, int device) {
    SFM_CHECK_ARG(M >= 1 && M <= TV_MAX, "need 1 <= M <= 8 candidates");
    SFM_CHECK_ARG(N >= 0, "N < 0");
    SFM_CHECK_ARG(counts && best, "null pointer");
    if (N == 0) {
        for (int m = 0; m < M; ++m) counts[m] = 0;
        *best = 0;
        return 0;
    }
    SFM_CHECK_ARG(P1 && P2s && R1 && C1 && Rs && Cs && x1 && x2 && X_best, "null pointer");
    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    const size_t pb = (size_t)N * sizeof(double2), xb = (size_t)N * 24, cb = TV_MAX * sizeof(unsigned long long);
    int rc;
    if ((rc = c->buf[0].reserve(pb)) || (rc = c->buf[1].reserve(pb)) || (rc = c->buf[2].reserve((size_t)M * xb)) ||
        (rc = c->buf[3].reserve(cb)))
        return rc;
    TvProj P;
    TvCams cam;
    std::memset(&P, 0, sizeof P);
    std::memcpy(P.p1, P1, sizeof P.p1);
    std::memcpy(P.p2, P2s, (size_t)M * 12 * sizeof(double));
    fill_cams(cam, R1, C1, Rs, Cs, M);
    hipStream_t s = c->stream;
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_HIP(hipMemcpyAsync(c->buf[0].p, x1, pb, hipMemcpyHostToDevice, s));
    SFM_HIP(hipMemcpyAsync(c->buf[1].p, x2, pb, hipMemcpyHostToDevice, s));
    SFM_HIP(hipMemsetAsync(c->buf[3].p, 0, cb, s));
    SFM_TRY(tm.mark(s));
    hipLaunchKernelGGL(k_two_view_select, dim3(ceil_div(N, 256), M), dim3(256), 0, s, P, cam,
                       c->buf[0].as<double2>(), c->buf[1].as<double2>(), N, c->buf[2].as<double>(),
                       c->buf[3].as<unsigned long long>());
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    unsigned long long dc[TV_MAX];
    SFM_HIP(hipMemcpyAsync(dc, c->buf[3].p, cb, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    *best = first_max(dc, M, counts);
    // only the winner's points come back, all of them only on request
    SFM_HIP(hipMemcpyAsync(X_best, c->buf[2].as<char>() + (size_t)*best * xb, xb, hipMemcpyDeviceToHost, s));
    if (X_all) SFM_HIP(hipMemcpyAsync(X_all, c->buf[2].p, (size_t)M * xb, hipMemcpyDeviceToHost, s));
    return tm.finish(s);
}

extern "C" int sfm_cheirality_count(const double *R1, const double *C1, const double *Rs, const double *Cs,
                                    int32_t M, const double *Xset, int64_t N, int64_t *counts, int32_t *best,
                                    int device) {
    SFM_CHECK_ARG(M >= 1 && M <= TV_MAX, "need 1 <= M <= 8 candidates");
    SFM_CHECK_ARG(N >= 0, "N < 0");
    SFM_CHECK_ARG(counts && best, "null pointer");
    if (N == 0) {
        for (int m = 0; m < M; ++m) counts[m] = 0;
        *best = 0;
        return 0;
    }
    SFM_CHECK_ARG(R1 && C1 && Rs && Cs && Xset, "null pointer");
    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    const size_t xb = (size_t)M * N * 24, cb = TV_MAX * sizeof(unsigned long long);
    int rc;
    if ((rc = c->buf[2].reserve(xb)) || (rc = c->buf[3].reserve(cb))) return rc;
    TvCams cam;
    fill_cams(cam, R1, C1, Rs, Cs, M);
    hipStream_t s = c->stream;
    SFM_HIP(hipMemcpyAsync(c->buf[2].p, Xset, xb, hipMemcpyHostToDevice, s));
    SFM_HIP(hipMemsetAsync(c->buf[3].p, 0, cb, s));
    hipLaunchKernelGGL(k_cheirality_count, dim3(ceil_div(N, 256), M), dim3(256), 0, s, cam, c->buf[2].as<double>(), N,
                       c->buf[3].as<unsigned long long>());
    SFM_HIP(hipGetLastError());
    unsigned long long dc[TV_MAX];
    SFM_HIP(hipMemcpyAsync(dc, c->buf[3].p, cb, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    *best = first_max(dc, M, counts);
    return 0;
}
