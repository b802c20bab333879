// Batched initial-pair selection: for every verified image pair of a store, in
// one call, the relative pose from its fundamental matrix, the cheirality
// counts of the four pose candidates, the winner's points with their parallax
// angles and its exact median, and the support of the best 4-point homography
// -- what tells a wide-baseline pair from one without baseline or of a plane.
// The reference chooses nothing (Wrapper_dev.py:156-179 starts from images 1
// and 2); sfm_two_view_select serves one pair per call from candidates built on
// the host.  Differs on purpose.
//
//   k_ip_homog  the scaffold's grid, block table and tile loop (hyp_batch.hpp).
//               Fit: a thread per hypothesis (Hartley normalisation, the 8 x 9
//               DLT system in registers, its null vector by the Householder LQ,
//               denormalisation, unit norm).  Score: a wave per hypothesis, the
//               transfer error over tiles of 1024.
//   k_ip_pose   one workgroup per pair.  Thread 0: E = K^T F K, the one-sided
//               Jacobi of E^T, the four candidates and their projections, all
//               left in LDS.  Every thread: its correspondences i = t, t + 256,
//               ... triangulated under the four candidates (counts: a ballot
//               per wave, the waves' integers added), then again under the
//               winner for X, good and angle.  The median is a radix select
//               over the bit patterns of the good angles, eight bits a pass in
//               an LDS histogram of integer atomics.  Last, the winner of the
//               homography table.
//
// Counts are integers and every floating-point value is computed by one thread
// from quantities of the pair alone, so a pair's outputs do not depend on the
// batch it is in.
#include <cmath>
#include <cstring>

#include "epi_sampson.hpp"
#include "hyp_batch.hpp"
#include "select.hpp"
#include "triangulate_point.hpp"

namespace sfm {

constexpr int IP_THREADS = 256;  // both kernels
constexpr int IP_WAVES = IP_THREADS / 64;
constexpr int IP_HT = 64;        // most hypotheses per workgroup
constexpr int IP_TILE = 1024;    // correspondences per LDS tile (32 KiB)
static_assert(IP_THREADS == 256, "the radix select has one thread per histogram bin");

// ------------------------------------------------------------------ homography
// The normalised 4-point DLT under x2 ~ H x1: h_rows' two rows per point, the
// null vector of the 8 x 9 system, H = T2^-1 Hn T1 with T = [[s, 0, ox], [0, s,
// oy], [0, 0, 1]] (the zeros left out), then vp_unit: unit Frobenius norm, the
// entry of largest magnitude positive, no division by H[2,2].
__device__ __forceinline__ void ip_h4(const double (&x1)[4], const double (&y1)[4], const double (&x2)[4],
                                      const double (&y2)[4], double (&H)[9]) {
#pragma clang fp contract(off)
    const Hartley h1 = hartley_k<4>(x1, y1), h2 = hartley_k<4>(x2, y2);
    double A[8][9];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        h_rows(h1.s * x1[i] + h1.ox, h1.s * y1[i] + h1.oy, h2.s * x2[i] + h2.ox, h2.s * y2[i] + h2.oy, A[2 * i],
               A[2 * i + 1]);
    double n[9];
    null_vector_8x9(A, n);
    const double is = 1.0 / h2.s;
    double M[3][3], G[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        M[0][c] = (n[c] - h2.ox * n[6 + c]) * is;
        M[1][c] = (n[3 + c] - h2.oy * n[6 + c]) * is;
        M[2][c] = n[6 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = M[r][0] * h1.s;
        G[3 * r + 1] = M[r][1] * h1.s;
        G[3 * r + 2] = (M[r][0] * h1.ox + M[r][1] * h1.oy) + M[r][2];
    }
    vp_unit(G, H);
}

// h = H [x; y; 1]: an inlier where h2 is finite, |h2| >= 1e-12 and the squared
// transfer error is below thr2.  False for anything not finite.
__device__ __forceinline__ bool ip_h_inlier(const double *H, double x, double y, double u, double v, double thr2) {
#pragma clang fp contract(off)
    const double h0 = (H[0] * x + H[1] * y) + H[2];
    const double h1 = (H[3] * x + H[4] * y) + H[5];
    const double h2 = (H[6] * x + H[7] * y) + H[8];
    if (!(isfinite(h2) && fabs(h2) >= 1e-12)) return false;
    const double du = u - h0 / h2, dv = v - h1 / h2;
    return du * du + dv * dv < thr2;
}

// Live pairs: n_p >= 8.  models (P x Hh x 9); counts (P x Hh).
__global__ void __launch_bounds__(IP_THREADS)
k_ip_homog(const int64_t *__restrict__ pair_start, const double2 *__restrict__ x1, const double2 *__restrict__ x2,
           const int32_t *__restrict__ samples, int32_t Hh, const int32_t *__restrict__ blk_start,
           const int32_t *__restrict__ tab, int32_t n_live, double thr, double *__restrict__ models,
           int32_t *__restrict__ counts) {
    __shared__ double sH[IP_HT][9];
    __shared__ double2 s1[IP_TILE];
    __shared__ double2 s2[IP_TILE];
    __shared__ int32_t sCnt[IP_HT];
    const int tid = threadIdx.x;
    const HypTile t = tile_of_block(blk_start, tab, n_live, Hh);
    const int nh = t.nh;
    const int64_t ps = pair_start[t.row];
    const int n = (int)(pair_start[t.row + 1] - ps);
    const int64_t row0 = (int64_t)t.row * Hh + t.hb;

    // ---- fit: a thread per hypothesis (nh <= IP_HT <= IP_THREADS)
    if (tid < nh) {
        double a[4], b[4], c[4], d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t j = ps + samples[(row0 + tid) * 4 + k];
            const double2 q1 = x1[j], q2 = x2[j];
            a[k] = q1.x; b[k] = q1.y; c[k] = q2.x; d[k] = q2.y;
        }
        double H[9];
        ip_h4(a, b, c, d, H);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            sH[tid][k] = H[k];
            models[(row0 + tid) * 9 + k] = H[k];
        }
        sCnt[tid] = 0;
    }
    __syncthreads();

    // ---- score: a wave per hypothesis, the pair's tile shared by all of them
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double thr2 = thr * thr;
    for_each_tile<IP_THREADS, IP_TILE>(
        n, [&](int i, int c) { s1[i] = x1[ps + c], s2[i] = x2[ps + c]; },
        [&](int nt) {
            for (int hl = wave; hl < nh; hl += IP_WAVES) {
                double H[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) H[j] = sH[hl][j];
                const int cnt = wave_count(nt, [&](int i) {
                    const double2 q1 = s1[i], q2 = s2[i];
                    return ip_h_inlier(H, q1.x, q1.y, q2.x, q2.y, thr2);
                });
                if (lane == 0) sCnt[hl] += cnt;  // this wave alone owns hl
            }
        });
    if (tid < nh) counts[row0 + tid] = sCnt[tid];
}

// ------------------------------------------------------------------ pose
// The four candidates of F, by one thread, into LDS: cand (4 x 12: R row-major,
// then t), P2 (4 x 12: K [R | t]), Cc (4 x 3: -R^T t); tmp: 18 doubles.  One-sided
// Jacobi on E^T (its columns are the rows of E) leaves U in the accumulated
// rotations -- the left singular vector of the least singular value with them --
// and sigma_j v_j in the columns; v3 = v1 x v2.  With (1, 2, 3) the two larger
// singular values in cyclic order after the least,
//   U W V^T = u2 v1^T - u1 v2^T + u3 v3^T,  U W^T V^T = -u2 v1^T + u1 v2^T + u3 v3^T.
// False where F or E is not finite or the second singular value is 0.
__device__ __forceinline__ bool ip_candidates(const double *K, const double *F, double *cand, double *P2, double *Cc,
                                              double *tmp) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && isfinite(F[k]) && isfinite(K[k]);
    double a[3][3], V[3][3];  // a[j][k] = E[j][k]: column j of E^T
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
                acc += K[3 * i + r] * ((F[3 * i] * K[c] + F[3 * i + 1] * K[3 + c]) + F[3 * i + 2] * K[6 + c]);
            a[r][c] = acc;
            fin = fin && isfinite(acc);
        }
    if (!fin) return false;
    jacobi_onesided<3, 3, 40>(a, V);
    const int z = weakest_column<3, 3>(a);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tmp[3 * j + k] = a[j][k];      // sigma_j v_j
            tmp[9 + 3 * j + k] = V[k][j];  // u_j
        }
    const int i1 = (z + 1) % 3, i2 = (z + 2) % 3;
    double v1[3], v2[3], u1[3], u2[3], u3[3];
    double n1 = 0.0, n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v1[k] = tmp[3 * i1 + k]; v2[k] = tmp[3 * i2 + k];
        u1[k] = tmp[9 + 3 * i1 + k]; u2[k] = tmp[9 + 3 * i2 + k]; u3[k] = tmp[9 + 3 * z + k];
        n1 += v1[k] * v1[k]; n2 += v2[k] * v2[k];
    }
    n1 = sqrt(n1); n2 = sqrt(n2);
    if (!(isfinite(n1) && isfinite(n2) && n1 > 0.0 && n2 > 0.0)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) { v1[k] = v1[k] / n1; v2[k] = v2[k] / n2; }
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const double sg = m == 0 ? 1.0 : -1.0;
        double R[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[3 * r + c] = sg * (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                           R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (det < 0.0)
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = -R[k];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int q = 2 * m + s;
            double t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = s == 0 ? u3[k] : -u3[k];
#pragma unroll
            for (int k = 0; k < 9; ++k) cand[12 * q + k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cand[12 * q + 9 + k] = t[k];
                Cc[3 * q + k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    P2[12 * q + 4 * r + c] = (K[3 * r] * R[c] + K[3 * r + 1] * R[3 + c]) + K[3 * r + 2] * R[6 + c];
                P2[12 * q + 4 * r + 3] = (K[3 * r] * t[0] + K[3 * r + 1] * t[1]) + K[3 * r + 2] * t[2];
            }
        }
    }
    return true;
}

// squared reprojection error of X under P (3 x 4) against (u, v); NaN or inf
// where the third coordinate is 0
__device__ __forceinline__ double ip_reproj2(const double *P, const double (&X)[3], double2 q) {
#pragma clang fp contract(off)
    const double h0 = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const double h1 = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    const double h2 = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    const double du = q.x - h0 / h2, dv = q.y - h1 / h2;
    return du * du + dv * dv;
}

struct IpOut {
    double *R, *C;          // P x 9, P x 3
    int64_t *counts;        // P x 4
    int32_t *best, *n_good;
    double *median;
    int32_t *h_count, *h_best;
    double *Hbest;          // P x 9
    int32_t *info;
    double *X;              // n_corr x 3
    uint8_t *good;          // n_corr
    double *angle;          // n_corr
    double *cands;          // P x 48
};

// One workgroup per pair.  Pairs of fewer than eight correspondences are the
// host's (info -1): nothing of them is read.
__global__ void __launch_bounds__(IP_THREADS)
k_ip_pose(const double *__restrict__ Kmat, const int64_t *__restrict__ pair_start, const double2 *__restrict__ x1,
          const double2 *__restrict__ x2, const double *__restrict__ Fs, int32_t Hh,
          const int32_t *__restrict__ hcounts, const double *__restrict__ hmodels, double max_reproj, IpOut o) {
    __shared__ double sK[9], sP1[12], sCand[4][12], sP2[4][12], sC[4][3], sTmp[18];
    __shared__ int32_t sOk, sCnt[IP_WAVES][4], sGood[IP_WAVES], sW[IP_WAVES], sSel, sRank;
    __shared__ int32_t hist[IP_THREADS];
    __shared__ int32_t sc[IP_WAVES];
    __shared__ int64_t sh[IP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t p = blockIdx.x;
    const int64_t ps = pair_start[p];
    const int n = (int)(pair_start[p + 1] - ps);
    if (n < 8) return;

    // ---- the homography table's winner (the scores are k_ip_homog's)
    int32_t hc = 0;
    int64_t hb = -1;
    if (Hh > 0) wg_select_best<IP_THREADS>(hcounts + p * Hh, Hh, sc, sh, hc, hb);  // holds a barrier
    if (tid < 9) o.Hbest[9 * p + tid] = hb >= 0 ? hmodels[(p * Hh + hb) * 9 + tid] : 0.0;
    if (tid == 0) {
        o.h_count[p] = hb >= 0 ? hc : 0;
        o.h_best[p] = (int32_t)hb;
    }

    // ---- candidates
    if (tid < IP_WAVES * 4) sCnt[tid >> 2][tid & 3] = 0;
    hist[tid] = 0;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) sK[k] = Kmat[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sP1[4 * r + c] = sK[3 * r + c];
            sP1[4 * r + 3] = 0.0;
        }
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = Fs[9 * p + k];
        sOk = ip_candidates(sK, F, &sCand[0][0], &sP2[0][0], &sC[0][0], sTmp) ? 1 : 0;
    }
    __syncthreads();
    const bool ok = sOk != 0;
    if (tid < 48) o.cands[48 * p + tid] = ok ? sCand[tid / 12][tid % 12] : 0.0;
    if (!ok) {  // info -2: the outputs of a pair that is not processed
        for (int i = tid; i < n; i += IP_THREADS) {
            double *xo = o.X + 3 * (ps + i);
            xo[0] = 0.0; xo[1] = 0.0; xo[2] = 0.0;
            o.good[ps + i] = 0;
            o.angle[ps + i] = 0.0;
        }
        if (tid < 9) o.R[9 * p + tid] = tid % 4 == 0 ? 1.0 : 0.0;
        if (tid < 3) o.C[3 * p + tid] = 0.0;
        if (tid < 4) o.counts[4 * p + tid] = 0;
        if (tid == 0) {
            o.best[p] = 0;
            o.n_good[p] = 0;
            o.median[p] = 0.0;
            o.info[p] = -2;
        }
        return;
    }

    // ---- cheirality: every correspondence under every candidate
    const double r1[3] = {0.0, 0.0, 1.0}, c1[3] = {0.0, 0.0, 0.0};
    for (int base = 0; base < n; base += IP_THREADS) {
        const int i = base + tid;
        double2 u = make_double2(0.0, 0.0), v = u;
        if (i < n) {
            u = x1[ps + i];
            v = x2[ps + i];
        }
#pragma unroll 1
        for (int m = 0; m < 4; ++m) {
            bool front = false;
            if (i < n) {
                double X[3];
                triangulate_point(sP1, sP2[m], u, v, X);
                front = in_front_of_both(r1, c1, &sCand[m][6], sC[m], X);
            }
            const int c = __popcll(__ballot(front));
            if (lane == 0) sCnt[wave][m] += c;  // this wave alone owns its row
        }
    }
    __syncthreads();
    int tot[4], best = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        tot[m] = 0;
#pragma unroll
        for (int w = 0; w < IP_WAVES; ++w) tot[m] += sCnt[w][m];
    }
    {
        int bc = tot[0];
#pragma unroll
        for (int m = 1; m < 4; ++m)
            if (tot[m] > bc) { bc = tot[m]; best = m; }
    }

    // ---- the winner's points
    const double mr2 = max_reproj * max_reproj;
    const double *Pb = sP2[best], *rb = &sCand[best][6], *cb = sC[best];
    int ng = 0;
    for (int base = 0; base < n; base += IP_THREADS) {
        const int i = base + tid;
        bool good = false;
        if (i < n) {
            const double2 u = x1[ps + i], v = x2[ps + i];
            double X[3];
            triangulate_point(sP1, Pb, u, v, X);
            good = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && in_front_of_both(r1, c1, rb, cb, X);
            if (good) good = ip_reproj2(sP1, X, u) < mr2 && ip_reproj2(Pb, X, v) < mr2;
            double ang = 0.0;
            if (good) {
#pragma clang fp contract(off)
                const double b0 = X[0] - cb[0], b1 = X[1] - cb[1], b2 = X[2] - cb[2];
                const double k0 = X[1] * b2 - X[2] * b1, k1 = X[2] * b0 - X[0] * b2, k2 = X[0] * b1 - X[1] * b0;
                ang = atan2(sqrt((k0 * k0 + k1 * k1) + k2 * k2), (X[0] * b0 + X[1] * b1) + X[2] * b2);
                if (!(ang >= 0.0)) ang = 0.0;  // an overflow inside the products: no angle
            }
            double *xo = o.X + 3 * (ps + i);
            xo[0] = X[0]; xo[1] = X[1]; xo[2] = X[2];
            o.good[ps + i] = good ? 1 : 0;
            o.angle[ps + i] = ang;
        }
        ng += __popcll(__ballot(good));
    }
    if (lane == 0) sGood[wave] = ng;
    __syncthreads();
    int n_good = 0;
#pragma unroll
    for (int w = 0; w < IP_WAVES; ++w) n_good += sGood[w];

    // ---- the lower median of the good angles: non-negative doubles order as
    // their bit patterns, so the element of sorted index k is found eight bits
    // a pass, from the top: a histogram of the next byte over the values that
    // share the prefix found so far, and the bin that holds rank k.  A thread
    // reads back the angles it wrote itself (i = t, t + 256, ...).
    unsigned long long prefix = 0;
    if (n_good > 0) {
        int k = (n_good - 1) / 2;
        for (int pass = 7; pass >= 0; --pass) {
            const int shift = 8 * pass;
            for (int i = tid; i < n; i += IP_THREADS) {
                if (!o.good[ps + i]) continue;
                const unsigned long long b = (unsigned long long)__double_as_longlong(o.angle[ps + i]);
                if (pass == 7 || ((b ^ prefix) >> (shift + 8)) == 0) atomicAdd(&hist[(b >> shift) & 255], 1);
            }
            __syncthreads();
            const int c = hist[tid];
            hist[tid] = 0;
            int inc = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(inc, d);
                if (lane >= d) inc += t;
            }
            if (lane == 63) sW[wave] = inc;
            __syncthreads();
            int excl = inc - c;
            for (int w = 0; w < wave; ++w) excl += sW[w];
            if (c > 0 && excl <= k && k < excl + c) {  // one thread
                sSel = tid;
                sRank = k - excl;
            }
            __syncthreads();
            prefix |= (unsigned long long)sSel << shift;
            k = sRank;
        }
    }

    if (tid < 9) o.R[9 * p + tid] = sCand[best][tid];
    if (tid < 3) o.C[3 * p + tid] = cb[tid];
    if (tid < 4) o.counts[4 * p + tid] = tot[0] * (tid == 0) + tot[1] * (tid == 1) + tot[2] * (tid == 2) + tot[3] * (tid == 3);
    if (tid == 0) {
        o.best[p] = best;
        o.n_good[p] = n_good;
        o.median[p] = __longlong_as_double((long long)prefix);
        o.info[p] = 0;
    }
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_init_pairs(const double *K, const int64_t *pair_start, int64_t P, const double *x1,
                              const double *x2, int64_t n_corr, const double *F, const int32_t *hsamples, int64_t Hh,
                              double h_threshold, double max_reproj, double *R, double *C, int64_t *counts,
                              int32_t *best, int32_t *n_good, double *median_angle, int32_t *h_count,
                              int32_t *h_best, double *Hbest, int32_t *info, double *X, uint8_t *good, double *angle,
                              double *cands, int32_t *hcounts, double *hmodels, int device) {
    SFM_CHECK_ARG(P >= 0 && n_corr >= 0, "P < 0 or n_corr < 0");
    SFM_CHECK_ARG(Hh >= 0 && Hh <= (int64_t)1 << 20, "Hh must lie in [0, 2^20]");
    SFM_CHECK_ARG((hsamples == nullptr) == (Hh == 0), "hsamples must be null exactly when Hh is 0");
    SFM_CHECK_ARG(std::isfinite(h_threshold) && h_threshold > 0.0, "h_threshold must be finite and positive");
    SFM_CHECK_ARG(std::isfinite(max_reproj) && max_reproj > 0.0, "max_reproj must be finite and positive");
    SFM_CHECK_ARG(Hh == 0 || P < (int64_t)0x7fffffff / Hh, "P x Hh too large for one call");
    SFM_CHECK_ARG(K && pair_start, "null pointer");
    SFM_TRY(check_csr(pair_start, P, n_corr, "pair_start", "correspondence", 0x7fffffff,
                      "a pair has too many correspondences"));
    SFM_CHECK_ARG(n_corr == 0 || (x1 && x2), "null pointer");
    SFM_CHECK_ARG(P == 0 || F, "null pointer");
    // a pair's samples are checked from four correspondences on; it is live from eight
    SFM_TRY(check_samples(pair_start, P, hsamples, Hh, 4, 4, "sample outside [0, n_p)"));
    const int64_t n_live = count_live(pair_start, P, 8);
    if (P == 0) return 0;
    SFM_CHECK_ARG(R && C && counts && best && n_good && median_angle && h_count && h_best && Hbest && info &&
                      ((X && good && angle) || n_corr == 0),
                  "null pointer");
    // info -1: fewer than eight correspondences
    for (int64_t p = 0; p < P; ++p) {
        if (pair_start[p + 1] - pair_start[p] >= 8) continue;
        for (int j = 0; j < 9; ++j) {
            R[9 * p + j] = j % 4 == 0 ? 1.0 : 0.0;
            Hbest[9 * p + j] = 0.0;
        }
        for (int j = 0; j < 3; ++j) C[3 * p + j] = 0.0;
        for (int j = 0; j < 4; ++j) counts[4 * p + j] = 0;
        best[p] = 0;
        n_good[p] = 0;
        median_angle[p] = 0.0;
        h_count[p] = 0;
        h_best[p] = -1;
        info[p] = -1;
        for (int64_t k = pair_start[p]; k < pair_start[p + 1]; ++k) {
            X[3 * k] = X[3 * k + 1] = X[3 * k + 2] = 0.0;
            good[k] = 0;
            angle[k] = 0.0;
        }
        if (cands) std::memset(cands + p * 48, 0, 48 * sizeof(double));
        if (hcounts) std::memset(hcounts + p * Hh, 0, (size_t)Hh * sizeof(int32_t));
        if (hmodels) std::memset(hmodels + p * Hh * 9, 0, (size_t)Hh * 9 * sizeof(double));
    }
    if (n_live == 0) return 0;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    TileTable tt;  // of the homography kernel
    SFM_TRY(tt.build(c->pinned, n_live, pair_start, P, 8, Hh, IP_HT, IP_TILE));

    const size_t PH = (size_t)P * (size_t)Hh;
    Pack in(c->buf[0]), out(c->buf[1]);
    const auto i_K = in.add<double>(9), i_F = in.add<double>(9 * P);
    const auto i_ps = in.add<int64_t>(P + 1);
    const auto i_x1 = in.add<double2>(n_corr), i_x2 = in.add<double2>(n_corr);
    const auto i_s = in.add<int32_t>(4 * PH);
    const auto i_t = in.add<int32_t>(tt.words());  // the block table
    const auto o_R = out.add<double>(9 * P), o_C = out.add<double>(3 * P), o_med = out.add<double>(P);
    const auto o_Hb = out.add<double>(9 * P), o_cands = out.add<double>(48 * P);
    const auto o_cnt = out.add<int64_t>(4 * P);
    const auto o_best = out.add<int32_t>(P), o_ng = out.add<int32_t>(P), o_hc = out.add<int32_t>(P);
    const auto o_hb = out.add<int32_t>(P), o_info = out.add<int32_t>(P);
    const auto o_X = out.add<double>(3 * n_corr), o_ang = out.add<double>(n_corr);
    const auto o_good = out.add<uint8_t>(n_corr);
    const auto o_hcnt = out.add<int32_t>(PH);
    const auto o_hm = out.add<double>(9 * PH);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    hipStream_t s = c->stream;
    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_K, K, s));
    SFM_TRY(in.upload(i_F, F, s));
    SFM_TRY(in.upload(i_ps, pair_start, s));
    SFM_TRY(in.upload(i_x1, x1, s));
    SFM_TRY(in.upload(i_x2, x2, s));
    SFM_TRY(in.upload(i_s, hsamples, s));
    SFM_TRY(in.upload(i_t, tt.blk, s));
    SFM_TRY(tm.mark(s));
    if (Hh > 0) {
        hipLaunchKernelGGL(k_ip_homog, dim3((unsigned)tt.blocks), dim3(IP_THREADS), 0, s, in.ptr(i_ps), in.ptr(i_x1),
                           in.ptr(i_x2), in.ptr(i_s), (int32_t)Hh, in.ptr(i_t), in.ptr(i_t, n_live + 1),
                           (int32_t)n_live, h_threshold, out.ptr(o_hm), out.ptr(o_hcnt));
        SFM_HIP(hipGetLastError());
    }
    SFM_TRY(tm.split(s));  // [3]: the homography kernel alone
    const IpOut o{out.ptr(o_R),  out.ptr(o_C),  out.ptr(o_cnt), out.ptr(o_best), out.ptr(o_ng),
                  out.ptr(o_med), out.ptr(o_hc), out.ptr(o_hb),  out.ptr(o_Hb),   out.ptr(o_info),
                  out.ptr(o_X),  out.ptr(o_good), out.ptr(o_ang), out.ptr(o_cands)};
    hipLaunchKernelGGL(k_ip_pose, dim3((unsigned)P), dim3(IP_THREADS), 0, s, in.ptr(i_K), in.ptr(i_ps), in.ptr(i_x1),
                       in.ptr(i_x2), in.ptr(i_F), (int32_t)Hh, out.ptr(o_hcnt), out.ptr(o_hm), max_reproj, o);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));
    SFM_TRY(for_each_live_run(pair_start, P, 8, [&](int64_t p0, int64_t p1, int64_t k0, int64_t k1) -> int {
        SFM_TRY(out.download_rows(R, o_R, 9, p0, p1, s));
        SFM_TRY(out.download_rows(C, o_C, 3, p0, p1, s));
        SFM_TRY(out.download_rows(counts, o_cnt, 4, p0, p1, s));
        SFM_TRY(out.download_rows(best, o_best, 1, p0, p1, s));
        SFM_TRY(out.download_rows(n_good, o_ng, 1, p0, p1, s));
        SFM_TRY(out.download_rows(median_angle, o_med, 1, p0, p1, s));
        SFM_TRY(out.download_rows(h_count, o_hc, 1, p0, p1, s));
        SFM_TRY(out.download_rows(h_best, o_hb, 1, p0, p1, s));
        SFM_TRY(out.download_rows(Hbest, o_Hb, 9, p0, p1, s));
        SFM_TRY(out.download_rows(info, o_info, 1, p0, p1, s));
        SFM_TRY(out.download_rows(X, o_X, 3, k0, k1, s));
        SFM_TRY(out.download_rows(good, o_good, 1, k0, k1, s));
        SFM_TRY(out.download_rows(angle, o_ang, 1, k0, k1, s));
        SFM_TRY(out.download_rows(cands, o_cands, 48, p0, p1, s));
        SFM_TRY(out.download_rows(hcounts, o_hcnt, Hh, p0, p1, s));
        return out.download_rows(hmodels, o_hm, 9 * Hh, p0, p1, s);
    }));
    return tm.finish(s);
}
