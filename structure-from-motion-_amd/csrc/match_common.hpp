// What descriptor matching (match_descriptors.hip) and guided matching
// (match_guided.hip) share: the tile constants, the norms kernel, the merge of
// two running top-2 states, the acceptance tests and the compaction, with the
// host code in front of and behind the nearest-neighbour kernels.  The kernels
// are the ones match_descriptors.hip describes; only the nearest-neighbour
// kernel differs between the two entry points.
#pragma once
#include <climits>
#include <cmath>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "staging.hpp"

namespace sfm {

constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = 4;
constexpr int MD_MS = 2;                       // 16-row subtiles per wave
constexpr int MD_BM = MD_WAVES * MD_MS * 16;   // rows of a workgroup
constexpr int MD_TN = 64;                      // columns of an LDS tile
constexpr int MD_PAD = 16;                     // bytes after each LDS row
constexpr int32_t MD_NONE = INT32_MAX;
constexpr int32_t MD_OUTSIDE = INT32_MAX - (1 << 24);  // norm of a column past the end: w stays >= 2^30
constexpr int32_t MD_VALID = 1 << 30;                  // every real w is far below
constexpr int64_t MD_MAX_KP = (int64_t)1 << 20;

typedef int md_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int md_sq4(uint32_t v) {  // sum of squares of four signed bytes
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = (int)(int8_t)(v >> (8 * k));
        s += b * b;
    }
    return s;
}

// norm[kp] = || desc[kp] - 128 ||^2; DIM / 16 threads per keypoint
template <int DIM>
__global__ __launch_bounds__(MD_THREADS) void k_md_norms(const uint8_t *desc, int64_t n_kp, int32_t *norm) {
    constexpr int CH = DIM / 16;
    const int64_t g = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    const int64_t kp = g / CH;
    int s = 0;
    if (kp < n_kp) {
        const uint4 v = *reinterpret_cast<const uint4 *>(desc + g * 16);
        s = md_sq4(v.x ^ 0x80808080u) + md_sq4(v.y ^ 0x80808080u) + md_sq4(v.z ^ 0x80808080u) +
            md_sq4(v.w ^ 0x80808080u);
    }
#pragma unroll
    for (int o = 1; o < CH; o <<= 1) s += __shfl_xor(s, o);
    if (kp < n_kp && g % CH == 0) norm[kp] = s;
}

// merge the running (m1, i1, m2) of another lane into this one's, by (w, column)
__device__ __forceinline__ void md_merge(int32_t &m1, int32_t &i1, int32_t &m2, int32_t om1, int32_t oi1, int32_t om2) {
    const bool other = om1 < m1 || (om1 == m1 && oi1 < i1);
    const int32_t lo2 = other ? om2 : m2, hi1 = other ? m1 : om1;
    m2 = lo2 < hi1 ? lo2 : hi1;
    m1 = other ? om1 : m1;
    i1 = other ? oi1 : i1;
}

// The nearest-neighbour pass that match_descriptors.hip describes (k_md_nn
// there): sfm_match_descriptors instantiates it for image pairs, and
// retrieval.hip for blocks of descriptors against a vocabulary's centres.
// pairs is (first, second) per pair when !SWAP and read as (second, first) when
// SWAP; row_off[p] is where the pair's rows start in nn / d1 / d2.
template <int DIM, bool SWAP>
__global__ __launch_bounds__(MD_THREADS) void k_md_nn(const uint8_t *__restrict__ desc, const int32_t *__restrict__ norm,
                                                      const int64_t *__restrict__ img_start,
                                                      const int32_t *__restrict__ pairs, int64_t P,
                                                      const int64_t *__restrict__ row_off, int32_t *__restrict__ nn,
                                                      int32_t *__restrict__ d1, int32_t *__restrict__ d2) {
    constexpr int KS = DIM / 64;                          // k steps
    constexpr int STRIDE = DIM + MD_PAD;                  // bytes of an LDS row
    constexpr int CH = DIM / 16;                          // 16-byte chunks per row
    constexpr int NQ = MD_TN * CH / MD_THREADS;           // chunks a thread stages per tile
    static_assert(MD_TN * CH % MD_THREADS == 0, "a tile is a whole number of passes");
    __shared__ __attribute__((aligned(16))) uint8_t sB[2][MD_TN * STRIDE];
    __shared__ int32_t sNb[2][MD_TN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    for (int64_t p = blockIdx.y; p < P; p += gridDim.y) {
        const int32_t ii = pairs[2 * p + (SWAP ? 1 : 0)], jj = pairs[2 * p + (SWAP ? 0 : 1)];
        const int64_t is = img_start[ii], js = img_start[jj];
        const int32_t ni = (int32_t)(img_start[ii + 1] - is), nj = (int32_t)(img_start[jj + 1] - js);
        const int32_t row0 = (int32_t)blockIdx.x * MD_BM;
        if (row0 >= ni) continue;  // uniform over the workgroup
        const int32_t wrow0 = row0 + wave * (MD_MS * 16);

        // this wave's rows, biased, in registers
        md_v4i a[MD_MS][KS];
#pragma unroll
        for (int ms = 0; ms < MD_MS; ++ms) {
            const int32_t r = wrow0 + ms * 16 + lr;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                md_v4i v = {0, 0, 0, 0};
                if (r < ni) {
                    v = *reinterpret_cast<const md_v4i *>(desc + (is + r) * DIM + ks * 64 + lk * 16);
                    v ^= (int)0x80808080;
                }
                a[ms][ks] = v;
            }
        }
        int32_t m1[MD_MS][4], i1[MD_MS][4], m2[MD_MS][4];
#pragma unroll
        for (int ms = 0; ms < MD_MS; ++ms)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m1[ms][j] = MD_NONE;
                m2[ms][j] = MD_NONE;
                i1[ms][j] = -1;
            }

        const int32_t ntiles = (nj + MD_TN - 1) / MD_TN;
        md_v4i st[NQ];
        int32_t st_nb = MD_OUTSIDE;
        // tile t of the second image: global -> registers, registers -> LDS buffer
        auto fetch = [&](int32_t t) {
            const int32_t c0 = t * MD_TN;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = tid + q * MD_THREADS, col = c / CH, kc = c % CH;
                md_v4i v = {0, 0, 0, 0};
                if (c0 + col < nj) {
                    v = *reinterpret_cast<const md_v4i *>(desc + (js + c0 + col) * DIM + kc * 16);
                    v ^= (int)0x80808080;
                }
                st[q] = v;
            }
            if (tid < MD_TN) st_nb = c0 + tid < nj ? norm[js + c0 + tid] : MD_OUTSIDE;
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = tid + q * MD_THREADS, col = c / CH, kc = c % CH;
                *reinterpret_cast<md_v4i *>(&sB[buf][col * STRIDE + kc * 16]) = st[q];
            }
            if (tid < MD_TN) sNb[buf][tid] = st_nb;
        };

        __syncthreads();  // the previous pair's last tile is no longer read
        if (ntiles > 0) {
            fetch(0);
            stash(0);
        }
        __syncthreads();
        for (int32_t t = 0; t < ntiles; ++t) {
            const int cur = t & 1;
            if (t + 1 < ntiles) fetch(t + 1);
#pragma unroll
            for (int ns = 0; ns < MD_TN / 16; ++ns) {
                md_v4i b[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    b[ks] = *reinterpret_cast<const md_v4i *>(&sB[cur][(ns * 16 + lr) * STRIDE + ks * 64 + lk * 16]);
                const int32_t nb = sNb[cur][ns * 16 + lr];
                const int32_t col = t * MD_TN + ns * 16 + lr;
#pragma unroll
                for (int ms = 0; ms < MD_MS; ++ms) {
                    md_v4i acc = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ms][ks], b[ks], acc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int32_t w = nb - 2 * acc[j];
                        const int32_t lo = m1[ms][j];
                        // the second smallest so far: the median of (m1 <= m2, w)
                        m2[ms][j] = min(m2[ms][j], max(lo, w));
                        i1[ms][j] = w < lo ? col : i1[ms][j];
                        m1[ms][j] = min(lo, w);
                    }
                }
            }
            if (t + 1 < ntiles) stash(cur ^ 1);
            __syncthreads();
        }

        // the 16 lanes that share a row (the same lane >> 4), then the row's outputs
#pragma unroll
        for (int ms = 0; ms < MD_MS; ++ms)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int32_t x1 = m1[ms][j], xi = i1[ms][j], x2 = m2[ms][j];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const int32_t o1 = __shfl_xor(x1, o), oi = __shfl_xor(xi, o), o2 = __shfl_xor(x2, o);
                    md_merge(x1, xi, x2, o1, oi, o2);
                }
                const int32_t r = wrow0 + ms * 16 + lk * 4 + j;
                if (lr == 0 && r < ni) {
                    const int32_t na = norm[is + r];
                    const bool has1 = x1 < MD_VALID, has2 = x2 < MD_VALID;
                    const int64_t o = row_off[p] + r;
                    nn[o] = has1 ? xi : -1;
                    if (d1) d1[o] = has1 ? na + x1 : MD_NONE;
                    if (d2) d2[o] = has2 ? na + x2 : MD_NONE;
                }
            }
    }
}

// flag[row_off[p] + a] = 1 when keypoint a of the pair's first image is matched
static __global__ __launch_bounds__(MD_THREADS) void k_md_accept(const int64_t *img_start, const int32_t *pairs,
                                                                 int64_t P, const int64_t *row_off,
                                                                 const int64_t *col_off, const int32_t *nn,
                                                                 const int32_t *d1, const int32_t *d2,
                                                                 const int32_t *nn_rev, double ratio_sq,
                                                                 int32_t max_dsq, int32_t *flag) {
    for (int64_t p = blockIdx.y; p < P; p += gridDim.y) {
        const int32_t ii = pairs[2 * p];
        const int32_t ni = (int32_t)(img_start[ii + 1] - img_start[ii]);
        const int32_t a = (int32_t)blockIdx.x * MD_THREADS + threadIdx.x;
        if (a >= ni) continue;
        const int64_t o = row_off[p] + a;
        const int32_t b = nn[o], e1 = d1[o], e2 = d2[o];
        bool ok = b >= 0 && e1 <= max_dsq;
        ok = ok && (e2 == MD_NONE || (double)e1 < ratio_sq * (double)e2);
        ok = ok && (!nn_rev || nn_rev[col_off[p] + b] == a);
        flag[o] = ok ? 1 : 0;
    }
}

static __global__ __launch_bounds__(MD_THREADS) void k_md_write(const int64_t *img_start, const int32_t *pairs,
                                                                int64_t P, const int64_t *row_off, const int32_t *nn,
                                                                const int32_t *d1, const int32_t *flag,
                                                                const int64_t *place, int64_t *match_start,
                                                                int32_t *match_a, int32_t *match_b,
                                                                int32_t *match_dsq) {
    for (int64_t p = blockIdx.y; p < P; p += gridDim.y) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            match_start[p] = place[row_off[p]];
            if (p == P - 1) match_start[P] = place[row_off[P]];
        }
        const int32_t ii = pairs[2 * p];
        const int32_t ni = (int32_t)(img_start[ii + 1] - img_start[ii]);
        const int32_t a = (int32_t)blockIdx.x * MD_THREADS + threadIdx.x;
        if (a >= ni) continue;
        const int64_t o = row_off[p] + a;
        if (!flag[o]) continue;
        const int64_t m = place[o];
        match_a[m] = a;
        match_b[m] = nn[o];
        match_dsq[m] = d1[o];
    }
}

#define MD_LAUNCH(kernel, grid, ...)                                          \
    do {                                                                      \
        hipLaunchKernelGGL(kernel, grid, dim3(MD_THREADS), 0, s, __VA_ARGS__); \
        SFM_HIP(hipGetLastError());                                           \
    } while (0)
#define MD_BY_DIM(launch)        \
    do {                         \
        if (dim == 64) {         \
            launch(64);          \
        } else if (dim == 128) { \
            launch(128);         \
        } else {                 \
            launch(256);         \
        }                        \
    } while (0)

// The pairs' extents in the pair-major arrays after the argument checks that
// both entry points share; host only, nothing written on a refusal.
struct MdPlan {
    std::vector<int64_t> off;  // row_off (P + 1) then col_off (P + 1)
    int64_t max_i = 0, max_j = 0;
    const int64_t *row_off() const { return off.data(); }
    const int64_t *col_off() const { return off.data() + off.size() / 2; }
};

inline int md_plan(const uint8_t *desc, int64_t n_kp, const int64_t *img_start, int32_t n_images, int32_t dim,
                   const int32_t *pairs, int64_t P, double ratio, int32_t max_dsq, int32_t cross_check,
                   int64_t capacity, const int64_t *match_start, const int32_t *match_a, const int32_t *match_b,
                   const int32_t *match_dsq, MdPlan &plan) {
    SFM_CHECK_ARG(n_kp >= 0 && n_images >= 0 && P >= 0 && capacity >= 0, "n_kp, n_images, P or capacity < 0");
    SFM_CHECK_ARG(dim == 64 || dim == 128 || dim == 256, "dim is not 64, 128 or 256");
    SFM_CHECK_ARG(std::isfinite(ratio) && ratio > 0.0 && ratio <= 1.0, "ratio outside (0, 1]");
    SFM_CHECK_ARG(max_dsq >= 0, "max_dsq < 0");
    SFM_CHECK_ARG(cross_check == 0 || cross_check == 1, "cross_check is not 0 or 1");
    SFM_CHECK_ARG(img_start && match_start, "null pointer");
    SFM_CHECK_ARG(n_kp == 0 || desc, "null pointer");
    SFM_CHECK_ARG(P == 0 || pairs, "null pointer");
    SFM_CHECK_ARG(capacity == 0 || (match_a && match_b && match_dsq), "null pointer");
    SFM_TRY(check_csr(img_start, n_images, n_kp, "img_start", "keypoint", MD_MAX_KP,
                      "an image with more than 2^20 keypoints"));
    // the pairs' extents in the pair-major arrays, and the bound on the matches
    plan.off.assign(2 * (size_t)(P + 1), 0);
    int64_t *row_off = plan.off.data(), *col_off = plan.off.data() + (P + 1);
    int64_t bound = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
        SFM_CHECK_ARG(i >= 0 && i < n_images && j >= 0 && j < n_images, "a pair image outside [0, n_images)");
        SFM_CHECK_ARG(i != j, "a pair of an image with itself");
        const int64_t ni = img_start[i + 1] - img_start[i], nj = img_start[j + 1] - img_start[j];
        row_off[p + 1] = row_off[p] + ni;
        col_off[p + 1] = col_off[p] + nj;
        bound += cross_check && nj < ni ? nj : ni;
        if (ni > plan.max_i) plan.max_i = ni;
        if (nj > plan.max_j) plan.max_j = nj;
    }
    SFM_CHECK_ARG(capacity >= bound, "capacity below the sum over the pairs of N_i (of min(N_i, N_j) with cross_check)");
    return 0;
}

inline int md_scan_bytes(int64_t n_rows, hipStream_t s, size_t &bytes) {
    bytes = 0;
    SFM_HIP(rocprim::exclusive_scan(nullptr, bytes, (int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0,
                                    (size_t)n_rows + 1, rocprim::plus<int64_t>(), s));
    return 0;
}

// Behind the nearest-neighbour passes: the tests per keypoint, the scan of the
// flags (n_rows + 1 entries, the last a 0, so that the scan's last entry is
// the total) and the compacted matches.  nn_rev is null without cross_check.
inline int md_compact(hipStream_t s, int64_t P, int64_t max_i, int64_t n_rows, const int64_t *d_is,
                      const int32_t *d_pairs, const int64_t *d_ro, const int64_t *d_co, const int32_t *d_nn,
                      const int32_t *d_d1, const int32_t *d_d2, const int32_t *d_rev, double ratio_sq,
                      int32_t max_dsq, int32_t *d_flag, int64_t *d_place, char *d_tmp, size_t tmp_bytes,
                      int64_t *d_ms, int32_t *d_a, int32_t *d_b, int32_t *d_dsq) {
    const unsigned gy = (unsigned)(P < 65535 ? P : 65535);
    const dim3 g_rows((unsigned)(max_i > 0 ? ceil_div(max_i, MD_THREADS) : 1), gy);
    SFM_HIP(hipMemsetAsync(d_flag + n_rows, 0, sizeof(int32_t), s));
    if (max_i > 0)
        MD_LAUNCH(k_md_accept, g_rows, d_is, d_pairs, P, d_ro, d_co, d_nn, d_d1, d_d2, d_rev, ratio_sq, max_dsq,
                  d_flag);
    SFM_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_flag, d_place, (int64_t)0, (size_t)n_rows + 1,
                                    rocprim::plus<int64_t>(), s));
    MD_LAUNCH(k_md_write, g_rows, d_is, d_pairs, P, d_ro, d_nn, d_d1, d_flag, d_place, d_ms, d_a, d_b, d_dsq);
    return 0;
}

}  // namespace sfm
