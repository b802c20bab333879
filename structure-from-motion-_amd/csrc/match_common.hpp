// What descriptor matching (match_descriptors.hip) and guided matching
// (match_guided.hip) share, which is everything but the gate: the kernels that
// match_descriptors.hip describes and the host driver of a call (md_run).  The
// nearest-neighbour kernel and the driver take the gate as a policy type:
// MdNoGate here, the epipolar band in match_guided.hip.  retrieval.hip uses the
// ungated kernel for its vocabulary search.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "staging.hpp"

namespace sfm {

constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = 4;
constexpr int MD_MS = 2;                       // 16-row subtiles per wave
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

// No gate: every column of the other image is a candidate.  What a gate policy
// supplies (match_guided.hip has the other one): the 16-row subtiles a wave
// takes, the workgroups per CU it is built for, and how many terms it keeps per
// row and per column.  A gate has besides, and the kernel calls, row<SWAP>(F,
// xy, t) and col<SWAP>(F, xy, t) for the terms and in<SWAP>(row terms, column
// terms, thr2) for the decision.
struct MdNoGate {
    static constexpr bool gated = false;
    static constexpr int min_blocks = 1;
    static constexpr int ms(int) { return MD_MS; }
    static constexpr int row_terms(bool) { return 0; }
    static constexpr int col_terms(bool) { return 0; }
};

// rows of a workgroup
template <class Gate> constexpr int md_bm(int dim) { return MD_WAVES * Gate::ms(dim) * 16; }

// The nearest-neighbour pass that match_descriptors.hip describes (k_md_nn
// there): the matchers instantiate it for image pairs, and retrieval.hip for
// blocks of descriptors against a vocabulary's centres.  pairs is (first,
// second) per pair when !SWAP and read as (second, first) when SWAP; row_off[p]
// is where the pair's rows start in nn / d1 / d2.  A gate splits its decision
// on (row, column) into terms of the row alone, which the lane that holds the
// row's results computes once per pair and keeps in registers, and terms of the
// column alone, which the threads that fetch the tile's norms compute and which
// travel through LDS beside them; an element the gate refuses contributes
// MD_OUTSIDE in place of its w.  Rows and columns past the end carry NaN terms.
// xy, Fs, thr2 and n_cand are the epipolar gate's (MdGateIn on the device, thr2
// the squared half-width) and unread without a gate.  They are parameters of
// their own and not a struct of the policy's: only on a parameter does
// __restrict__ reach the compiler (not on a struct's members), and without it
// the gated kernels take 12 to 14 more VGPRs.
template <int DIM, bool SWAP, class Gate>
__global__ __launch_bounds__(MD_THREADS, Gate::min_blocks) void k_md_nn(
    const uint8_t *__restrict__ desc, const int32_t *__restrict__ norm, const int64_t *__restrict__ img_start,
    const int32_t *__restrict__ pairs, int64_t P, const int64_t *__restrict__ row_off, int32_t *__restrict__ nn,
    int32_t *__restrict__ d1, int32_t *__restrict__ d2, const double2 *__restrict__ xy,
    const double *__restrict__ Fs, double thr2, int32_t *__restrict__ n_cand) {
#pragma clang fp contract(off)
    constexpr bool GATED = Gate::gated;
    constexpr int MS = Gate::ms(DIM), BM = md_bm<Gate>(DIM);
    constexpr int KS = DIM / 64;                          // k steps
    constexpr int STRIDE = DIM + MD_PAD;                  // bytes of an LDS row
    constexpr int CH = DIM / 16;                          // 16-byte chunks per row
    constexpr int NQ = MD_TN * CH / MD_THREADS;           // chunks a thread stages per tile
    constexpr int NR = std::max(Gate::row_terms(SWAP), 1);  // gate terms of a row (there is no array of none)
    constexpr int NC = std::max(Gate::col_terms(SWAP), 1);  // ... and of a column
    static_assert(MD_TN * CH % MD_THREADS == 0, "a tile is a whole number of passes");
    __shared__ __attribute__((aligned(16))) uint8_t sB[2][MD_TN * STRIDE];
    __shared__ int32_t sNb[2][MD_TN];
    // the columns' terms, one array per term so that the 16 columns a wave reads are consecutive doubles;
    // without a gate nothing refers to it and it takes no LDS
    __shared__ double sT[2][NC][MD_TN];
    // a lane's gate state: the pair's F, the terms and the candidates of its result rows, the terms of the
    // column it staged and of the column it multiplies
    struct GateRegs {
        double F[9], rt[MS][4][NR], st_t[NC], ct[NC];
        int32_t cnt[MS][4];
    };
    struct NoRegs {};
    std::conditional_t<GATED, GateRegs, NoRegs> gr;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const double nan = __builtin_nan("");
    for (int64_t p = blockIdx.y; p < P; p += gridDim.y) {
        const int32_t ii = pairs[2 * p + (SWAP ? 1 : 0)], jj = pairs[2 * p + (SWAP ? 0 : 1)];
        const int64_t is = img_start[ii], js = img_start[jj];
        const int32_t ni = (int32_t)(img_start[ii + 1] - is), nj = (int32_t)(img_start[jj + 1] - js);
        const int32_t row0 = (int32_t)blockIdx.x * BM;
        if (row0 >= ni) continue;  // uniform over the workgroup
        const int32_t wrow0 = row0 + wave * (MS * 16);
        if constexpr (GATED) {
#pragma unroll
            for (int k = 0; k < 9; ++k) gr.F[k] = Fs[9 * p + k];
        }

        // this wave's rows, biased, in registers
        md_v4i a[MS][KS];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {
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
        int32_t m1[MS][4], i1[MS][4], m2[MS][4];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m1[ms][j] = MD_NONE;
                m2[ms][j] = MD_NONE;
                i1[ms][j] = -1;
                if constexpr (GATED) {
                    gr.cnt[ms][j] = 0;
                    const int32_t r = wrow0 + ms * 16 + lk * 4 + j;
                    double t[4] = {nan, nan, nan, nan};
                    if (r < ni) Gate::template row<SWAP>(gr.F, xy[is + r], t);
#pragma unroll
                    for (int k = 0; k < NR; ++k) gr.rt[ms][j][k] = t[k];
                }
            }

        const int32_t ntiles = (nj + MD_TN - 1) / MD_TN;
        md_v4i st[NQ];
        int32_t st_nb = MD_OUTSIDE;
        if constexpr (GATED) {
#pragma unroll
            for (int k = 0; k < NC; ++k) gr.st_t[k] = nan;
        }
        // tile t of the second image: global -> registers, registers -> LDS buffer
        auto fetch = [&](int32_t t) {
#pragma clang fp contract(off)
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
            if (tid < MD_TN) {
                if constexpr (GATED) {
                    double tt[4] = {nan, nan, nan, nan};
                    st_nb = MD_OUTSIDE;
                    if (c0 + tid < nj) {
                        st_nb = norm[js + c0 + tid];
                        Gate::template col<SWAP>(gr.F, xy[js + c0 + tid], tt);
                    }
#pragma unroll
                    for (int k = 0; k < NC; ++k) gr.st_t[k] = tt[k];
                } else {
                    st_nb = c0 + tid < nj ? norm[js + c0 + tid] : MD_OUTSIDE;
                }
            }
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = tid + q * MD_THREADS, col = c / CH, kc = c % CH;
                *reinterpret_cast<md_v4i *>(&sB[buf][col * STRIDE + kc * 16]) = st[q];
            }
            if (tid < MD_TN) {
                sNb[buf][tid] = st_nb;
                if constexpr (GATED) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) sT[buf][k][tid] = gr.st_t[k];
                }
            }
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
                if constexpr (GATED) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) gr.ct[k] = sT[cur][k][ns * 16 + lr];
                }
                const int32_t col = t * MD_TN + ns * 16 + lr;
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) {
                    md_v4i acc = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ms][ks], b[ks], acc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        int32_t w;
                        if constexpr (GATED) {  // the decision first: the order the registers were measured with
                            const bool in = Gate::template in<SWAP>(gr.rt[ms][j], gr.ct, thr2);
                            w = in ? nb - 2 * acc[j] : MD_OUTSIDE;
                            if (!SWAP) gr.cnt[ms][j] += in ? 1 : 0;
                        } else {
                            w = nb - 2 * acc[j];
                        }
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
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int32_t x1 = m1[ms][j], xi = i1[ms][j], x2 = m2[ms][j], xc = 0;
                if constexpr (GATED) xc = gr.cnt[ms][j];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const int32_t o1 = __shfl_xor(x1, o), oi = __shfl_xor(xi, o), o2 = __shfl_xor(x2, o);
                    md_merge(x1, xi, x2, o1, oi, o2);
                    if (GATED && !SWAP) xc += __shfl_xor(xc, o);
                }
                const int32_t r = wrow0 + ms * 16 + lk * 4 + j;
                if (lr == 0 && r < ni) {
                    const int32_t na = norm[is + r];
                    const bool has1 = x1 < MD_VALID, has2 = x2 < MD_VALID;
                    const int64_t o = row_off[p] + r;
                    nn[o] = has1 ? xi : -1;
                    if (d1) d1[o] = has1 ? na + x1 : MD_NONE;
                    if (d2) d2[o] = has2 ? na + x2 : MD_NONE;
                    if constexpr (GATED && !SWAP) {
                        if (n_cand) n_cand[o] = xc;
                    }
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

// f(std::integral_constant<int, dim>()) for a checked dim: kernels take it as a template argument
template <class F> int md_by_dim(int dim, F f) {
    if (dim == 64) return f(std::integral_constant<int, 64>());
    if (dim == 128) return f(std::integral_constant<int, 128>());
    return f(std::integral_constant<int, 256>());
}

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

// What sfm_match_descriptors_guided takes beyond sfm_match_descriptors (include/sfmcore.h); all unset without a gate
struct MdGateIn {
    const double *xy = nullptr, *F = nullptr;
    double gate = 0.0;
    int32_t *n_cand = nullptr;
};

// A call of either matcher, from the argument checks to the downloads.  The
// arguments are sfm_match_descriptors' and, checked after them, the gate's.
template <class Gate>
int md_run(const uint8_t *desc, int64_t n_kp, const int64_t *img_start, int32_t n_images, int32_t dim,
           const int32_t *pairs, int64_t P, double ratio, int32_t max_dsq, int32_t cross_check, int64_t capacity,
           int64_t *match_start, int32_t *match_a, int32_t *match_b, int32_t *match_dsq, int32_t *nn, int32_t *d1,
           int32_t *d2, int32_t *nn_rev, const MdGateIn &gi, int device) {
    constexpr bool GATED = Gate::gated;
    MdPlan plan;
    SFM_TRY(md_plan(desc, n_kp, img_start, n_images, dim, pairs, P, ratio, max_dsq, cross_check, capacity, match_start,
                    match_a, match_b, match_dsq, plan));
    if constexpr (GATED) {
        SFM_CHECK_ARG(n_kp == 0 || gi.xy, "null pointer");
        SFM_CHECK_ARG(P == 0 || gi.F, "null pointer");
        SFM_CHECK_ARG(std::isfinite(gi.gate) && gi.gate >= 0.0, "gate negative or not finite");
    }
    const int64_t *row_off = plan.row_off(), *col_off = plan.col_off();
    const int64_t max_i = plan.max_i, max_j = plan.max_j;
    const double ratio_sq = ratio * ratio;

    match_start[0] = 0;
    if (P == 0) return 0;
    const int64_t n_rows = row_off[P], n_cols = col_off[P];
    const bool reverse = cross_check || nn_rev;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    size_t tmp_bytes = 0;
    SFM_TRY(md_scan_bytes(n_rows, s, tmp_bytes));

    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_desc = in.add<uint8_t>(n_kp * dim);
    const auto i_xy = in.add<double2>(GATED ? n_kp : 0);
    const auto i_F = in.add<double>(GATED ? 9 * P : 0);
    const auto i_is = in.add<int64_t>(n_images + 1);
    const auto i_pairs = in.add<int32_t>(2 * P);
    const auto i_ro = in.add<int64_t>(P + 1), i_co = in.add<int64_t>(P + 1);
    const auto o_ms = out.add<int64_t>(P + 1);
    const auto o_a = out.add<int32_t>(n_rows), o_b = out.add<int32_t>(n_rows), o_dsq = out.add<int32_t>(n_rows);
    const auto o_nn = out.add<int32_t>(n_rows), o_d1 = out.add<int32_t>(n_rows), o_d2 = out.add<int32_t>(n_rows);
    const auto o_rev = out.add<int32_t>(reverse ? n_cols : 0);
    const auto o_cand = out.add<int32_t>(gi.n_cand ? n_rows : 0);
    const auto w_norm = work.add<int32_t>(n_kp);
    const auto w_flag = work.add<int32_t>(n_rows + 1);  // a last 0, so that the scan's last entry is the total
    const auto w_place = work.add<int64_t>(n_rows + 1);
    const auto w_tmp = work.add<char>(tmp_bytes);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_desc, desc, s));
    SFM_TRY(in.upload(i_xy, gi.xy, s));
    SFM_TRY(in.upload(i_F, gi.F, s));
    SFM_TRY(in.upload(i_is, img_start, s));
    SFM_TRY(in.upload(i_pairs, pairs, s));
    SFM_TRY(in.upload(i_ro, row_off, s));
    SFM_TRY(in.upload(i_co, col_off, s));
    SFM_TRY(tm.mark(s));

    const unsigned gy = (unsigned)(P < 65535 ? P : 65535);
    const uint8_t *d_desc = in.ptr(i_desc);
    const int64_t *d_is = in.ptr(i_is), *d_ro = in.ptr(i_ro), *d_co = in.ptr(i_co);
    const int32_t *d_pairs = in.ptr(i_pairs);
    int32_t *d_norm = work.ptr(w_norm);
    int32_t *d_nn = out.ptr(o_nn), *d_d1 = out.ptr(o_d1), *d_d2 = out.ptr(o_d2);
    int32_t *d_rev = reverse ? out.ptr(o_rev) : nullptr;
    const double2 *d_xy = in.ptr(i_xy);
    const double *d_F = in.ptr(i_F);
    const double thr2 = gi.gate * gi.gate;  // may be +inf: every den > 0 then passes
    int32_t *d_cand = gi.n_cand ? out.ptr(o_cand) : nullptr;
    if (n_kp > 0) {
        const dim3 g_norm((unsigned)ceil_div(n_kp * (dim / 16), MD_THREADS));
        SFM_TRY(md_by_dim(dim, [&](auto D) -> int {
            MD_LAUNCH(k_md_norms<D()>, g_norm, d_desc, n_kp, d_norm);
            return 0;
        }));
    }
    if (max_i > 0) {
        const dim3 g_fwd((unsigned)ceil_div(max_i, md_bm<Gate>(dim)), gy);
        SFM_TRY(md_by_dim(dim, [&](auto D) -> int {
            MD_LAUNCH((k_md_nn<D(), false, Gate>), g_fwd, d_desc, d_norm, d_is, d_pairs, P, d_ro, d_nn, d_d1, d_d2,
                      d_xy, d_F, thr2, d_cand);
            return 0;
        }));
    }
    if (reverse && max_j > 0) {
        const dim3 g_rev((unsigned)ceil_div(max_j, md_bm<Gate>(dim)), gy);
        SFM_TRY(md_by_dim(dim, [&](auto D) -> int {
            MD_LAUNCH((k_md_nn<D(), true, Gate>), g_rev, d_desc, d_norm, d_is, d_pairs, P, d_co, d_rev,
                      (int32_t *)nullptr, (int32_t *)nullptr, d_xy, d_F, thr2, (int32_t *)nullptr);
            return 0;
        }));
    }
    SFM_TRY(md_compact(s, P, max_i, n_rows, d_is, d_pairs, d_ro, d_co, d_nn, d_d1, d_d2,
                       cross_check ? (const int32_t *)d_rev : (const int32_t *)nullptr, ratio_sq, max_dsq,
                       work.ptr(w_flag), work.ptr(w_place), work.ptr(w_tmp), tmp_bytes, out.ptr(o_ms), out.ptr(o_a),
                       out.ptr(o_b), out.ptr(o_dsq)));
    SFM_TRY(tm.mark(s));

    // match_start first: its last entry sizes the other copies
    SFM_TRY(out.download(match_start, o_ms, s));
    SFM_HIP(hipStreamSynchronize(s));
    const size_t total = (size_t)match_start[P];
    SFM_TRY(out.download(match_a, o_a, 0, total, s));
    SFM_TRY(out.download(match_b, o_b, 0, total, s));
    SFM_TRY(out.download(match_dsq, o_dsq, 0, total, s));
    SFM_TRY(out.download(nn, o_nn, s));
    SFM_TRY(out.download(d1, o_d1, s));
    SFM_TRY(out.download(d2, o_d2, s));
    SFM_TRY(out.download(nn_rev, o_rev, s));
    SFM_TRY(out.download(gi.n_cand, o_cand, s));
    SFM_TRY(tm.finish(s));
    return 0;
}

}  // namespace sfm
