// Guided descriptor matching: sfm_match_descriptors with the candidates of a
// keypoint restricted to the keypoints of the other image inside a band
// around its epipolar line (include/sfmcore.h).  The pair's F comes from pair
// verification; the gate is vp_inlier of epi_sampson.hpp, bit for bit.
//
//   k_md_norms   as in match_descriptors.hip (match_common.hpp).
//   k_mg_nn      k_md_nn with a gate: the same workgroup of 4 waves over
//                MD_BM = 128 rows (64 at dim 256, one 16-row subtile per wave:
//                mg_ms), the A fragments in registers, the second
//                image through double-buffered LDS tiles of MD_TN = 64 columns,
//                the products on v_mfma_i32_16x16x64_i8 and the running top-2
//                per row.  vp_inlier splits into what depends on the first
//                image's keypoint alone, l = F (x, y, 1) and l0^2 + l1^2, and
//                what depends on the second's alone, (u, v) and m0^2 + m1^2
//                with m = F^T (u, v, 1).  A lane computes the terms of its
//                result rows (rows 4 (l >> 4) + 0..3 of each subtile) once per
//                pair in the prologue and keeps them in registers; the column
//                terms are computed by the 64 threads that fetch the tile's
//                norms and travel through LDS beside them (one array per term,
//                so that the 16 columns a wave reads are consecutive doubles).
//                Per element e = (u l0 + v l1) + l2, den = (l0^2 + l1^2) +
//                (m0^2 + m1^2) and den > 0 && e e < thr2 den are vp_inlier's
//                operations in its order, fp64 without contraction.  An
//                element outside the band contributes MD_OUTSIDE in place of
//                its w, so the top-2 update, the 16-lane merge and has1 / has2
//                are k_md_nn's; the forward pass counts the elements inside
//                per row (n_cand).  In the swapped pass (nn_rev) the rows are
//                the second image's keypoints and carry (u, v, m0^2 + m1^2),
//                the columns the first's and carry (l0, l1, l2, l0^2 + l1^2):
//                the same operands in the same roles, so a pair of keypoints is
//                a candidate in both passes or in neither.  A column past the
//                image's end carries NaN terms and fails the gate.
//   k_md_accept, rocPRIM scan, k_md_write   as in match_descriptors.hip.
//
// Integer minima, a scan and a gate without a reduction: every output is the
// same from run to run.
#include "match_common.hpp"

namespace sfm {

// 16-row subtiles per wave and rows of a workgroup: the gate terms of the rows
// take 8 VGPRs per row, and at dim 256 two subtiles do not fit beside the A
// fragments at two waves per SIMD.
constexpr int mg_ms(int dim) { return dim == 256 ? 1 : MD_MS; }
constexpr int mg_bm(int dim) { return MD_WAVES * mg_ms(dim) * 16; }

// What vp_inlier computes from the first image's keypoint alone: t = (l0, l1,
// l2, l0^2 + l1^2) with l = F (x, y, 1).
__device__ __forceinline__ void mg_first(const double (&F)[9], double x, double y, double (&t)[4]) {
#pragma clang fp contract(off)
    t[0] = (F[0] * x + F[1] * y) + F[2];
    t[1] = (F[3] * x + F[4] * y) + F[5];
    t[2] = (F[6] * x + F[7] * y) + F[8];
    t[3] = t[0] * t[0] + t[1] * t[1];
}

// ... and from the second's alone: t = (u, v, m0^2 + m1^2) with m = F^T (u, v, 1).
__device__ __forceinline__ void mg_second(const double (&F)[9], double u, double v, double (&t)[4]) {
#pragma clang fp contract(off)
    const double m0 = (F[0] * u + F[3] * v) + F[6];
    const double m1 = (F[1] * u + F[4] * v) + F[7];
    t[0] = u;
    t[1] = v;
    t[2] = m0 * m0 + m1 * m1;
    t[3] = 0.0;
}

// vp_inlier's decision from the two sides' terms
__device__ __forceinline__ bool mg_gate(const double *first, const double *second, double thr2) {
#pragma clang fp contract(off)
    const double e = (second[0] * first[0] + second[1] * first[1]) + first[2];
    const double den = first[3] + second[2];
    const double e2 = e * e;
    return den > 0.0 && e2 < thr2 * den;
}

// k_md_nn's arguments, and: xy the keypoints (desc's row order), F nine doubles
// per pair, thr2 the squared half-width, n_cand (forward pass only, nullable)
// the number of columns inside the band of each row.
template <int DIM, bool SWAP>
__global__ __launch_bounds__(MD_THREADS, 2) void k_mg_nn(const uint8_t *__restrict__ desc, const int32_t *__restrict__ norm,
                                                      const double2 *__restrict__ xy, const double *__restrict__ Fs,
                                                      double thr2, const int64_t *__restrict__ img_start,
                                                      const int32_t *__restrict__ pairs, int64_t P,
                                                      const int64_t *__restrict__ row_off, int32_t *__restrict__ nn,
                                                      int32_t *__restrict__ d1, int32_t *__restrict__ d2,
                                                      int32_t *__restrict__ n_cand) {
#pragma clang fp contract(off)
    constexpr int MS = mg_ms(DIM), BM = mg_bm(DIM);
    constexpr int KS = DIM / 64;                          // k steps
    constexpr int STRIDE = DIM + MD_PAD;                  // bytes of an LDS row
    constexpr int CH = DIM / 16;                          // 16-byte chunks per row
    constexpr int NQ = MD_TN * CH / MD_THREADS;           // chunks a thread stages per tile
    constexpr int NR = SWAP ? 3 : 4;                      // gate terms of a row
    constexpr int NC = SWAP ? 4 : 3;                      // ... and of a column
    static_assert(MD_TN * CH % MD_THREADS == 0, "a tile is a whole number of passes");
    __shared__ __attribute__((aligned(16))) uint8_t sB[2][MD_TN * STRIDE];
    __shared__ int32_t sNb[2][MD_TN];
    __shared__ double sT[2][NC][MD_TN];

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
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = Fs[9 * p + k];

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
        // the gate terms of the rows this lane holds results of
        double rt[MS][4][NR];
        int32_t m1[MS][4], i1[MS][4], m2[MS][4], cnt[MS][4];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m1[ms][j] = MD_NONE;
                m2[ms][j] = MD_NONE;
                i1[ms][j] = -1;
                cnt[ms][j] = 0;
                const int32_t r = wrow0 + ms * 16 + lk * 4 + j;
                double t[4] = {nan, nan, nan, nan};
                if (r < ni) {
                    const double2 q = xy[is + r];
                    if (SWAP) mg_second(F, q.x, q.y, t);
                    else mg_first(F, q.x, q.y, t);
                }
#pragma unroll
                for (int k = 0; k < NR; ++k) rt[ms][j][k] = t[k];
            }

        const int32_t ntiles = (nj + MD_TN - 1) / MD_TN;
        md_v4i st[NQ];
        int32_t st_nb = MD_OUTSIDE;
        double st_t[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) st_t[k] = nan;
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
                double tt[4] = {nan, nan, nan, nan};
                st_nb = MD_OUTSIDE;
                if (c0 + tid < nj) {
                    st_nb = norm[js + c0 + tid];
                    const double2 q = xy[js + c0 + tid];
                    if (SWAP) mg_first(F, q.x, q.y, tt);
                    else mg_second(F, q.x, q.y, tt);
                }
#pragma unroll
                for (int k = 0; k < NC; ++k) st_t[k] = tt[k];
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
#pragma unroll
                for (int k = 0; k < NC; ++k) sT[buf][k][tid] = st_t[k];
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
                double ct[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) ct[k] = sT[cur][k][ns * 16 + lr];
                const int32_t col = t * MD_TN + ns * 16 + lr;
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) {
                    md_v4i acc = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ms][ks], b[ks], acc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool in = SWAP ? mg_gate(ct, rt[ms][j], thr2) : mg_gate(rt[ms][j], ct, thr2);
                        const int32_t w = in ? nb - 2 * acc[j] : MD_OUTSIDE;
                        if (!SWAP) cnt[ms][j] += in ? 1 : 0;
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
                int32_t x1 = m1[ms][j], xi = i1[ms][j], x2 = m2[ms][j], xc = cnt[ms][j];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const int32_t o1 = __shfl_xor(x1, o), oi = __shfl_xor(xi, o), o2 = __shfl_xor(x2, o);
                    md_merge(x1, xi, x2, o1, oi, o2);
                    if (!SWAP) xc += __shfl_xor(xc, o);
                }
                const int32_t r = wrow0 + ms * 16 + lk * 4 + j;
                if (lr == 0 && r < ni) {
                    const int32_t na = norm[is + r];
                    const bool has1 = x1 < MD_VALID, has2 = x2 < MD_VALID;
                    const int64_t o = row_off[p] + r;
                    nn[o] = has1 ? xi : -1;
                    if (d1) d1[o] = has1 ? na + x1 : MD_NONE;
                    if (d2) d2[o] = has2 ? na + x2 : MD_NONE;
                    if (!SWAP && n_cand) n_cand[o] = xc;
                }
            }
    }
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_match_descriptors_guided(const uint8_t *desc, const double *xy, int64_t n_kp,
                                            const int64_t *img_start, int32_t n_images, int32_t dim,
                                            const int32_t *pairs, const double *F, int64_t P, double gate, double ratio,
                                            int32_t max_dsq, int32_t cross_check, int64_t capacity,
                                            int64_t *match_start, int32_t *match_a, int32_t *match_b,
                                            int32_t *match_dsq, int32_t *nn, int32_t *d1, int32_t *d2, int32_t *nn_rev,
                                            int32_t *n_cand, int device) {
    MdPlan plan;
    SFM_TRY(md_plan(desc, n_kp, img_start, n_images, dim, pairs, P, ratio, max_dsq, cross_check, capacity, match_start,
                    match_a, match_b, match_dsq, plan));
    SFM_CHECK_ARG(n_kp == 0 || xy, "null pointer");
    SFM_CHECK_ARG(P == 0 || F, "null pointer");
    SFM_CHECK_ARG(std::isfinite(gate) && gate >= 0.0, "gate negative or not finite");
    const int64_t *row_off = plan.row_off(), *col_off = plan.col_off();
    const int64_t max_i = plan.max_i, max_j = plan.max_j;
    const double ratio_sq = ratio * ratio, thr2 = gate * gate;  // thr2 may be +inf: every den > 0 then passes

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
    const auto i_xy = in.add<double2>(n_kp);
    const auto i_F = in.add<double>(9 * P);
    const auto i_is = in.add<int64_t>(n_images + 1);
    const auto i_pairs = in.add<int32_t>(2 * P);
    const auto i_ro = in.add<int64_t>(P + 1), i_co = in.add<int64_t>(P + 1);
    const auto o_ms = out.add<int64_t>(P + 1);
    const auto o_a = out.add<int32_t>(n_rows), o_b = out.add<int32_t>(n_rows), o_dsq = out.add<int32_t>(n_rows);
    const auto o_nn = out.add<int32_t>(n_rows), o_d1 = out.add<int32_t>(n_rows), o_d2 = out.add<int32_t>(n_rows);
    const auto o_rev = out.add<int32_t>(reverse ? n_cols : 0);
    const auto o_cand = out.add<int32_t>(n_cand ? n_rows : 0);
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
    SFM_TRY(in.upload(i_xy, xy, s));
    SFM_TRY(in.upload(i_F, F, s));
    SFM_TRY(in.upload(i_is, img_start, s));
    SFM_TRY(in.upload(i_pairs, pairs, s));
    SFM_TRY(in.upload(i_ro, row_off, s));
    SFM_TRY(in.upload(i_co, col_off, s));
    SFM_TRY(tm.mark(s));

    const unsigned gy = (unsigned)(P < 65535 ? P : 65535);
    const uint8_t *d_desc = in.ptr(i_desc);
    const double2 *d_xy = in.ptr(i_xy);
    const double *d_F = in.ptr(i_F);
    const int64_t *d_is = in.ptr(i_is), *d_ro = in.ptr(i_ro), *d_co = in.ptr(i_co);
    const int32_t *d_pairs = in.ptr(i_pairs);
    int32_t *d_norm = work.ptr(w_norm);
    int32_t *d_nn = out.ptr(o_nn), *d_d1 = out.ptr(o_d1), *d_d2 = out.ptr(o_d2);
    int32_t *d_rev = reverse ? out.ptr(o_rev) : nullptr;
    int32_t *d_cand = n_cand ? out.ptr(o_cand) : nullptr;
    if (n_kp > 0) {
        const dim3 g_norm((unsigned)ceil_div(n_kp * (dim / 16), MD_THREADS));
#define MG_NORMS(D) MD_LAUNCH(k_md_norms<D>, g_norm, d_desc, n_kp, d_norm)
        MD_BY_DIM(MG_NORMS);
#undef MG_NORMS
    }
    if (max_i > 0) {
        const dim3 g_fwd((unsigned)ceil_div(max_i, mg_bm(dim)), gy);
#define MG_FWD(D)                                                                                                   \
    MD_LAUNCH((k_mg_nn<D, false>), g_fwd, d_desc, d_norm, d_xy, d_F, thr2, d_is, d_pairs, P, d_ro, d_nn, d_d1, d_d2, \
              d_cand)
        MD_BY_DIM(MG_FWD);
#undef MG_FWD
    }
    if (reverse && max_j > 0) {
        const dim3 g_rev((unsigned)ceil_div(max_j, mg_bm(dim)), gy);
#define MG_REV(D)                                                                                             \
    MD_LAUNCH((k_mg_nn<D, true>), g_rev, d_desc, d_norm, d_xy, d_F, thr2, d_is, d_pairs, P, d_co, d_rev,       \
              (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr)
        MD_BY_DIM(MG_REV);
#undef MG_REV
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
    SFM_TRY(out.download(n_cand, o_cand, s));
    SFM_TRY(tm.finish(s));
    return 0;
}
