// Pair selection by image retrieval: a visual vocabulary (k-means on uint8
// descriptors with uint8 centres, sfm_vocab_train) and tf-idf retrieval over
// the quantised words with the top-k neighbours per image (sfm_select_pairs).
// The stage that chooses the pairs sfm_match_descriptors is given; matching
// itself stays exhaustive per pair.  The reference has no such stage.
// Everything is integer work except the score (include/sfmcore.h).
//
// sfm_vocab_train
//   k_md_norms, k_md_nn   the matcher's kernels (match_common.hpp), no gate:
//                the centres are appended to the descriptors as one more
//                "image", the descriptor rows are cut into pseudo-images of at
//                most MD_MAX_KP rows, and every pseudo-image is paired with the
//                centres.  nn is the word, d1 the squared distance.
//   k_vt_tally   members per centre (64-bit atomics) and the int64 inertia
//                (a wave's sum by shuffles, one atomic per wave).
//   rocPRIM      a radix sort of the words with the row number as the value
//                (cam_major_sort of csr_sort.hip): the members of a centre
//                become adjacent.
//   k_vt_sums    DIM / 4 lanes walk VT_ROWS adjacent sorted rows, four bytes of
//                a row each, and keep the byte sums of the current word in
//                registers; they go to the global uint32 sums with atomics
//                only where the word changes and at the end of the walk:
//                (n / VT_ROWS + n_words) dim atomics and not n dim.
//   k_vt_update  one thread per centre byte: the mean rounded half up, and a
//                flag when a byte changed, which the host reads once per
//                iteration.
//
// sfm_select_pairs
//   k_sp_keys    key = image << word_bits | word per keypoint.
//   rocPRIM      a radix sort of the keys; k_sp_heads marks the first of every
//                run of equal keys and an exclusive scan numbers the runs: an
//                entry is one (image, word) with h = the run's length.
//   k_sp_entries the entries' first positions and keys; df by atomics.
//   rocPRIM      an exclusive scan of df: the postings' CSR by word.
//   k_sp_post    v = h q[df] per entry, and the entry's place in its word's
//                posting list by an atomic cursor (the order inside a list
//                varies from run to run; the integer sums do not).
//   k_sp_norm2   one workgroup per image: norm2 and its fp64 root.
//   k_sp_query   one workgroup per query image with an int64 accumulator per
//                database image in LDS (8 n_images bytes, 128 KB at the
//                16,384 images the entry allows): 16 lanes per entry of the
//                query walk the word's posting list and add v_i v_j with LDS
//                atomics.  Then top_k rounds of a workgroup arg-max by (score
//                descending, j ascending) over the j with dot > 0; a chosen j
//                has its accumulator zeroed.
//
// Integer atomics are order-independent: every output is the same from run to
// run.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "match_common.hpp"

namespace sfm {

int cam_major_sort(void *temp, size_t &temp_bytes, const int32_t *cam, uint32_t *keys_out, int32_t *perm_out,
                   int64_t no, int32_t nc, hipStream_t s);  // csr_sort.hip

constexpr int VT_ROWS = 64;                         // sorted rows one lane group walks
constexpr int64_t VT_MAX_TRAIN = (int64_t)1 << 24;  // 255 * 2^24 < 2^32: the uint32 sums
constexpr int32_t VT_MAX_WORDS = 1 << 20;
constexpr int32_t SP_MAX_IMAGES = 16384;
constexpr int64_t SP_MAX_KP = (int64_t)1 << 18;
constexpr int SP_THREADS = 512;
constexpr int SP_LANES = 16;  // lanes per entry of the query

typedef unsigned long long u64;

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// count[w] += members, *inertia += dsq over the rows
static __global__ __launch_bounds__(MD_THREADS) void k_vt_tally(const int32_t *__restrict__ word,
                                                               const int32_t *__restrict__ dsq, int64_t n, u64 *count,
                                                               u64 *inertia) {
    int64_t sum = 0;
    for (int64_t a = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x; a < n; a += (int64_t)gridDim.x * MD_THREADS) {
        atomicAdd(&count[word[a]], (u64)1);
        sum += dsq[a];
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(inertia, (u64)sum);
}

// sums[w][k] += byte k of every member of w; key / perm are the sorted words and their rows
template <int DIM>
__global__ __launch_bounds__(MD_THREADS) void k_vt_sums(const uint8_t *__restrict__ desc,
                                                        const uint32_t *__restrict__ key,
                                                        const int32_t *__restrict__ perm, int64_t n, uint32_t *sums) {
    constexpr int G = DIM / 4;  // lanes of a group
    const int l = threadIdx.x % G;
    const int64_t base = ((int64_t)blockIdx.x * (MD_THREADS / G) + threadIdx.x / G) * VT_ROWS;
    const int64_t end = base + VT_ROWS < n ? base + VT_ROWS : n;
    uint32_t cur = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    bool any = false;
    auto flush = [&]() {
        uint32_t *dst = sums + (int64_t)cur * DIM + 4 * l;
        atomicAdd(dst + 0, s0);
        atomicAdd(dst + 1, s1);
        atomicAdd(dst + 2, s2);
        atomicAdd(dst + 3, s3);
        s0 = s1 = s2 = s3 = 0;
    };
    for (int64_t r = base; r < end; r += 4) {
        uint32_t w[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            w[u] = v[u] = 0;
            if (r + u < end) {
                w[u] = key[r + u];
                v[u] = *reinterpret_cast<const uint32_t *>(desc + (int64_t)perm[r + u] * DIM + 4 * l);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r + u >= end) break;
            if (any && w[u] != cur) flush();
            cur = w[u];
            any = true;
            s0 += v[u] & 255u;
            s1 += (v[u] >> 8) & 255u;
            s2 += (v[u] >> 16) & 255u;
            s3 += v[u] >> 24;
        }
    }
    if (any) flush();
}

// centres[w][k] = floor((2 sum + cnt) / (2 cnt)) where cnt > 0; *changed = 1 when a byte differs
static __global__ __launch_bounds__(MD_THREADS) void k_vt_update(uint8_t *centres, const uint32_t *__restrict__ sums,
                                                                const u64 *__restrict__ count, int64_t n_bytes,
                                                                int32_t dim, int32_t *changed) {
    const int64_t g = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (g >= n_bytes) return;
    const u64 c = count[g / dim];
    if (c == 0) return;
    const uint8_t v = (uint8_t)((2 * (u64)sums[g] + c) / (2 * c));
    if (v != centres[g]) {
        centres[g] = v;
        *changed = 1;
    }
}

// key[a] = image of keypoint a << word_bits | word[a]
static __global__ __launch_bounds__(MD_THREADS) void k_sp_keys(const int32_t *__restrict__ word,
                                                              const int64_t *__restrict__ img_start, int32_t n_images,
                                                              int64_t n_kp, int word_bits, u64 *key) {
    const int64_t a = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (a >= n_kp) return;
    int32_t lo = 0, hi = n_images;  // the last image with img_start <= a: images may be empty
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (img_start[mid] <= a) lo = mid; else hi = mid;
    }
    key[a] = ((u64)lo << word_bits) | (u64)word[a];
}

// flag[a] = 1 at the first of every run of equal keys; flag[n_kp] = 0
static __global__ __launch_bounds__(MD_THREADS) void k_sp_heads(const u64 *__restrict__ key, int64_t n_kp,
                                                               int32_t *flag) {
    const int64_t a = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (a > n_kp) return;
    flag[a] = a < n_kp && (a == 0 || key[a] != key[a - 1]) ? 1 : 0;
}

// entry e = place[a] of a run's first keypoint a: its position and key; df of its word.  ent_pos[E] = n_kp.
static __global__ __launch_bounds__(MD_THREADS) void k_sp_entries(const u64 *__restrict__ key,
                                                                 const int32_t *__restrict__ flag,
                                                                 const int64_t *__restrict__ place, int64_t n_kp,
                                                                 int word_bits, int64_t *ent_pos, u64 *ent_key,
                                                                 int32_t *df) {
    const int64_t a = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (a > n_kp) return;
    if (a == n_kp) {
        ent_pos[place[a]] = n_kp;
        return;
    }
    if (!flag[a]) return;
    const int64_t e = place[a];
    ent_pos[e] = a;
    ent_key[e] = key[a];
    atomicAdd(&df[key[a] & (((u64)1 << word_bits) - 1)], 1);
}

// v of every entry, and the entry in its word's posting list
static __global__ __launch_bounds__(MD_THREADS) void k_sp_post(const int64_t *__restrict__ place, int64_t n_kp,
                                                              const int64_t *__restrict__ ent_pos,
                                                              const u64 *__restrict__ ent_key, int word_bits,
                                                              const int32_t *__restrict__ df,
                                                              const int32_t *__restrict__ q,
                                                              const int64_t *__restrict__ wstart, int32_t *cursor,
                                                              int32_t *ent_v, int32_t *post_img, int32_t *post_v) {
    const int64_t e = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (e >= place[n_kp]) return;
    const u64 k = ent_key[e];
    const int32_t w = (int32_t)(k & (((u64)1 << word_bits) - 1));
    const int32_t v = (int32_t)(ent_pos[e + 1] - ent_pos[e]) * q[df[w]];  // h <= 2^18, q < 2^12
    ent_v[e] = v;
    const int64_t slot = wstart[w] + atomicAdd(&cursor[w], 1);
    post_img[slot] = (int32_t)(k >> word_bits);
    post_v[slot] = v;
}

// norm2[i] = sum of v^2 over the entries of image i, root[i] = sqrt((double)norm2[i])
static __global__ __launch_bounds__(MD_THREADS) void k_sp_norm2(const int64_t *__restrict__ img_start,
                                                               const int64_t *__restrict__ place,
                                                               const int32_t *__restrict__ ent_v, int64_t *norm2,
                                                               double *root) {
    __shared__ int64_t part[MD_THREADS / 64];
    const int i = blockIdx.x;
    const int64_t e0 = place[img_start[i]], e1 = place[img_start[i + 1]];
    int64_t sum = 0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += MD_THREADS) sum += (int64_t)ent_v[e] * ent_v[e];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int k = 0; k < MD_THREADS / 64; ++k) t += part[k];
        norm2[i] = t;
        root[i] = sqrt((double)t);
    }
}

// (score, j) order: score descending, then j ascending; j < 0 is "none"
__device__ __forceinline__ void sp_better(double &s, int32_t &j, double os, int32_t oj) {
    if (oj >= 0 && (j < 0 || os > s || (os == s && oj < j))) {
        s = os;
        j = oj;
    }
}

// Row i of neighbour / score / dot.  Dynamic LDS: n_images int64 accumulators, then per wave a double and an int.
static __global__ __launch_bounds__(SP_THREADS) void k_sp_query(const int64_t *__restrict__ img_start,
                                                               const int64_t *__restrict__ place,
                                                               const u64 *__restrict__ ent_key,
                                                               const int32_t *__restrict__ ent_v, int word_bits,
                                                               const int64_t *__restrict__ wstart,
                                                               const int32_t *__restrict__ post_img,
                                                               const int32_t *__restrict__ post_v,
                                                               const double *__restrict__ root, int32_t n_images,
                                                               int32_t top_k, int32_t *neighbour, double *score,
                                                               int64_t *dot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sp_lds[];
    constexpr int NW = SP_THREADS / 64;
    u64 *acc = reinterpret_cast<u64 *>(sp_lds);
    double *ws = reinterpret_cast<double *>(acc + n_images);
    int32_t *wj = reinterpret_cast<int32_t *>(ws + NW);
    const int i = blockIdx.x, t = threadIdx.x;
    for (int32_t j = t; j < n_images; j += SP_THREADS) acc[j] = 0;
    __syncthreads();

    const int64_t e0 = place[img_start[i]], e1 = place[img_start[i + 1]];
    const u64 mask = ((u64)1 << word_bits) - 1;
    for (int64_t e = e0 + t / SP_LANES; e < e1; e += SP_THREADS / SP_LANES) {
        const int64_t vi = ent_v[e];
        if (vi == 0) continue;  // a word in every image
        const int32_t w = (int32_t)(ent_key[e] & mask);
        const int64_t p1 = wstart[w + 1];
        for (int64_t p = wstart[w] + t % SP_LANES; p < p1; p += SP_LANES)
            atomicAdd(&acc[post_img[p]], (u64)(vi * (int64_t)post_v[p]));
    }
    __syncthreads();
    if (t == 0) acc[i] = 0;  // an image is no neighbour of itself
    __syncthreads();

    const double ri = root[i];
    int32_t *nb = neighbour + (int64_t)i * top_k;
    double *sc = score + (int64_t)i * top_k;
    int64_t *dt = dot ? dot + (int64_t)i * top_k : nullptr;
    int32_t k = 0;
    for (; k < top_k; ++k) {
        double bs = 0.0;
        int32_t bj = -1;
        for (int32_t j = t; j < n_images; j += SP_THREADS) {  // ascending j per thread
            const int64_t d = (int64_t)acc[j];
            if (d > 0) sp_better(bs, bj, (double)d / (ri * root[j]), j);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o);
            const int32_t oj = __shfl_xor(bj, o);
            sp_better(bs, bj, os, oj);
        }
        if ((t & 63) == 0) {
            ws[t >> 6] = bs;
            wj[t >> 6] = bj;
        }
        __syncthreads();
        bs = ws[0];
        bj = wj[0];
#pragma unroll
        for (int u = 1; u < NW; ++u) sp_better(bs, bj, ws[u], wj[u]);
        if (bj < 0) break;  // uniform: every thread read the same LDS
        if (t == 0) {
            nb[k] = bj;
            sc[k] = bs;
            if (dt) dt[k] = (int64_t)acc[bj];
        }
        __syncthreads();  // the round's reads of acc, ws and wj are over
        if (t == 0) acc[bj] = 0;
        __syncthreads();
    }
    for (int32_t r = k + t; r < top_k; r += SP_THREADS) {
        nb[r] = -1;
        sc[r] = 0.0;
        if (dt) dt[r] = 0;
    }
}

static int bit_length(int64_t n) {  // bits that hold 0 .. n - 1, at least 1
    int b = 1;
    while (b < 62 && ((int64_t)1 << b) < n) ++b;
    return b;
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_vocab_train(const uint8_t *desc, int64_t n, int32_t dim, int32_t n_words, int32_t max_iterations,
                               uint8_t *centres, int32_t *word, int64_t *count, int64_t *inertia, int32_t *iterations,
                               int device) {
    SFM_CHECK_ARG(desc && centres && iterations, "null pointer");
    SFM_CHECK_ARG(dim == 64 || dim == 128 || dim == 256, "dim is not 64, 128 or 256");
    SFM_CHECK_ARG(n >= 1, "n < 1");
    SFM_CHECK_ARG(n_words >= 1 && n_words <= n && n_words <= VT_MAX_WORDS, "n_words outside [1, min(n, 2^20)]");
    SFM_CHECK_ARG(max_iterations >= 0, "max_iterations < 0");
    SFM_CHECK_ARG(max_iterations == 0 || n <= VT_MAX_TRAIN, "more than 2^24 descriptors with max_iterations > 0");

    // the rows as pseudo-images of at most MD_MAX_KP rows, each paired with the centres (the last "image")
    const int64_t P = (n + MD_MAX_KP - 1) / MD_MAX_KP;
    std::vector<int64_t> is(P + 2);
    std::vector<int32_t> pairs(2 * P);
    for (int64_t p = 0; p < P; ++p) {
        is[p] = p * MD_MAX_KP;
        pairs[2 * p] = (int32_t)p;
        pairs[2 * p + 1] = (int32_t)P;
    }
    is[P] = n;
    is[P + 1] = n + n_words;
    const int64_t max_i = n < MD_MAX_KP ? n : MD_MAX_KP;
    const int64_t n_bytes = (int64_t)n_words * dim;
    const bool train = max_iterations > 0;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    size_t tmp_bytes = 0;
    if (train) SFM_TRY(cam_major_sort(nullptr, tmp_bytes, nullptr, nullptr, nullptr, n, n_words, s));

    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_desc = in.add<uint8_t>((n + n_words) * dim);  // the centres behind the descriptors
    const auto i_is = in.add<int64_t>(P + 2);                  // ... which is also row_off
    const auto i_pairs = in.add<int32_t>(2 * P);
    const auto o_word = out.add<int32_t>(n);
    const auto o_count = out.add<u64>(n_words);
    const auto o_inertia = out.add<u64>(max_iterations + 1);
    const auto w_norm = work.add<int32_t>(n + n_words);
    const auto w_dsq = work.add<int32_t>(n);
    const auto w_changed = work.add<int32_t>(max_iterations + 1);
    const auto w_sums = work.add<uint32_t>(train ? n_bytes : 0);
    const auto w_key = work.add<uint32_t>(train ? n : 0);
    const auto w_perm = work.add<int32_t>(train ? n : 0);
    const auto w_tmp = work.add<char>(tmp_bytes);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_desc, desc, 0, (size_t)(n * dim), s));
    SFM_TRY(in.upload(i_desc, centres, (size_t)(n * dim), (size_t)n_bytes, s));
    SFM_TRY(in.upload(i_is, is.data(), s));
    SFM_TRY(in.upload(i_pairs, pairs.data(), s));
    SFM_TRY(tm.mark(s));

    uint8_t *d_desc = in.ptr(i_desc), *d_centres = in.ptr(i_desc, (size_t)(n * dim));
    const int64_t *d_is = in.ptr(i_is);
    const int32_t *d_pairs = in.ptr(i_pairs);
    int32_t *d_norm = work.ptr(w_norm), *d_word = out.ptr(o_word), *d_dsq = work.ptr(w_dsq);
    int32_t *d_changed = work.ptr(w_changed);
    u64 *d_count = out.ptr(o_count), *d_inertia = out.ptr(o_inertia);
    const dim3 g_nn((unsigned)ceil_div(max_i, md_bm<MdNoGate>(dim)), (unsigned)(P < 65535 ? P : 65535));
    const dim3 g_tally((unsigned)(ceil_div(n, MD_THREADS) < 4096 ? ceil_div(n, MD_THREADS) : 4096));
    const dim3 g_update((unsigned)ceil_div(n_bytes, MD_THREADS));
    SFM_HIP(hipMemsetAsync(d_inertia, 0, o_inertia.bytes(), s));
    SFM_HIP(hipMemsetAsync(d_changed, 0, w_changed.bytes(), s));

    // norms from row `first` on, the assignment to the present centres and its tally into inertia[t]
    auto assign = [&](int64_t first, int32_t t) -> int {
        const int64_t rows = n + n_words - first;
        const dim3 g_norm((unsigned)ceil_div(rows * (dim / 16), MD_THREADS));
        const uint8_t *nd = d_desc + first * dim;
        int32_t *nn = d_norm + first;
        SFM_TRY(md_by_dim(dim, [&](auto D) -> int {
            MD_LAUNCH(k_md_norms<D()>, g_norm, nd, rows, nn);
            MD_LAUNCH((k_md_nn<D(), false, MdNoGate>), g_nn, (const uint8_t *)d_desc, (const int32_t *)d_norm, d_is,
                      d_pairs, P, d_is, d_word, d_dsq, (int32_t *)nullptr, (const double2 *)nullptr,
                      (const double *)nullptr, 0.0, (int32_t *)nullptr);
            return 0;
        }));
        SFM_HIP(hipMemsetAsync(d_count, 0, o_count.bytes(), s));
        MD_LAUNCH(k_vt_tally, g_tally, (const int32_t *)d_word, (const int32_t *)d_dsq, n, d_count, d_inertia + t);
        return 0;
    };

    SFM_TRY(assign(0, 0));
    int32_t T = 0;
    while (T < max_iterations) {
        uint32_t *d_sums = work.ptr(w_sums), *d_key = work.ptr(w_key);
        int32_t *d_perm = work.ptr(w_perm);
        SFM_HIP(hipMemsetAsync(d_sums, 0, w_sums.bytes(), s));
        SFM_TRY(cam_major_sort(work.ptr(w_tmp), tmp_bytes, d_word, d_key, d_perm, n, n_words, s));
        const int per_block = MD_THREADS / (dim / 4) * VT_ROWS;
        const dim3 g_sums((unsigned)ceil_div(n, per_block));
        SFM_TRY(md_by_dim(dim, [&](auto D) -> int {
            MD_LAUNCH(k_vt_sums<D()>, g_sums, (const uint8_t *)d_desc, (const uint32_t *)d_key,
                      (const int32_t *)d_perm, n, d_sums);
            return 0;
        }));
        MD_LAUNCH(k_vt_update, g_update, d_centres, (const uint32_t *)d_sums, (const u64 *)d_count, n_bytes, dim,
                  d_changed + T);
        int32_t changed = 0;
        SFM_HIP(hipMemcpyAsync(&changed, d_changed + T, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        SFM_HIP(hipStreamSynchronize(s));
        ++T;
        if (!changed) {  // the same centres: the same words, counts and inertia
            SFM_HIP(hipMemcpyAsync(d_inertia + T, d_inertia + T - 1, sizeof(u64), hipMemcpyDeviceToDevice, s));
            break;
        }
        SFM_TRY(assign(n, T));
    }
    SFM_TRY(tm.mark(s));

    SFM_TRY(in.download(centres, i_desc, (size_t)(n * dim), (size_t)n_bytes, s));
    SFM_TRY(out.download(word, o_word, s));
    SFM_TRY(out.download(count, o_count, s));
    SFM_TRY(out.download(inertia, o_inertia, 0, (size_t)T + 1, s));
    SFM_TRY(tm.finish(s));
    *iterations = T;
    return 0;
}

extern "C" int sfm_select_pairs(const int32_t *word, int64_t n_kp, const int64_t *img_start, int32_t n_images,
                                int32_t n_words, int32_t top_k, int32_t *neighbour, double *score, int64_t *dot,
                                int64_t *norm2, int32_t *df, int device) {
    SFM_CHECK_ARG(n_kp >= 0 && n_images >= 0, "n_kp or n_images < 0");
    SFM_CHECK_ARG(n_images <= SP_MAX_IMAGES, "more than 16,384 images");
    SFM_CHECK_ARG(n_words >= 1 && n_words <= VT_MAX_WORDS, "n_words outside [1, 2^20]");
    SFM_CHECK_ARG(top_k >= 0, "top_k < 0");
    SFM_CHECK_ARG(img_start, "null pointer");
    SFM_CHECK_ARG(n_kp == 0 || word, "null pointer");
    SFM_CHECK_ARG(n_images == 0 || top_k == 0 || (neighbour && score), "null pointer");
    SFM_TRY(check_csr(img_start, n_images, n_kp, "img_start", "keypoint", SP_MAX_KP,
                      "an image with more than 2^18 keypoints"));
    SFM_TRY(check_index(word, n_kp, n_words, "a word outside [0, n_words)"));
    if (n_images == 0 || top_k == 0) return 0;

    const int64_t n_out = (int64_t)n_images * top_k;
    if (n_kp == 0) {  // no keypoint at all: every row is padding
        for (int64_t k = 0; k < n_out; ++k) {
            neighbour[k] = -1;
            score[k] = 0.0;
            if (dot) dot[k] = 0;
        }
        for (int32_t i = 0; norm2 && i < n_images; ++i) norm2[i] = 0;
        for (int32_t w = 0; df && w < n_words; ++w) df[w] = 0;
        return 0;
    }
    // q[d] = floor(256 log(n_images / d) + 0.5), d = 1 .. n_images; q[0] is never read
    std::vector<int32_t> q((size_t)n_images + 1, 0);
    for (int32_t d = 1; d <= n_images; ++d)
        q[d] = (int32_t)std::floor(256.0 * std::log((double)n_images / (double)d) + 0.5);
    const int word_bits = bit_length(n_words), key_bits = word_bits + bit_length(n_images);

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    size_t sort_bytes = 0, scan_kp = 0, scan_w = 0;
    SFM_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, (const u64 *)nullptr, (u64 *)nullptr, (size_t)n_kp, 0,
                                     key_bits, s));
    SFM_TRY(md_scan_bytes(n_kp, s, scan_kp));
    SFM_TRY(md_scan_bytes(n_words, s, scan_w));
    const size_t tmp_bytes = std::max(sort_bytes, std::max(scan_kp, scan_w));

    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_word = in.add<int32_t>(n_kp);
    const auto i_is = in.add<int64_t>(n_images + 1);
    const auto i_q = in.add<int32_t>(n_images + 1);
    const auto o_nb = out.add<int32_t>(n_out);
    const auto o_score = out.add<double>(n_out);
    const auto o_dot = out.add<int64_t>(n_out);
    const auto o_norm2 = out.add<int64_t>(n_images);
    const auto o_df = out.add<int32_t>(n_words + 1);  // a last 0, so that the scan's last entry is the total
    const auto w_key = work.add<u64>(n_kp), w_skey = work.add<u64>(n_kp);
    const auto w_flag = work.add<int32_t>(n_kp + 1);
    const auto w_place = work.add<int64_t>(n_kp + 1);
    const auto w_epos = work.add<int64_t>(n_kp + 1);
    const auto w_ekey = work.add<u64>(n_kp);
    const auto w_ev = work.add<int32_t>(n_kp);
    const auto w_wstart = work.add<int64_t>(n_words + 1);
    const auto w_cursor = work.add<int32_t>(n_words);
    const auto w_pimg = work.add<int32_t>(n_kp), w_pv = work.add<int32_t>(n_kp);
    const auto w_root = work.add<double>(n_images);
    const auto w_tmp = work.add<char>(tmp_bytes);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_word, word, s));
    SFM_TRY(in.upload(i_is, img_start, s));
    SFM_TRY(in.upload(i_q, q.data(), s));
    SFM_TRY(tm.mark(s));

    const int32_t *d_word = in.ptr(i_word), *d_q = in.ptr(i_q);
    const int64_t *d_is = in.ptr(i_is);
    u64 *d_key = work.ptr(w_key), *d_skey = work.ptr(w_skey), *d_ekey = work.ptr(w_ekey);
    int32_t *d_flag = work.ptr(w_flag), *d_ev = work.ptr(w_ev), *d_cursor = work.ptr(w_cursor);
    int32_t *d_pimg = work.ptr(w_pimg), *d_pv = work.ptr(w_pv), *d_df = out.ptr(o_df);
    int64_t *d_place = work.ptr(w_place), *d_epos = work.ptr(w_epos), *d_wstart = work.ptr(w_wstart);
    double *d_root = work.ptr(w_root);
    char *d_tmp = work.ptr(w_tmp);
    const dim3 g_kp((unsigned)ceil_div(n_kp, MD_THREADS)), g_kp1((unsigned)ceil_div(n_kp + 1, MD_THREADS));
    SFM_HIP(hipMemsetAsync(d_df, 0, o_df.bytes(), s));
    SFM_HIP(hipMemsetAsync(d_cursor, 0, w_cursor.bytes(), s));
    MD_LAUNCH(k_sp_keys, g_kp, d_word, d_is, n_images, n_kp, word_bits, d_key);
    size_t tb = tmp_bytes;
    SFM_HIP(rocprim::radix_sort_keys(d_tmp, tb, (const u64 *)d_key, d_skey, (size_t)n_kp, 0, key_bits, s));
    MD_LAUNCH(k_sp_heads, g_kp1, (const u64 *)d_skey, n_kp, d_flag);
    tb = tmp_bytes;
    SFM_HIP(rocprim::exclusive_scan(d_tmp, tb, d_flag, d_place, (int64_t)0, (size_t)n_kp + 1,
                                    rocprim::plus<int64_t>(), s));
    MD_LAUNCH(k_sp_entries, g_kp1, (const u64 *)d_skey, (const int32_t *)d_flag, (const int64_t *)d_place, n_kp,
              word_bits, d_epos, d_ekey, d_df);
    tb = tmp_bytes;
    SFM_HIP(rocprim::exclusive_scan(d_tmp, tb, d_df, d_wstart, (int64_t)0, (size_t)n_words + 1,
                                    rocprim::plus<int64_t>(), s));
    MD_LAUNCH(k_sp_post, g_kp, (const int64_t *)d_place, n_kp, (const int64_t *)d_epos, (const u64 *)d_ekey, word_bits,
              (const int32_t *)d_df, d_q, (const int64_t *)d_wstart, d_cursor, d_ev, d_pimg, d_pv);
    MD_LAUNCH(k_sp_norm2, dim3((unsigned)n_images), d_is, (const int64_t *)d_place, (const int32_t *)d_ev,
              out.ptr(o_norm2), d_root);
    const size_t lds = (size_t)n_images * 8 + (SP_THREADS / 64) * 16;
    if (lds > 48 * 1024)
        SFM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sp_query),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_sp_query, dim3((unsigned)n_images), dim3(SP_THREADS), lds, s, d_is,
                       (const int64_t *)d_place, (const u64 *)d_ekey, (const int32_t *)d_ev, word_bits,
                       (const int64_t *)d_wstart, (const int32_t *)d_pimg, (const int32_t *)d_pv,
                       (const double *)d_root, n_images, top_k, out.ptr(o_nb), out.ptr(o_score),
                       dot ? out.ptr(o_dot) : (int64_t *)nullptr);
    SFM_HIP(hipGetLastError());
    SFM_TRY(tm.mark(s));

    SFM_TRY(out.download(neighbour, o_nb, s));
    SFM_TRY(out.download(score, o_score, s));
    SFM_TRY(out.download(dot, o_dot, s));
    SFM_TRY(out.download(norm2, o_norm2, s));
    SFM_TRY(out.download(df, o_df, 0, (size_t)n_words, s));
    SFM_TRY(tm.finish(s));
    return 0;
}
