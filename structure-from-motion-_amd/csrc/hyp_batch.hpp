// The scaffold of the hypothesis-batch entry points (verify_pairs.hip,
// essential_pairs.hip, init_pairs.hip, register_views.hip, register_p3p.hip):
// CSR rows (pairs or views) of correspondences, a host-drawn table of H samples
// per row, a fit-and-score kernel on a flat grid over (row, hypothesis tile)
// and a winner-and-refit kernel with one workgroup per row.  A row below the
// entry point's minimum is dead: the host writes its outputs (info -1) and the
// device never reads it.
//
// The grid comes from a host prefix table over the live rows: blk_start
// (n_live + 1) holds each live row's first block, tab (n_live x 2) the row and
// the hypotheses per block chosen for it -- HT, HT / 2 from TILE
// correspondences, HT / 4 from 4 TILE, so that the score loop of a long row is
// spread over more blocks.  That loop stages the row through LDS in tiles of
// TILE correspondences, a wave per model, ballot popcount.
//
// Every sum runs in a fixed order over quantities of the row alone (strided
// per-thread partial sums, a 64-lane butterfly, the wave results added along a
// fixed tree) and counts are integers, so a row's outputs do not depend on the
// batch it is in.  The host part compiles without a device compiler
// (tests/hyp_batch_host.cpp).
#pragma once
#include "staging.hpp"

namespace sfm {

inline int64_t count_live(const int64_t *start, int64_t rows, int64_t min_n) {
    int64_t n_live = 0;
    for (int64_t r = 0; r < rows; ++r) n_live += start[r + 1] - start[r] >= min_n;
    return n_live;
}

// samples (rows x H x k): every entry of a row of n >= min_n items lies in
// [0, n), the k of a hypothesis are distinct; shorter rows are not looked at
inline int check_samples(const int64_t *start, int64_t rows, const int32_t *samples, int64_t H, int k, int64_t min_n,
                         const char *outside_msg) {
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t n = start[r + 1] - start[r];
        if (n < min_n) continue;
        for (int64_t h = 0; h < H; ++h) {
            const int32_t *s = samples + (r * H + h) * k;
            for (int a = 0; a < k; ++a) {
                SFM_CHECK_ARG(s[a] >= 0 && s[a] < n, outside_msg);
                for (int b = 0; b < a; ++b) SFM_CHECK_ARG(s[a] != s[b], "a hypothesis repeats a sample");
            }
        }
    }
    return 0;
}

// The block table as 3 n_live + 1 int32: blk_start, then tab.  n_live is the caller's count_live().
struct TileTable {
    int64_t n_live = 0, blocks = 0;
    const int32_t *blk = nullptr;
    size_t words() const { return (size_t)(3 * n_live + 1); }
    // the arithmetic alone: dst holds 3 live + 1 words
    int fill(int32_t *dst, int64_t live, const int64_t *start, int64_t rows, int64_t min_n, int64_t H, int HT,
             int TILE) {
        n_live = live;
        blocks = 0;
        blk = dst;
        int32_t *tab = dst + (n_live + 1);
        for (int64_t r = 0, j = 0; r < rows; ++r) {
            const int64_t n = start[r + 1] - start[r];
            if (n < min_n) continue;
            const int32_t ht = n >= 4 * TILE ? HT / 4 : (n >= TILE ? HT / 2 : HT);
            dst[j] = (int32_t)blocks;
            tab[2 * j] = (int32_t)r;
            tab[2 * j + 1] = ht;
            blocks += (H + ht - 1) / ht;
            SFM_CHECK_ARG(blocks <= (int64_t)0x7fffffff, "too many hypothesis tiles for one launch");
            ++j;
        }
        dst[n_live] = (int32_t)blocks;
        return 0;
    }
    // ... in pinned memory, from where it is uploaded
    int build(HostBuf &pinned, int64_t live, const int64_t *start, int64_t rows, int64_t min_n, int64_t H, int HT,
              int TILE) {
        SFM_TRY(pinned.reserve((size_t)(3 * live + 1) * sizeof(int32_t)));
        return fill(pinned.as<int32_t>(), live, start, rows, min_n, H, HT, TILE);
    }
};

// fn(r0, r1, k0, k1) for every maximal run [r0, r1) of live rows, [k0, k1) its
// items: live rows are copied out a run at a time, so that what the host wrote
// for the dead rows stays
template <class Fn> int for_each_live_run(const int64_t *start, int64_t rows, int64_t min_n, Fn fn) {
    for (int64_t r0 = 0, r1; r0 < rows; r0 = r1 + 1) {  // row r1, where the run ends, is dead or past the last
        for (r1 = r0; r1 < rows && start[r1 + 1] - start[r1] >= min_n;) ++r1;
        if (r1 > r0) SFM_TRY(fn(r0, r1, start[r0], start[r1]));
    }
    return 0;
}

// Ki = adj(K) / det K; returns det K.  Nothing is checked: a singular K gives
// entries that are not finite.
inline double inv3_adjugate(const double *K, double *Ki) {
    const double c0 = K[4] * K[8] - K[5] * K[7], c1 = K[5] * K[6] - K[3] * K[8], c2 = K[3] * K[7] - K[4] * K[6];
    const double det = (K[0] * c0 + K[1] * c1) + K[2] * c2;
    const double adj[9] = {c0, K[2] * K[7] - K[1] * K[8], K[1] * K[5] - K[2] * K[4],
                           c1, K[0] * K[8] - K[2] * K[6], K[2] * K[3] - K[0] * K[5],
                           c2, K[1] * K[6] - K[0] * K[7], K[0] * K[4] - K[1] * K[3]};
    for (int j = 0; j < 9; ++j) Ki[j] = adj[j] / det;
    return det;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------ device
struct HypTile {
    int32_t row, ht, hb, nh;  // the block's row, its hypotheses per block, the block's first and how many it has
};

// the live row of this block: the last j with blk_start[j] <= blockIdx.x
__device__ __forceinline__ HypTile tile_of_block(const int32_t *blk_start, const int32_t *tab, int32_t n_live,
                                                 int32_t H) {
    int lo = 0, hi = n_live - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk_start[mid] <= (int32_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int32_t ht = tab[2 * lo + 1], hb = ((int32_t)blockIdx.x - blk_start[lo]) * ht;
    return HypTile{tab[2 * lo], ht, hb, min(ht, H - hb)};
}

// sum over the 64 lanes by a butterfly: both partners add the same pair, so
// every lane holds the same bits
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) x += __shfl_xor(x, w);
    return x;
}

// Fixed-order sum of NV values over a workgroup of NW waves: the butterfly,
// then the wave results as 0 + 1 or (0 + 1) + (2 + 3).  red: NW x NV.  The
// butterfly is wave_sum's with the step as the outer loop -- NV independent
// shuffles a step, not NV chains of six: with wave_sum per element the refits
// that sum 29 values (k_rv_refine, register_refine.hpp) ran 2 % and 1 % slower.
template <int NW, int NV> __device__ __forceinline__ void wg_sum(double (&x)[NV], double (*red)[NV]) {
    static_assert(NW == 2 || NW == 4, "the tree over the wave results is written out");
#pragma unroll
    for (int w = 32; w > 0; w >>= 1)
#pragma unroll
        for (int j = 0; j < NV; ++j) x[j] += __shfl_xor(x[j], w);
    __syncthreads();  // the last use of red is over
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) red[threadIdx.x >> 6][j] = x[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if constexpr (NW == 2) x[j] = red[0][j] + red[1][j];
        else x[j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    }
}

// The row's n correspondences through LDS in tiles of TILE: stage(i, c) copies
// correspondence c of the row to place i of the tile (NT threads, strided),
// body(nt) scores the nt staged ones.  Owns the barriers.
template <int NT, int TILE, class Stage, class Body>
__device__ __forceinline__ void for_each_tile(int n, Stage stage, Body body) {
    for (int base = 0; base < n; base += TILE) {
        const int nt = min(TILE, n - base);
        for (int i = threadIdx.x; i < nt; i += NT) stage(i, base + i);
        __syncthreads();
        body(nt);
        __syncthreads();
    }
}

// how many i in [0, nt) pass pred, counted by this wave: 64 at a time, ballot popcount
template <class Pred> __device__ __forceinline__ int wave_count(int nt, Pred pred) {
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    for (int j = 0; j < nt; j += 64) {
        const int i = j + lane;
        bool in = false;
        if (i < nt) in = pred(i);
        cnt += __popcll(__ballot(in));
    }
    return cnt;
}

// the refitted state (n2 inliers at cost2) replaces the current one only if it is not worse
__device__ __forceinline__ bool not_worse(int n2, double cost2, int n, double cost) {
    return n2 > n || (n2 == n && cost2 <= cost);
}

// mask <- trial over the row (a thread reads and writes its own i = t, t + NT,
// ... alone); whether any entry changed, to every thread
template <int NT> __device__ __forceinline__ int adopt_trial(uint8_t *mask, const uint8_t *trial, int n) {
    int changed = 0;
    for (int i = threadIdx.x; i < n; i += NT) {
        changed |= mask[i] != trial[i];
        mask[i] = trial[i];
    }
    return __syncthreads_or(changed);
}
#endif  // __HIPCC__

}  // namespace sfm
