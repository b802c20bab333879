// Track merging: the match rows of a store that share a keypoint joined into
// tracks, on the device.  A matching-file line lists only the direct matches of
// one keypoint, so one scene point arrives as several rows; every incremental
// pipeline has this step between matching and geometry (union-find over
// keypoints, inconsistent tracks rejected).  The reference has no counterpart.
//
// The definitions (include/sfmcore.h) make every output a minimum or a sorted
// order, so the result does not depend on which thread arrives first:
//
//   k_mt_rows      the row of every observation (a thread per row).
//   k_mt_insert    keypoints: an open-addressed table of >= 2 n_obs slots that
//                  hold observation indices.  An empty slot is claimed by a
//                  compare-and-swap; an observation of the slot's key lowers it
//                  with atomicMin.  The slot's holder only ever changes among
//                  observations of one key, so comparing another key against
//                  whichever holder is read stays valid.  Linear probing,
//                  bounded by the table size (a full table sets a status word).
//   k_mt_keypoint  keypoint[i] = the holder of i's slot, in a launch of its own.
//   k_mt_union     components: a lock-free union-find over rows, one union per
//                  observation between its row and its keypoint's row.  The
//                  larger root is always hooked under the smaller, so a root
//                  is the smallest row of its component.
//   k_mt_flatten   component[r] = the root of r (parents no longer change).
//   k_mt_insert    again, keyed on (component, image) and fed the keypoints: a
//                  slot keeps the smallest keypoint of its key ...
//   k_mt_conflict  ... and a component is flagged when an observation's
//                  keypoint is not the one its slot kept.
//   k_mt_label     conflict, label and the head flag (label[r] == r) of a row;
//                  an exclusive scan of the heads numbers the tracks.
//   k_mt_emit      the observation that emits each distinct (label, keypoint):
//                  the keypoint itself in a clean component, the first
//                  observation of that keypoint inside a conflicting row that
//                  is kept; its 64-bit key (track, image, keypoint) and the
//                  track's count (integer atomicAdd).
//   rocPRIM        one radix sort of the keys orders the tracks and the
//                  observations inside them; an exclusive scan of the counts
//                  is track_start.
//   k_mt_scatter   track_obs and each emitter's position; k_mt_slot obs_slot.
//
// No thread waits for another: every retry follows a compare-and-swap that
// failed because another thread's succeeded, a walk to a root ends because
// parents only decrease, and dependent phases are separate launches.
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "staging.hpp"

namespace sfm {

constexpr int MT_THREADS = 256;
constexpr int32_t MT_EMPTY = 0x7fffffff;  // above every observation index (n_obs <= 2^30)

__device__ __forceinline__ int32_t mt_load(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t mt_mix(uint64_t h) {
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

// the bit pattern of a coordinate with -0.0 mapped to +0.0
__device__ __forceinline__ uint64_t mt_bits(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return b == 0x8000000000000000ull ? 0ull : b;
}

// The two tables' keys.  KEYPOINT: (image, x, y) of observation i.  COMPONENT:
// (component of i's row, image of i), i a keypoint.
struct MtKey {
    uint64_t a, b;
    uint32_t c;
    __device__ bool operator==(const MtKey &o) const { return a == o.a && b == o.b && c == o.c; }
    __device__ uint64_t hash() const { return mt_mix(a ^ mt_mix(b ^ mt_mix(c + 0x9e3779b97f4a7c15ull))); }
};

struct MtIn {
    const int32_t *image;
    const double *x, *y;
    const int32_t *obs_row, *component;
};

template <bool COMPONENT> __device__ __forceinline__ MtKey mt_key(const MtIn &in, int32_t i) {
    if (COMPONENT) return MtKey{(uint64_t)in.component[in.obs_row[i]], 0ull, (uint32_t)in.image[i]};
    return MtKey{mt_bits(in.x[i]), mt_bits(in.y[i]), (uint32_t)in.image[i]};
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_rows(const int64_t *row_start, int64_t n_rows, int32_t *obs_row) {
    const int64_t r = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    for (int64_t k = row_start[r]; k < row_start[r + 1]; ++k) obs_row[k] = (int32_t)r;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_fill(int32_t *p, int64_t n, int32_t value, int32_t iota) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n) p[i] = iota ? (int32_t)i : value;
}

// Observation i (COMPONENT: its keypoint) into the table; slot_of[i] is where.
template <bool COMPONENT>
__global__ __launch_bounds__(MT_THREADS) void k_mt_insert(MtIn in, const int32_t *keypoint, int64_t n_obs,
                                                          int32_t *table, uint32_t mask, uint32_t *slot_of,
                                                          int32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n_obs) return;
    const int32_t me = COMPONENT ? keypoint[i] : (int32_t)i;
    const MtKey key = mt_key<COMPONENT>(in, me);
    uint32_t slot = (uint32_t)key.hash() & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
        int32_t cur = mt_load(table + slot);
        if (cur == MT_EMPTY) {
            cur = atomicCAS(table + slot, MT_EMPTY, me);
            if (cur == MT_EMPTY) {
                slot_of[i] = slot;
                return;
            }
        }
        if (cur == me || mt_key<COMPONENT>(in, cur) == key) {
            if (me < cur) atomicMin(table + slot, me);
            slot_of[i] = slot;
            return;
        }
    }
    atomicOr(status, 1);  // the table is full: cannot happen with 2 n_obs slots
    slot_of[i] = 0;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_keypoint(const int32_t *table, const uint32_t *slot_of, int64_t n_obs,
                                                            int32_t *keypoint) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n_obs) keypoint[i] = table[slot_of[i]];
}

// the root of r; halves the path on the way (a parent only ever decreases, and
// every value written is an ancestor, so atomicMin keeps that true)
__device__ __forceinline__ int32_t mt_find(int32_t *parent, int32_t r) {
    int32_t p = mt_load(parent + r);
    while (p != r) {
        const int32_t g = mt_load(parent + p);
        if (g != p) atomicMin(parent + r, g);
        r = p;
        p = g;
    }
    return r;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_union(const int32_t *obs_row, const int32_t *keypoint, int64_t n_obs,
                                                         int32_t *parent) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n_obs) return;
    int32_t a = obs_row[i], b = obs_row[keypoint[i]];
    while (a != b) {
        a = mt_find(parent, a);
        b = mt_find(parent, b);
        if (a == b) break;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        // hi was a root when read: hook it under lo unless another union got
        // there first, in which case that union succeeded and this one retries
        if (atomicCAS(parent + hi, hi, lo) == hi) break;
    }
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_flatten(const int32_t *parent, int64_t n_rows, int32_t *component) {
    const int64_t r0 = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (r0 >= n_rows) return;
    int32_t r = (int32_t)r0, p = parent[r];
    while (p != r) {
        r = p;
        p = parent[r];
    }
    component[r0] = r;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_conflict(const int32_t *table, const uint32_t *slot_of,
                                                            const int32_t *keypoint, const int32_t *obs_row,
                                                            const int32_t *component, int64_t n_obs,
                                                            int32_t *comp_conflict) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n_obs) return;
    if (table[slot_of[i]] != keypoint[i]) comp_conflict[component[obs_row[i]]] = 1;  // every writer writes 1
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_label(const int32_t *component, const int32_t *comp_conflict,
                                                         int64_t n_rows, int32_t policy, uint8_t *conflict,
                                                         int32_t *label, int32_t *head) {
    const int64_t r = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (r > n_rows) return;
    if (r == n_rows) {
        head[r] = 0;  // so that the scan's last entry is the track count
        return;
    }
    const int32_t cf = comp_conflict[component[r]];
    const int32_t l = !cf ? component[r] : (policy == SFM_MERGE_DROP ? -1 : (int32_t)r);
    conflict[r] = (uint8_t)cf;
    label[r] = l;
    head[r] = l == (int32_t)r;
}

// emitter[i]: the observation that stands for (label of i's row, keypoint[i])
// in the output, -1 for a dropped row.  An emitter writes its sort key and
// counts for its track; every other observation's key sorts behind all tracks.
__global__ __launch_bounds__(MT_THREADS) void k_mt_emit(const int64_t *row_start, const int32_t *obs_row,
                                                        const int32_t *image, const int32_t *keypoint,
                                                        const uint8_t *conflict, const int32_t *label,
                                                        const int32_t *track_id, int64_t n_obs, int64_t n_rows,
                                                        int kp_bits, int img_bits, int32_t *emitter, uint64_t *keys,
                                                        int32_t *vals, int32_t *count) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= n_obs) return;
    const int32_t r = obs_row[i], l = label[r], kp = keypoint[i];
    int32_t e = -1;
    if (l >= 0) {
        e = kp;  // a clean component: the keypoint lies in one of its rows
        if (conflict[r]) {  // a kept row: the first observation of the row with this keypoint
            int64_t k = row_start[r];
            while (keypoint[k] != kp) ++k;
            e = (int32_t)k;
        }
    }
    emitter[i] = e;
    vals[i] = (int32_t)i;
    uint64_t t = (uint64_t)n_rows;
    if (e == (int32_t)i) {
        t = (uint64_t)track_id[l];
        atomicAdd(count + t, 1);
    }
    keys[i] = (t << (kp_bits + img_bits)) | ((uint64_t)image[i] << kp_bits) | (uint64_t)kp;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_heads(const int32_t *head, const int32_t *track_id, int64_t n_rows,
                                                         int32_t *track_label) {
    const int64_t r = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (r < n_rows && head[r]) track_label[track_id[r]] = (int32_t)r;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_scatter(const int32_t *sorted_vals, const int32_t *keypoint,
                                                           const int64_t *track_start, const int32_t *track_id,
                                                           int64_t n_obs, int64_t n_rows, int32_t *track_obs,
                                                           int32_t *position, int64_t *totals) {
    const int64_t p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    const int64_t n_emit = track_start[track_id[n_rows]];
    if (p == 0) {
        totals[0] = track_id[n_rows];
        totals[1] = n_emit;
    }
    if (p >= n_emit) return;  // the emitters sort first
    const int32_t e = sorted_vals[p];
    track_obs[p] = keypoint[e];
    position[e] = (int32_t)p;
}

__global__ __launch_bounds__(MT_THREADS) void k_mt_slot(const int32_t *emitter, const int32_t *position, int64_t n_obs,
                                                        int32_t *obs_slot) {
    const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i < n_obs) obs_slot[i] = emitter[i] >= 0 ? position[emitter[i]] : -1;
}

static int bits_for(uint64_t n) {  // bits that hold every value in [0, n]
    int b = 1;
    while (b < 64 && (n >> b)) ++b;
    return b;
}

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_merge_tracks(const int64_t *row_start, int64_t n_rows, const int32_t *image, const double *x,
                                const double *y, int64_t n_obs, int32_t n_images, int32_t policy, int32_t *keypoint,
                                int32_t *component, uint8_t *conflict, int32_t *label, int64_t *n_tracks,
                                int32_t *track_label, int64_t *track_start, int32_t *track_obs, int32_t *obs_slot,
                                int device) {
    SFM_CHECK_ARG(n_rows >= 0 && n_obs >= 0 && n_images >= 0, "n_rows < 0, n_obs < 0 or n_images < 0");
    SFM_CHECK_ARG(policy == SFM_MERGE_DROP || policy == SFM_MERGE_KEEP_ROWS, "unknown policy");
    SFM_CHECK_ARG(row_start && n_tracks, "null pointer");
    SFM_CHECK_ARG(n_obs <= (int64_t)1 << 30 && n_rows <= (int64_t)1 << 30, "more than 2^30 rows or observations");
    SFM_TRY(check_csr(row_start, n_rows, n_obs, "row_start", "observation"));
    SFM_CHECK_ARG(n_obs == 0 || (image && x && y), "null pointer");
    SFM_TRY(check_index(image, n_obs, n_images, "an image outside [0, n_images)"));
    for (int64_t k = 0; k < n_obs; ++k)
        SFM_CHECK_ARG(std::isfinite(x[k]) && std::isfinite(y[k]), "a coordinate is not finite");
    // the sort key: (track or n_rows, image, keypoint)
    const int kp_bits = bits_for((uint64_t)n_obs), img_bits = bits_for((uint64_t)n_images);
    const int trk_bits = bits_for((uint64_t)n_rows);
    SFM_CHECK_ARG(kp_bits + img_bits + trk_bits <= 64, "n_rows x n_images x n_obs too large for one 64-bit sort key");

    *n_tracks = 0;
    if (track_start) track_start[0] = 0;
    if (n_rows == 0) return 0;
    if (n_obs == 0) {  // rows without observations: each its own component, no track has an observation
        for (int64_t r = 0; r < n_rows; ++r) {
            if (component) component[r] = (int32_t)r;
            if (label) label[r] = (int32_t)r;
            if (track_label) track_label[r] = (int32_t)r;
            if (conflict) conflict[r] = 0;
            if (track_start) track_start[r + 1] = 0;
        }
        *n_tracks = n_rows;
        return 0;
    }

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    uint64_t slots = 1024;
    while (slots < 2 * (uint64_t)n_obs) slots <<= 1;
    const uint32_t mask = (uint32_t)(slots - 1);

    // rocPRIM's scratch: sizes first (no device work), the largest is reserved
    size_t tmp_sort = 0, tmp_scan32 = 0, tmp_scan64 = 0;
    SFM_HIP(rocprim::radix_sort_pairs(nullptr, tmp_sort, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                      (int32_t *)nullptr, (size_t)n_obs, 0, kp_bits + img_bits + trk_bits, s));
    SFM_HIP(rocprim::exclusive_scan(nullptr, tmp_scan32, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0,
                                    (size_t)n_rows + 1, rocprim::plus<int32_t>(), s));
    SFM_HIP(rocprim::exclusive_scan(nullptr, tmp_scan64, (int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0,
                                    (size_t)n_rows + 1, rocprim::plus<int64_t>(), s));
    size_t tmp_bytes = tmp_sort > tmp_scan32 ? tmp_sort : tmp_scan32;
    if (tmp_scan64 > tmp_bytes) tmp_bytes = tmp_scan64;

    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_rs = in.add<int64_t>(n_rows + 1);
    const auto i_img = in.add<int32_t>(n_obs);
    const auto i_x = in.add<double>(n_obs), i_y = in.add<double>(n_obs);
    const auto o_kp = out.add<int32_t>(n_obs), o_slot = out.add<int32_t>(n_obs), o_tobs = out.add<int32_t>(n_obs);
    const auto o_comp = out.add<int32_t>(n_rows), o_label = out.add<int32_t>(n_rows), o_tl = out.add<int32_t>(n_rows);
    const auto o_cf = out.add<uint8_t>(n_rows);
    const auto o_ts = out.add<int64_t>(n_rows + 1);
    const auto o_tid = out.add<int32_t>(n_rows + 1);  // its last entry is the track count
    const auto o_status = out.add<int32_t>(1);
    const auto o_tot = out.add<int64_t>(2);  // n_tracks and the length of track_obs
    const auto w_table = work.add<int32_t>(slots);
    const auto w_slot_of = work.add<uint32_t>(n_obs);
    const auto w_row = work.add<int32_t>(n_obs), w_emit = work.add<int32_t>(n_obs), w_pos = work.add<int32_t>(n_obs);
    const auto w_parent = work.add<int32_t>(n_rows), w_ccf = work.add<int32_t>(n_rows);
    const auto w_head = work.add<int32_t>(n_rows + 1), w_count = work.add<int32_t>(n_rows + 1);
    const auto w_k0 = work.add<uint64_t>(n_obs), w_k1 = work.add<uint64_t>(n_obs);
    const auto w_v0 = work.add<int32_t>(n_obs), w_v1 = work.add<int32_t>(n_obs);
    const auto w_tmp = work.add<char>(tmp_bytes);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_rs, row_start, s));
    SFM_TRY(in.upload(i_img, image, s));
    SFM_TRY(in.upload(i_x, x, s));
    SFM_TRY(in.upload(i_y, y, s));
    SFM_TRY(tm.mark(s));

    const dim3 T(MT_THREADS);
    const dim3 g_obs((unsigned)ceil_div(n_obs, MT_THREADS)), g_rows((unsigned)ceil_div(n_rows + 1, MT_THREADS));
    const dim3 g_table((unsigned)ceil_div((int64_t)slots, MT_THREADS));
    int32_t *table = work.ptr(w_table), *obs_row = work.ptr(w_row), *parent = work.ptr(w_parent);
    int32_t *d_kp = out.ptr(o_kp), *d_comp = out.ptr(o_comp), *d_label = out.ptr(o_label), *d_tid = out.ptr(o_tid);
    int32_t *d_status = out.ptr(o_status);
    uint32_t *slot_of = work.ptr(w_slot_of);
    const MtIn mi{in.ptr(i_img), in.ptr(i_x), in.ptr(i_y), obs_row, d_comp};
#define MT_LAUNCH(kernel, grid, ...)                                  \
    do {                                                              \
        hipLaunchKernelGGL(kernel, grid, T, 0, s, __VA_ARGS__);       \
        SFM_HIP(hipGetLastError());                                   \
    } while (0)
    SFM_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    MT_LAUNCH(k_mt_rows, g_rows, in.ptr(i_rs), n_rows, obs_row);
    // keypoints
    MT_LAUNCH(k_mt_fill, g_table, table, (int64_t)slots, MT_EMPTY, 0);
    MT_LAUNCH(k_mt_insert<false>, g_obs, mi, (const int32_t *)nullptr, n_obs, table, mask, slot_of, d_status);
    MT_LAUNCH(k_mt_keypoint, g_obs, table, slot_of, n_obs, d_kp);
    // components
    MT_LAUNCH(k_mt_fill, g_rows, parent, n_rows, 0, 1);
    MT_LAUNCH(k_mt_union, g_obs, obs_row, d_kp, n_obs, parent);
    MT_LAUNCH(k_mt_flatten, g_rows, parent, n_rows, d_comp);
    // conflicts
    MT_LAUNCH(k_mt_fill, g_table, table, (int64_t)slots, MT_EMPTY, 0);
    MT_LAUNCH(k_mt_insert<true>, g_obs, mi, d_kp, n_obs, table, mask, slot_of, d_status);
    SFM_HIP(hipMemsetAsync(work.ptr(w_ccf), 0, w_ccf.bytes(), s));
    MT_LAUNCH(k_mt_conflict, g_obs, table, slot_of, d_kp, obs_row, d_comp, n_obs, work.ptr(w_ccf));
    MT_LAUNCH(k_mt_label, g_rows, d_comp, work.ptr(w_ccf), n_rows, policy, out.ptr(o_cf), d_label, work.ptr(w_head));
    // tracks
    size_t tb = tmp_bytes;
    SFM_HIP(rocprim::exclusive_scan(work.ptr(w_tmp), tb, work.ptr(w_head), d_tid, (int32_t)0, (size_t)n_rows + 1,
                                    rocprim::plus<int32_t>(), s));
    MT_LAUNCH(k_mt_heads, g_rows, work.ptr(w_head), d_tid, n_rows, out.ptr(o_tl));
    SFM_HIP(hipMemsetAsync(work.ptr(w_count), 0, w_count.bytes(), s));
    MT_LAUNCH(k_mt_emit, g_obs, in.ptr(i_rs), obs_row, in.ptr(i_img), d_kp, out.ptr(o_cf), d_label, d_tid, n_obs, n_rows,
              kp_bits, img_bits, work.ptr(w_emit), work.ptr(w_k0), work.ptr(w_v0), work.ptr(w_count));
    tb = tmp_bytes;
    SFM_HIP(rocprim::exclusive_scan(work.ptr(w_tmp), tb, work.ptr(w_count), out.ptr(o_ts), (int64_t)0,
                                    (size_t)n_rows + 1, rocprim::plus<int64_t>(), s));
    tb = tmp_bytes;
    SFM_HIP(rocprim::radix_sort_pairs(work.ptr(w_tmp), tb, work.ptr(w_k0), work.ptr(w_k1), work.ptr(w_v0),
                                      work.ptr(w_v1), (size_t)n_obs, 0, kp_bits + img_bits + trk_bits, s));
    MT_LAUNCH(k_mt_scatter, g_obs, work.ptr(w_v1), d_kp, out.ptr(o_ts), d_tid, n_obs, n_rows, out.ptr(o_tobs),
              work.ptr(w_pos), out.ptr(o_tot));
    MT_LAUNCH(k_mt_slot, g_obs, work.ptr(w_emit), work.ptr(w_pos), n_obs, out.ptr(o_slot));
#undef MT_LAUNCH
    SFM_TRY(tm.mark(s));

    // the counts first: they size the other copies
    int64_t tot[2] = {0, 0};
    int32_t status = 0;
    SFM_TRY(out.download(tot, o_tot, s));
    SFM_TRY(out.download(&status, o_status, s));
    SFM_HIP(hipStreamSynchronize(s));
    if (status != 0) {
        set_error("merge_tracks: a hash table filled up");
        return SFM_ERR_HIP;
    }
    const size_t nt = (size_t)tot[0];
    SFM_TRY(out.download(track_start, o_ts, 0, nt + 1, s));
    SFM_TRY(out.download(track_label, o_tl, 0, nt, s));
    SFM_TRY(out.download(component, o_comp, s));
    SFM_TRY(out.download(conflict, o_cf, s));
    SFM_TRY(out.download(label, o_label, s));
    SFM_TRY(out.download(keypoint, o_kp, s));
    SFM_TRY(out.download(obs_slot, o_slot, s));
    SFM_TRY(out.download(track_obs, o_tobs, 0, (size_t)tot[1], s));
    SFM_TRY(tm.finish(s));
    *n_tracks = (int64_t)nt;
    return 0;
}
