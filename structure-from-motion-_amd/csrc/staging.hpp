// Host-side staging shared by the per-call entry points: the layout of a
// packed device buffer with its copies (Pack), the HIP-event phase timer of a
// call (CallTimer) and the argument checks of CSR rows.  Host code only.
#pragma once
#include "sfm_common.hpp"

namespace sfm {

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// `count` elements of T at byte offset `off` of a Pack.
template <class T> struct Slot {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
};

// Several arrays in one DevBuf, each on a 256-byte boundary in the order of
// the add() calls.  DevBuf::reserve frees and reallocates, so device addresses
// exist only after reserve(): ptr() and the copies abort before it, add()
// after it.  A copy of no bytes, or from / to a null host pointer (an
// optional array), issues no HIP call.
class Pack {
  public:
    explicit Pack(DevBuf &buf) : buf_(buf) {}
    template <class T> Slot<T> add(size_t count) {
        require(!reserved_, "add() after reserve()");
        const Slot<T> s{bytes_, count};
        bytes_ += up256(s.bytes());
        return s;
    }
    size_t bytes() const { return bytes_; }
    int reserve() {
        const int rc = buf_.reserve(bytes_);
        reserved_ = rc == 0;
        return rc;
    }
    // device address of element `first` of the slot
    template <class T> T *ptr(Slot<T> s, size_t first = 0) const {
        require(reserved_, "device pointer before reserve()");
        return reinterpret_cast<T *>(buf_.as<char>() + s.off) + first;
    }
    // host -> slot and slot -> host: the whole slot, or `count` elements from
    // element `first` on (`host` is then that element's place on the host)
    template <class T> int upload(Slot<T> s, const void *h, hipStream_t st) const { return upload(s, h, 0, s.count, st); }
    template <class T> int upload(Slot<T> s, const void *host, size_t first, size_t count, hipStream_t st) const {
        if (count && host) SFM_HIP(hipMemcpyAsync(ptr(s, first), host, count * sizeof(T), hipMemcpyHostToDevice, st));
        return 0;
    }
    template <class T> int download(void *h, Slot<T> s, hipStream_t st) const { return download(h, s, 0, s.count, st); }
    template <class T> int download(void *host, Slot<T> s, size_t first, size_t count, hipStream_t st) const {
        if (count && host) SFM_HIP(hipMemcpyAsync(host, ptr(s, first), count * sizeof(T), hipMemcpyDeviceToHost, st));
        return 0;
    }
    // rows [r0, r1) of `per` elements each, to their place in the host array of all rows
    template <class T> int download_rows(T *host, Slot<T> s, size_t per, int64_t r0, int64_t r1, hipStream_t st) const {
        return host ? download(host + per * r0, s, per * r0, per * (size_t)(r1 - r0), st) : 0;
    }

  private:
    static void require(bool ok, const char *what) {
        if (ok) return;
        std::fprintf(stderr, "sfm::Pack: %s\n", what);
        std::abort();
    }
    DevBuf &buf_;
    size_t bytes_ = 0;
    bool reserved_ = false;
};

// sfm_last_timings of a call in four slots: [0] upload, [1] kernels, [2]
// download, [3] the kernels again or, after split(), the kernels up to it.
// mark() before the uploads, after them and after the kernels (ev[0..2]);
// finish() after the downloads: ev[3], the synchronise and the four slots.
// With call timing off no event is recorded and the slots are zero.
class CallTimer {
  public:
    explicit CallTimer(ThreadCtx *c) : c_(c), on_(call_timing()) {}
    int mark(hipStream_t s) { return record(n_++, s); }
    int split(hipStream_t s) { return record(split_ = 4, s); }
    int finish(hipStream_t s) {
        SFM_TRY(record(3, s));
        SFM_HIP(hipStreamSynchronize(s));
        float t[5] = {0, 0, 0, 0, 0};
        for (int k = 0; on_ && k < 3; ++k) (void)hipEventElapsedTime(&t[k], c_->ev[k], c_->ev[k + 1]);
        if (on_ && split_) (void)hipEventElapsedTime(&t[4], c_->ev[1], c_->ev[split_]);
        const double t4[4] = {t[0], t[1], t[2], split_ ? t[4] : t[1]};
        set_timings(t4, 4);
        return 0;
    }

  private:
    int record(int k, hipStream_t s) {
        if (on_) SFM_HIP(hipEventRecord(c_->ev[k], s));  // HIP events only when asked (each costs the stream us)
        return 0;
    }
    ThreadCtx *c_;
    bool on_;
    int n_ = 0, split_ = 0;
};

// CSR row starts: start[0] == 0, no row of negative length (nor, where
// max_row is given, of more than max_row items: `too_long` is that message),
// start[rows] == n_items.  `name` is the array's, `item` what a row holds.
inline int check_csr(const int64_t *start, int64_t rows, int64_t n_items, const std::string &name, const char *item,
                     int64_t max_row = INT64_MAX, const char *too_long = "") {
    SFM_CHECK_ARG(start[0] == 0, (name + " does not start at 0").c_str());
    for (int64_t r = 0; r < rows; ++r) {
        SFM_CHECK_ARG(start[r + 1] >= start[r], (name + " decreases").c_str());
        SFM_CHECK_ARG(start[r + 1] - start[r] <= max_row, too_long);
    }
    SFM_CHECK_ARG(start[rows] == n_items, (name + " does not end at the " + item + " count").c_str());
    return 0;
}

// every idx[k] in [0, n_targets): an index out of range is an error here,
// never a device read.  `msg` is the whole message.
inline int check_index(const int32_t *idx, int64_t n_items, int64_t n_targets, const char *msg) {
    for (int64_t k = 0; k < n_items; ++k) SFM_CHECK_ARG(idx[k] >= 0 && idx[k] < n_targets, msg);
    return 0;
}

}  // namespace sfm
