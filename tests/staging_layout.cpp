// Stand-alone check of csrc/staging.hpp's packed-buffer arithmetic (built and
// run by tests/test_staging.py, host only, under ASan + UBSan).  No device
// call is made: a Pack that was never reserved has no device memory, and every
// HIP call of the header sits behind reserve().
//
//   staging_layout             the checks; exit status 0 and "ok" when they hold
//   staging_layout early-ptr   asks for a device pointer before reserve(): must abort
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "staging.hpp"

// what libsfmcore's sfm_api.hip defines for the header
namespace sfm {
void set_error(const char *, ...) {}
void set_timings(const double *, int) {}
bool call_timing() { return false; }
}  // namespace sfm

using namespace sfm;

static int failures = 0;
#define EXPECT_EQ(a, b)                                                                                      \
    do {                                                                                                     \
        const size_t a_ = (size_t)(a), b_ = (size_t)(b);                                                     \
        if (a_ != b_) {                                                                                      \
            std::printf("%s:%d: %s = %zu, %s = %zu\n", __FILE__, __LINE__, #a, a_, #b, b_);                  \
            ++failures;                                                                                      \
        }                                                                                                    \
    } while (0)

// the rounding of the per-file helpers this header replaces
static size_t ref_up256(size_t n) { return (n + 255) & ~(size_t)255; }

static void rounding() {
    EXPECT_EQ(up256(0), 0);
    EXPECT_EQ(up256(1), 256);
    EXPECT_EQ(up256(255), 256);
    EXPECT_EQ(up256(256), 256);
    EXPECT_EQ(up256(257), 512);
    for (size_t n = 0; n < 2000; ++n) EXPECT_EQ(up256(n), ref_up256(n));
}

static void alignment_and_empty_slots() {
    DevBuf buf;
    Pack p(buf);
    const auto a = p.add<uint8_t>(1);
    const auto z = p.add<double>(0);  // an absent array
    const auto b = p.add<int32_t>(65);
    const auto c = p.add<double2>(3);
    EXPECT_EQ(a.off, 0);
    EXPECT_EQ(z.off, 256);
    EXPECT_EQ(z.bytes(), 0);
    EXPECT_EQ(b.off, 256);  // the empty slot took up256(0) = 0 bytes
    EXPECT_EQ(c.off, 256 + 512);
    EXPECT_EQ(p.bytes(), 256 + 512 + 256);
    for (size_t off : {a.off, z.off, b.off, c.off, p.bytes()}) EXPECT_EQ(off % 256, 0);
    // no bytes, or no host array: no copy, so no HIP call and no device pointer -- before reserve() either would abort
    double host[1] = {0.0};
    EXPECT_EQ(p.upload(z, host, nullptr), 0);
    EXPECT_EQ(p.download(host, z, nullptr), 0);
    EXPECT_EQ(p.upload(b, nullptr, nullptr), 0);
    EXPECT_EQ(p.download(nullptr, b, nullptr), 0);
    EXPECT_EQ(p.upload(b, host, 7, 0, nullptr), 0);
    EXPECT_EQ(p.download(host, b, 7, 0, nullptr), 0);
}

// sfm_triangulate_tracks before the helper (multiview.hip)
static void multiview(int64_t T, int64_t n_obs, int32_t n_cams) {
    const size_t b_ts = (size_t)(T + 1) * sizeof(int64_t), b_xy = (size_t)n_obs * sizeof(double2),
                 b_cam = (size_t)n_obs * sizeof(int32_t), b_x = (size_t)T * 3 * sizeof(double),
                 b_p = (size_t)n_cams * 12 * sizeof(double);
    const size_t o_xy = ref_up256(b_ts), o_cam = o_xy + ref_up256(b_xy), o_x0 = o_cam + ref_up256(b_cam),
                 o_p = o_x0 + ref_up256(b_x), in_bytes = o_p + ref_up256(b_p);
    const size_t o_cost = ref_up256(b_x), o_info = o_cost + ref_up256((size_t)T * sizeof(double)),
                 o_front = o_info + ref_up256((size_t)T * sizeof(int32_t)), out_bytes = o_front + ref_up256((size_t)T);
    DevBuf b0, b1;
    Pack in(b0), out(b1);
    const auto i_ts = in.add<int64_t>(T + 1);
    const auto i_xy = in.add<double2>(n_obs);
    const auto i_cam = in.add<int32_t>(n_obs);
    const auto i_x0 = in.add<double>(3 * T);
    const auto i_p = in.add<double>(12 * (size_t)n_cams);
    const auto s_x = out.add<double>(3 * T);
    const auto s_cost = out.add<double>(T);
    const auto s_info = out.add<int32_t>(T);
    const auto s_front = out.add<uint8_t>(T);
    EXPECT_EQ(i_ts.off, 0);
    EXPECT_EQ(i_ts.bytes(), b_ts);
    EXPECT_EQ(i_xy.off, o_xy);
    EXPECT_EQ(i_xy.bytes(), b_xy);
    EXPECT_EQ(i_cam.off, o_cam);
    EXPECT_EQ(i_cam.bytes(), b_cam);
    EXPECT_EQ(i_x0.off, o_x0);
    EXPECT_EQ(i_x0.bytes(), b_x);
    EXPECT_EQ(i_p.off, o_p);
    EXPECT_EQ(i_p.bytes(), b_p);
    EXPECT_EQ(in.bytes(), in_bytes);
    EXPECT_EQ(s_x.off, 0);
    EXPECT_EQ(s_x.bytes(), b_x);
    EXPECT_EQ(s_cost.off, o_cost);
    EXPECT_EQ(s_info.off, o_info);
    EXPECT_EQ(s_front.off, o_front);
    EXPECT_EQ(s_front.bytes(), T);
    EXPECT_EQ(out.bytes(), out_bytes);
}

// sfm_triangulate_tracks_robust before the helper (robust_tracks.hip)
static void robust_tracks(int64_t T, int64_t n_obs, int32_t n_cams) {
    const size_t b_ts = (size_t)(T + 1) * sizeof(int64_t), b_xy = (size_t)n_obs * sizeof(double2),
                 b_cam = (size_t)n_obs * sizeof(int32_t), b_x = (size_t)T * 3 * sizeof(double),
                 b_c = (size_t)n_cams * 3 * sizeof(double), b_p = (size_t)n_cams * 12 * sizeof(double),
                 b_d = (size_t)T * sizeof(double), b_i = (size_t)T * sizeof(int32_t);
    const size_t o_xy = ref_up256(b_ts), o_cam = o_xy + ref_up256(b_xy), o_c = o_cam + ref_up256(b_cam),
                 o_p = o_c + ref_up256(b_c), in_bytes = o_p + ref_up256(b_p);
    const size_t o_cost = ref_up256(b_x), o_ang = o_cost + ref_up256(b_d), o_info = o_ang + ref_up256(b_d),
                 o_ninl = o_info + ref_up256(b_i), o_pair = o_ninl + ref_up256(b_i), o_cnt = o_pair + ref_up256(b_i),
                 o_mask = o_cnt + ref_up256(b_i), out_bytes = o_mask + ref_up256((size_t)n_obs);
    DevBuf b0, b1;
    Pack in(b0), out(b1);
    const auto i_ts = in.add<int64_t>(T + 1);
    const auto i_xy = in.add<double2>(n_obs);
    const auto i_cam = in.add<int32_t>(n_obs);
    const auto i_c = in.add<double>(3 * (size_t)n_cams);
    const auto i_p = in.add<double>(12 * (size_t)n_cams);
    const auto s_x = out.add<double>(3 * T);
    const auto s_cost = out.add<double>(T);
    const auto s_ang = out.add<double>(T);
    const auto s_info = out.add<int32_t>(T);
    const auto s_ninl = out.add<int32_t>(T);
    const auto s_pair = out.add<int32_t>(T);
    const auto s_cnt = out.add<int32_t>(T);
    const auto s_mask = out.add<uint8_t>(n_obs);
    EXPECT_EQ(i_ts.off, 0);
    EXPECT_EQ(i_xy.off, o_xy);
    EXPECT_EQ(i_cam.off, o_cam);
    EXPECT_EQ(i_c.off, o_c);
    EXPECT_EQ(i_c.bytes(), b_c);
    EXPECT_EQ(i_p.off, o_p);
    EXPECT_EQ(i_p.bytes(), b_p);
    EXPECT_EQ(in.bytes(), in_bytes);
    EXPECT_EQ(s_x.off, 0);
    EXPECT_EQ(s_cost.off, o_cost);
    EXPECT_EQ(s_ang.off, o_ang);
    EXPECT_EQ(s_info.off, o_info);
    EXPECT_EQ(s_ninl.off, o_ninl);
    EXPECT_EQ(s_pair.off, o_pair);
    EXPECT_EQ(s_cnt.off, o_cnt);
    EXPECT_EQ(s_cnt.bytes(), b_i);
    EXPECT_EQ(s_mask.off, o_mask);
    EXPECT_EQ(s_mask.bytes(), n_obs);
    EXPECT_EQ(out.bytes(), out_bytes);
}

// sfm_register_views before the helper (register_views.hip)
static void register_views(int64_t V, int64_t H, int64_t n_corr, int64_t n_pts, int64_t n_live) {
    const size_t VH = (size_t)V * (size_t)H;
    const size_t b_vs = (size_t)(V + 1) * sizeof(int64_t), b_xy = (size_t)n_corr * sizeof(double2),
                 b_X = (size_t)n_pts * 3 * sizeof(double), b_pt = (size_t)n_corr * sizeof(int32_t),
                 b_s = VH * 6 * sizeof(int32_t), b_t = (size_t)(3 * n_live + 1) * sizeof(int32_t);
    const size_t o_xy = ref_up256(b_vs), o_X = o_xy + ref_up256(b_xy), o_pt = o_X + ref_up256(b_X),
                 o_s = o_pt + ref_up256(b_pt), o_t = o_s + ref_up256(b_s), in_bytes = o_t + ref_up256(b_t);
    const size_t b_C = (size_t)V * 3 * sizeof(double), b_R = (size_t)V * 9 * sizeof(double),
                 b_d = (size_t)V * sizeof(double), b_i = (size_t)V * sizeof(int32_t), b_cnt = VH * sizeof(int32_t),
                 b_m = VH * 12 * sizeof(double);
    const size_t o_R = ref_up256(b_C), o_cost = o_R + ref_up256(b_R), o_info = o_cost + ref_up256(b_d),
                 o_ninl = o_info + ref_up256(b_i), o_hyp = o_ninl + ref_up256(b_i), o_bc = o_hyp + ref_up256(b_i),
                 o_cnt = o_bc + ref_up256(b_i), o_mP = o_cnt + ref_up256(b_cnt), o_mCR = o_mP + ref_up256(b_m),
                 o_mask = o_mCR + ref_up256(b_m), o_m2 = o_mask + ref_up256((size_t)n_corr),
                 out_bytes = o_m2 + ref_up256((size_t)n_corr);
    DevBuf b0, b1;
    Pack in(b0), out(b1);
    const auto i_vs = in.add<int64_t>(V + 1);
    const auto i_xy = in.add<double2>(n_corr);
    const auto i_X = in.add<double>(3 * n_pts);
    const auto i_pt = in.add<int32_t>(n_corr);
    const auto i_s = in.add<int32_t>(6 * VH);
    const auto i_t = in.add<int32_t>(3 * n_live + 1);
    const auto s_C = out.add<double>(3 * V);
    const auto s_R = out.add<double>(9 * V);
    const auto s_cost = out.add<double>(V);
    const auto s_info = out.add<int32_t>(V);
    const auto s_ninl = out.add<int32_t>(V);
    const auto s_hyp = out.add<int32_t>(V);
    const auto s_bc = out.add<int32_t>(V);
    const auto s_cnt = out.add<int32_t>(VH);
    const auto s_mP = out.add<double>(12 * VH);
    const auto s_mCR = out.add<double>(12 * VH);
    const auto s_mask = out.add<uint8_t>(n_corr);
    const auto s_m2 = out.add<uint8_t>(n_corr);
    EXPECT_EQ(i_vs.off, 0);
    EXPECT_EQ(i_vs.bytes(), b_vs);
    EXPECT_EQ(i_xy.off, o_xy);
    EXPECT_EQ(i_X.off, o_X);
    EXPECT_EQ(i_X.bytes(), b_X);
    EXPECT_EQ(i_pt.off, o_pt);
    EXPECT_EQ(i_s.off, o_s);
    EXPECT_EQ(i_s.bytes(), b_s);
    EXPECT_EQ(i_t.off, o_t);
    EXPECT_EQ(i_t.bytes(), b_t);
    EXPECT_EQ(in.bytes(), in_bytes);
    EXPECT_EQ(s_C.off, 0);
    EXPECT_EQ(s_C.bytes(), b_C);
    EXPECT_EQ(s_R.off, o_R);
    EXPECT_EQ(s_R.bytes(), b_R);
    EXPECT_EQ(s_cost.off, o_cost);
    EXPECT_EQ(s_info.off, o_info);
    EXPECT_EQ(s_ninl.off, o_ninl);
    EXPECT_EQ(s_hyp.off, o_hyp);
    EXPECT_EQ(s_bc.off, o_bc);
    EXPECT_EQ(s_cnt.off, o_cnt);
    EXPECT_EQ(s_cnt.bytes(), b_cnt);
    EXPECT_EQ(s_mP.off, o_mP);
    EXPECT_EQ(s_mP.bytes(), b_m);
    EXPECT_EQ(s_mCR.off, o_mCR);
    EXPECT_EQ(s_mask.off, o_mask);
    EXPECT_EQ(s_m2.off, o_m2);
    EXPECT_EQ(out.bytes(), out_bytes);
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "early-ptr")) {
        DevBuf buf;
        Pack p(buf);
        const auto s = p.add<double>(4);
        std::printf("%p\n", (void *)p.ptr(s));  // aborts: no reserve() yet
        return 0;
    }
    rounding();
    alignment_and_empty_slots();
    multiview(257, 1000, 5);
    robust_tracks(257, 1000, 5);
    register_views(3, 64, 40, 20, 2);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
