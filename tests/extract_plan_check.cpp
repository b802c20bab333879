// Stand-alone check of csrc/extract_plan.hpp: the octave sizes and offsets of
// a pyramid, the blur taps, the candidate bound, the chunk size and the
// candidate key of feature extraction (built and run by
// tests/test_extract_plan.py, host only, under ASan + UBSan).  No device call.
#include <cstdio>
#include <cstdlib>

#include "extract_plan.hpp"

using namespace sfm;

static int failures = 0;
#define EXPECT(cond)                                                 \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void octaves() {
    EXPECT(ef_max_octaves(16, 16) == 1);
    EXPECT(ef_max_octaves(15, 400) == 0);
    EXPECT(ef_max_octaves(31, 31) == 2);
    EXPECT(ef_max_octaves(32, 32) == 2);
    EXPECT(ef_max_octaves(97, 130) == 3);
    EXPECT(ef_max_octaves(1200, 1600) == 7);
    EXPECT(ef_max_octaves(65536, 65536) == 13);
    const EfLayout L = ef_layout(33, 47, 2);
    EXPECT(L.h[0] == 33 && L.w[0] == 47 && L.h[1] == 17 && L.w[1] == 24);
    EXPECT(L.off[0] == 0 && L.off[1] == 6 * 33 * 47 && L.per_image == 6 * (33 * 47 + 17 * 24));
    EXPECT(L.cand_bound == 3 * 2 * (17 * 24 + 9 * 12));
    for (int64_t h = 16; h < 80; h += 7)
        for (int64_t w = 16; w < 300; w += 31) {
            const int n = ef_max_octaves(h, w);
            const EfLayout M = ef_layout(h, w, n);
            EXPECT(n >= 1 && M.h[n - 1] >= 16 && M.w[n - 1] >= 16);
            for (int o = 1; o < n; ++o) {
                EXPECT(M.h[o] == (M.h[o - 1] + 1) / 2 && M.w[o] == (M.w[o - 1] + 1) / 2);
                EXPECT(2 * (M.h[o] - 1) <= M.h[o - 1] - 1 && 2 * (M.w[o] - 1) <= M.w[o - 1] - 1);  // the down-sample's reads
                EXPECT(M.off[o] == M.off[o - 1] + (int64_t)6 * M.h[o - 1] * M.w[o - 1]);
            }
        }
}

static void taps() {
    EfTaps t;
    EXPECT(ef_taps(ef_sigma_inc(1.6, 0), t) && t.R == 7);
    EXPECT(ef_taps(ef_sigma_inc(1.6, 5), t) && t.R == 13);
    EXPECT(ef_max_radius(1.6) == 13 && ef_max_radius(3.2) <= EF_MAX_R && ef_max_radius(3.3) > EF_MAX_R);
    EXPECT(!ef_taps(7.0, t));
    for (double s = 0.3; s < 6.2; s += 0.37) {
        if (!ef_taps(s, t)) {
            EXPECT(ef_radius(s) > EF_MAX_R);
            continue;
        }
        double sum = 0.0;
        for (int k = 0; k <= 2 * t.R; ++k) {
            sum += t.w[k];
            EXPECT(t.w[k] >= 0.0f && t.w[k] == t.w[2 * t.R - k]);
        }
        EXPECT(std::fabs(sum - 1.0) < 1e-6);
        for (int k = 2 * t.R + 1; k <= 2 * EF_MAX_R; ++k) EXPECT(t.w[k] == 0.0f);
    }
}

static void chunks() {
    const EfLayout L = ef_layout(1200, 1600, 7);
    const int64_t n = ef_chunk_images(L, 1200, 1600, 200);
    EXPECT(n >= 1 && n <= 200 && ef_chunk_bytes(L, 1200, 1600, n) <= EF_WS_BYTES);
    EXPECT(ef_chunk_bytes(L, 1200, 1600, n + 1) > EF_WS_BYTES);
    EXPECT(ef_chunk_images(L, 1200, 1600, 1) == 1);
    const EfLayout S = ef_layout(16, 16, 1);
    EXPECT(ef_chunk_images(S, 16, 16, 100000) == EF_MAX_CHUNK);
    EXPECT(ef_cand_capacity(S, 3) == 3 * S.cand_bound && ef_cand_capacity(L, 200) == EF_MAX_CAND);
    const EfLayout B = ef_layout(65536, 65536, 13);  // one image above the workspace: still one image per chunk
    EXPECT(ef_chunk_images(B, 65536, 65536, 5) == 1);
}

static void keys() {
    int32_t f[5];
    ef_unkey(ef_key(255, 12, 3, 65530, 65535), f);
    EXPECT(f[0] == 255 && f[1] == 12 && f[2] == 3 && f[3] == 65530 && f[4] == 65535);
    EXPECT(ef_key(0, 1, 1, 5, 5) > ef_key(0, 0, 3, 65535, 65535));
    EXPECT(ef_key(0, 0, 2, 5, 5) > ef_key(0, 0, 1, 65535, 65535));
    EXPECT(ef_key(0, 0, 1, 6, 0) > ef_key(0, 0, 1, 5, 65535));
    EXPECT(ef_key(1, 0, 1, 5, 5) > ef_key(0, 12, 3, 65535, 65535));
}

int main() {
    octaves();
    taps();
    chunks();
    keys();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
