// Stand-alone check of the host part of csrc/hyp_batch.hpp (built and run by
// tests/test_hyp_batch_host.py, host only, under ASan + UBSan; no device call
// is made).  The block table lives in a std::vector of exactly 3 n_live + 1
// words here, so a write past it is the sanitizer's to report.
//
//   hyp_batch_host    the checks; exit status 0 and "ok" when they hold
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hyp_batch.hpp"

// what libsfmcore's sfm_api.hip defines for the headers; the last message is kept
static char last_error[256];
namespace sfm {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
void set_timings(const double *, int) {}
bool call_timing() { return false; }
}  // namespace sfm

using namespace sfm;

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                               \
        }                                                             \
    } while (0)

static std::vector<int64_t> csr(const std::vector<int64_t> &n) {
    std::vector<int64_t> s(n.size() + 1, 0);
    for (size_t r = 0; r < n.size(); ++r) s[r + 1] = s[r] + n[r];
    return s;
}

// the rule the five entry points each wrote out: HT below TILE, HT / 2 from TILE, HT / 4 from 4 TILE
static int64_t ref_ht(int64_t n, int64_t HT, int64_t TILE) { return n >= 4 * TILE ? HT / 4 : n >= TILE ? HT / 2 : HT; }

static void tile_table(const std::vector<int64_t> &n, int64_t min_n, int64_t H, int HT) {
    const int TILE = 1024;
    const std::vector<int64_t> start = csr(n);
    const int64_t rows = (int64_t)n.size();
    int64_t n_live = 0;
    for (int64_t v : n) n_live += v >= min_n;
    EXPECT(count_live(start.data(), rows, min_n) == n_live);
    std::vector<int32_t> words(3 * n_live + 1, -7);
    TileTable tt;
    EXPECT(tt.fill(words.data(), n_live, start.data(), rows, min_n, H, HT, TILE) == 0);
    EXPECT(tt.n_live == n_live && tt.words() == words.size() && tt.blk == words.data());
    const int32_t *blk = words.data(), *tab = blk + (n_live + 1);
    int64_t blocks = 0, j = 0;
    for (int64_t r = 0; r < rows; ++r) {
        if (n[r] < min_n) continue;
        const int64_t ht = ref_ht(n[r], HT, TILE);
        EXPECT(blk[j] == blocks && tab[2 * j] == r && tab[2 * j + 1] == ht);
        blocks += (H + ht - 1) / ht;
        ++j;
    }
    EXPECT(j == n_live && blk[n_live] == blocks && tt.blocks == blocks);
}

static void tile_tables() {
    const int64_t mins[4] = {8, 5, 6, 4};
    const int hts[4] = {64, 32, 16, 8};
    const int64_t Hs[5] = {1, 63, 64, 65, 70};
    for (int64_t m : mins)
        for (int HT : hts)
            for (int64_t H : Hs) {
                tile_table({m - 1, m, 1023, 1024, 4095, 4096}, m, H, HT);
                tile_table({1023, m - 1, 4096, m - 1, m - 1, 1024, m, m - 1}, m, H, HT);  // dead rows between live ones
                tile_table({m - 1, 0, m - 1}, m, H, HT);  // all dead: one word, 0 blocks
                tile_table({}, m, H, HT);
            }
    // one block too many for a launch: 2^20 hypotheses in tiles of 8 are 2^17 blocks a row, 2^14 rows make 2^31
    const int64_t R = 1 << 14, H = (int64_t)1 << 20;
    const std::vector<int64_t> start = csr(std::vector<int64_t>(R, 4096));
    std::vector<int32_t> words(3 * R + 1);
    TileTable tt;
    EXPECT(tt.fill(words.data(), R, start.data(), R, 4, H, 32, 1024) == SFM_ERR_ARG);
    EXPECT(std::strstr(last_error, "too many hypothesis tiles for one launch"));
    EXPECT(tt.fill(words.data(), R - 1, start.data(), R - 1, 4, H, 32, 1024) == 0);
    EXPECT(tt.blocks == ((int64_t)1 << 31) - ((int64_t)1 << 17));
}

static void live_runs() {
    const int64_t m = 6;
    const std::vector<std::vector<int64_t>> cases = {
        {}, {5}, {6}, {5, 5}, {6, 7, 8}, {5, 6, 7, 5, 5, 9, 5}, {6, 5, 6}, {0, 0, 6, 6}, {6, 6, 0, 0}};
    for (const auto &n : cases) {
        const std::vector<int64_t> start = csr(n);
        const int64_t rows = (int64_t)n.size();
        std::vector<int> seen(n.size(), 0);
        int64_t last_end = -1;
        const int rc = for_each_live_run(start.data(), rows, m, [&](int64_t r0, int64_t r1, int64_t k0, int64_t k1) {
            EXPECT(0 <= r0 && r0 < r1 && r1 <= rows && r0 > last_end);  // not empty, in order, apart from the last
            EXPECT(r0 == 0 || n[r0 - 1] < m);                            // maximal to the left ...
            EXPECT(r1 == rows || n[r1] < m);                             // ... and to the right
            EXPECT(k0 == start[r0] && k1 == start[r1]);
            for (int64_t r = r0; r < r1; ++r) ++seen[r];
            last_end = r1;
            return 0;
        });
        EXPECT(rc == 0);
        for (int64_t r = 0; r < rows; ++r) EXPECT(seen[r] == (n[r] >= m ? 1 : 0));
        // a failing copy ends the loop with its status
        int calls = 0;
        const int rc2 = for_each_live_run(start.data(), rows, m, [&](int64_t, int64_t, int64_t, int64_t) {
            ++calls;
            return SFM_ERR_HIP;
        });
        EXPECT(calls <= 1 && rc2 == (calls ? SFM_ERR_HIP : 0));
    }
}

static void samples() {
    const int64_t H = 3, m = 4;
    const int k = 3;
    const std::vector<int64_t> n = {5, 3, 4};  // the middle row is dead
    const std::vector<int64_t> start = csr(n);
    const std::vector<int32_t> good = {0, 1, 2, 4, 3, 0, 2, 4, 1, /* dead */ 9, 9, -1, 0, 0, 0, 7, 7, 7,
                                       3, 2, 1, 0, 1, 3, 1, 2, 0};
    const char *msg = "sample outside [0, n_v)";
    EXPECT(check_samples(start.data(), 3, good.data(), H, k, m, msg) == 0);
    std::vector<int32_t> t = good;
    t[2 * 9 + 4] = 4;  // row 2 has four items
    last_error[0] = 0;
    EXPECT(check_samples(start.data(), 3, t.data(), H, k, m, msg) == SFM_ERR_ARG);
    EXPECT(!std::strcmp(last_error, "argument: sample outside [0, n_v)"));
    t = good;
    t[0] = -1;
    EXPECT(check_samples(start.data(), 3, t.data(), H, k, m, msg) == SFM_ERR_ARG);
    EXPECT(!std::strcmp(last_error, "argument: sample outside [0, n_v)"));
    t = good;
    t[5] = 4;  // hypothesis 1 of row 0: (4, 3, 4)
    EXPECT(check_samples(start.data(), 3, t.data(), H, k, m, "sample outside [0, n_p)") == SFM_ERR_ARG);
    EXPECT(!std::strcmp(last_error, "argument: a hypothesis repeats a sample"));
    // the dead row's entries are never read as samples: with its minimum lowered they are
    EXPECT(check_samples(start.data(), 3, good.data(), H, k, 3, msg) == SFM_ERR_ARG);
    // no hypotheses and no table (init_pairs without homographies)
    EXPECT(check_samples(start.data(), 3, nullptr, 0, 4, m, msg) == 0);
}

static void inverse() {
    const double K[9] = {531.122155322710, 0.0, 407.192550839899, 0.0, 531.541737503901, 313.308715048366,
                         0.0, 0.0, 1.0};
    double Ki[9];
    const double det = inv3_adjugate(K, Ki);
    EXPECT(std::fabs(det - K[0] * K[4]) <= 1e-15 * K[0] * K[4]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double a = 0.0, b = 0.0, ma = 0.0, mb = 0.0;
            for (int j = 0; j < 3; ++j) {
                a += Ki[3 * r + j] * K[3 * j + c];
                b += K[3 * r + j] * Ki[3 * j + c];
                ma += std::fabs(Ki[3 * r + j] * K[3 * j + c]);
                mb += std::fabs(K[3 * r + j] * Ki[3 * j + c]);
            }
            // an entry of Ki is a product, det a product and the quotient: three roundings; the product and
            // the sum here two more.  Eight unit roundoffs of the terms' magnitudes bound them.
            EXPECT(std::fabs(a - (r == c)) <= 4 * DBL_EPSILON * ma && std::fabs(b - (r == c)) <= 4 * DBL_EPSILON * mb);
        }
    const double S[9] = {1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 0.0, 1.0};
    EXPECT(inv3_adjugate(S, Ki) == 0.0 && !std::isfinite(Ki[0]));
}

int main() {
    tile_tables();
    live_runs();
    samples();
    inverse();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
