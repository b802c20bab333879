// Host-side arithmetic of feature extraction (extract_features.hip): the
// octaves' sizes and places in an image's pyramid, the blur taps, the bound on
// an image's candidates and the number of images a chunk holds.  No HIP call
// and no device code: tests/extract_plan_check.cpp compiles it alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define EF_HD __host__ __device__
#else
#define EF_HD
#endif

namespace sfm {

constexpr int EF_S = 3;                 // layers per octave
constexpr int EF_LAYERS = EF_S + 3;     // Gaussian images per octave
constexpr int EF_BORDER = 5;
constexpr int EF_MAX_R = 25;            // largest blur radius the tile kernel's LDS holds
constexpr int EF_MAX_OCTAVES = 16;
constexpr int EF_MAX_SIDE = 1 << 16;    // rows and columns fit 17 bits of a candidate key
constexpr int EF_MIN_SIDE = 16;
constexpr int64_t EF_WS_BYTES = (int64_t)1 << 30;   // pyramid + candidate keys of a chunk
constexpr int64_t EF_MAX_CHUNK = 256;               // images of a chunk (8 bits of a selection key)
constexpr int64_t EF_MAX_CAND = (int64_t)1 << 22;   // candidates of a chunk
constexpr int64_t EF_MAX_KP = (int64_t)1 << 22;     // keypoints of a chunk

struct EfTaps {
    int R;
    float w[2 * EF_MAX_R + 1];
};

// octaves that keep the smaller side >= 16, each taking every second pixel of the one before
inline int ef_max_octaves(int64_t H, int64_t W) {
    int n = 0;
    while ((H < W ? H : W) >= EF_MIN_SIDE && n < EF_MAX_OCTAVES) {
        ++n;
        H = (H + 1) / 2;
        W = (W + 1) / 2;
    }
    return n;
}

// sigma_inc of layer l of an octave (l == 0: the first octave's blur of the input, assumed to carry 0.5)
inline double ef_sigma_inc(double sigma, int l) {
    if (l == 0) return std::sqrt(sigma * sigma - 0.25);
    const double a = sigma * std::pow(2.0, l / (double)EF_S), b = sigma * std::pow(2.0, (l - 1) / (double)EF_S);
    return std::sqrt(a * a - b * b);
}

inline int ef_radius(double s) { return (int)std::ceil(4.0 * s); }

// 2 R + 1 weights in fp64, normalised to sum 1, then rounded to fp32; false when R > EF_MAX_R
inline bool ef_taps(double s, EfTaps &t) {
    const int R = ef_radius(s);
    if (R < 1 || R > EF_MAX_R) return false;
    double g[2 * EF_MAX_R + 1], sum = 0.0;
    for (int i = -R; i <= R; ++i) sum += g[i + R] = std::exp(-((double)i * (double)i) / (2.0 * s * s));
    t.R = R;
    for (int k = 0; k <= 2 * R; ++k) t.w[k] = (float)(g[k] / sum);
    for (int k = 2 * R + 1; k <= 2 * EF_MAX_R; ++k) t.w[k] = 0.0f;
    return true;
}

// the largest radius a call with this sigma needs (layer S + 2)
inline int ef_max_radius(double sigma) {
    const int a = ef_radius(ef_sigma_inc(sigma, 0)), b = ef_radius(ef_sigma_inc(sigma, EF_LAYERS - 1));
    return a > b ? a : b;
}

// An image's pyramid: octave o is h[o] x w[o], its EF_LAYERS layers start at
// float off[o] of the image's block of `per_image` floats.
struct EfLayout {
    int n_octaves = 0;
    int32_t h[EF_MAX_OCTAVES] = {}, w[EF_MAX_OCTAVES] = {};
    int64_t off[EF_MAX_OCTAVES] = {};
    int64_t per_image = 0;
    int64_t cand_bound = 0;  // no image has more candidates: see ef_layout
};

// Of the four pixels of a 2 x 2 block every two are neighbours, so a block
// holds at most one strict maximum and one strict minimum per DoG layer:
// at most 2 ceil(h / 2) ceil(w / 2) candidates per layer, EF_S layers per octave.
inline EfLayout ef_layout(int64_t H, int64_t W, int n_octaves) {
    EfLayout L;
    L.n_octaves = n_octaves;
    for (int o = 0; o < n_octaves; ++o) {
        L.h[o] = (int32_t)H;
        L.w[o] = (int32_t)W;
        L.off[o] = L.per_image;
        L.per_image += (int64_t)EF_LAYERS * H * W;
        L.cand_bound += (int64_t)EF_S * 2 * ((H + 1) / 2) * ((W + 1) / 2);
        H = (H + 1) / 2;
        W = (W + 1) / 2;
    }
    return L;
}

// candidates a chunk of n images has room for
inline int64_t ef_cand_capacity(const EfLayout &L, int64_t n) {
    const int64_t b = L.cand_bound * n;
    return b < EF_MAX_CAND ? b : EF_MAX_CAND;
}

// bytes of a chunk of n images that grow with n: the images, the pyramids and the candidate keys with their sorted copy
inline int64_t ef_chunk_bytes(const EfLayout &L, int64_t H, int64_t W, int64_t n) {
    return n * (H * W + L.per_image * (int64_t)sizeof(float)) + 2 * (int64_t)sizeof(uint64_t) * ef_cand_capacity(L, n);
}

// the most images, between 1 and EF_MAX_CHUNK, whose chunk stays inside EF_WS_BYTES (one image is always taken)
inline int64_t ef_chunk_images(const EfLayout &L, int64_t H, int64_t W, int64_t n_images) {
    int64_t n = n_images < EF_MAX_CHUNK ? n_images : EF_MAX_CHUNK;
    while (n > 1 && ef_chunk_bytes(L, H, W, n) > EF_WS_BYTES) --n;
    return n < 1 ? 1 : n;
}

// the 64-bit sort key of a candidate: (image in chunk, octave, layer, row, column)
EF_HD inline uint64_t ef_key(uint32_t img, uint32_t oct, uint32_t layer, uint32_t row, uint32_t col) {
    return ((uint64_t)img << 40) | ((uint64_t)oct << 36) | ((uint64_t)layer << 34) | ((uint64_t)row << 17) | col;
}
inline void ef_unkey(uint64_t k, int32_t out[5]) {
    out[0] = (int32_t)(k >> 40);
    out[1] = (int32_t)((k >> 36) & 15);
    out[2] = (int32_t)((k >> 34) & 3);
    out[3] = (int32_t)((k >> 17) & 0x1ffff);
    out[4] = (int32_t)(k & 0x1ffff);
}

}  // namespace sfm
