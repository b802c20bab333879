// Feature extraction: images to keypoints and 128-byte gradient-histogram
// descriptors, on the device -- the stage in front of sfm_match_descriptors.
// A difference-of-Gaussians detector after Lowe, with the definitions of
// include/sfmcore.h.  The reference has no extractor.
//
// The images of a call are processed in chunks whose pyramids fit a fixed
// workspace (extract_plan.hpp); per chunk:
//
//   k_ef_blur     one Gaussian layer from the one before: a workgroup owns a
//                 32 x 64 tile, loads it with a halo of R on every side into
//                 LDS (reflect-101 at the borders, the uint8 -> fp32 conversion
//                 for the first layer), runs the row pass into a second LDS tile
//                 and the column pass from there: a layer is read once and
//                 written once.  The taps are kernel arguments.
//   k_ef_down     the first layer of an octave: every second pixel of layer S.
//   k_ef_detect   a workgroup owns 8 x 32 pixels of an octave: the five DoG
//                 images of the tile with a halo of 1 are formed in LDS from the
//                 six Gaussian layers, each thread tests its pixel in DoG layers
//                 1..S against the threshold and its 26 neighbours, and appends
//                 a 64-bit key (image, octave, layer, row, column).
//   rocPRIM       a radix sort of the keys: the candidates' order.
//   k_ef_refine   a thread per candidate: the quadratic fit, the moves and the
//                 contrast and edge tests.
//   k_ef_orient   16 lanes per candidate: each lane sums its share of the
//                 window into a histogram of its own in LDS, the 16 are added in
//                 lane order, smoothed twice, and the peaks counted (first
//                 launch) or written as keypoints (second launch, behind a scan
//                 of the counts).  No floating-point atomics.
//   selection     with max_keypoints: a stable radix sort by (image, response
//                 descending) ranks the keypoints of an image; a scan of the
//                 kept flags gives the output places, in key order.
//   k_ef_describe a wave per kept keypoint: the 4 x 4 x 8 histogram in LDS as
//                 64-bit fixed point (2^-36), so that the atomic adds commute
//                 and the sum does not depend on their order; normalise, clamp,
//                 normalise, pack, in the same kernel, which also writes the
//                 keypoint's other outputs to their final place.
//
// Integer atomics, sorts, scans and fixed summation orders only: every output
// is the same from run to run.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "extract_plan.hpp"
#include "staging.hpp"

namespace sfm {

constexpr int EF_THREADS = 256;
constexpr int EF_TH = 32, EF_TW = 64;    // blur tile
constexpr int EF_DH = 8, EF_DW = 32;     // detect tile
constexpr int EF_NBINS = 36;
constexpr int EF_GROUP = 16;             // lanes per candidate in k_ef_orient
constexpr float EF_TWO_PI = 6.283185307179586f;

__device__ __forceinline__ int ef_reflect(int i, int n) {
    const int p = 2 * (n - 1);
    int m = (i < 0 ? -i : i) % p;
    return m >= n ? p - m : m;
}

// dst (H x W) = the blur of src, read as src[(r * step) * srcW + c * step]
template <bool U8>
__global__ __launch_bounds__(EF_THREADS) void k_ef_blur(const void *__restrict__ src_, int64_t src_stride, int srcW,
                                                        float *__restrict__ dst_, int64_t dst_stride, int H, int W,
                                                        EfTaps t) {
    extern __shared__ __attribute__((aligned(16))) float ef_lds[];
    const int R = t.R, IW = EF_TW + 2 * R, IH = EF_TH + 2 * R;
    float *sIn = ef_lds, *sMid = ef_lds + IH * IW;
    const int r0 = blockIdx.y * EF_TH, c0 = blockIdx.x * EF_TW, tid = threadIdx.x;
    float *dst = dst_ + (int64_t)blockIdx.z * dst_stride;
    for (int idx = tid; idx < IH * IW; idx += EF_THREADS) {
        const int rr = idx / IW, cc = idx - rr * IW;
        const int64_t at = (int64_t)ef_reflect(r0 + rr - R, H) * srcW + ef_reflect(c0 + cc - R, W);
        float v;
        if (U8)
            v = (float)(static_cast<const uint8_t *>(src_) + (int64_t)blockIdx.z * src_stride)[at] / 255.0f;
        else
            v = (static_cast<const float *>(src_) + (int64_t)blockIdx.z * src_stride)[at];
        sIn[idx] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < IH * EF_TW; idx += EF_THREADS) {
        const int rr = idx / EF_TW, cc = idx % EF_TW;
        const float *p = sIn + rr * IW + cc;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * R; ++k) acc = fmaf(t.w[k], p[k], acc);
        sMid[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < EF_TH * EF_TW; idx += EF_THREADS) {
        const int rr = idx / EF_TW, cc = idx % EF_TW;
        const float *p = sMid + rr * EF_TW + cc;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * R; ++k) acc = fmaf(t.w[k], p[k * EF_TW], acc);
        if (r0 + rr < H && c0 + cc < W) dst[(int64_t)(r0 + rr) * W + c0 + cc] = acc;
    }
}

// dst (H x W) = every second pixel of src (srcW columns); one image per blockIdx.z
static __global__ __launch_bounds__(EF_THREADS) void k_ef_down(const float *__restrict__ src, int64_t stride, int srcW,
                                                               float *__restrict__ dst, int H, int W) {
    const int64_t i = (int64_t)blockIdx.x * EF_THREADS + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
    dst[(int64_t)blockIdx.z * stride + i] = src[(int64_t)blockIdx.z * stride + (int64_t)(2 * r) * srcW + 2 * c];
}

// layers: the octave's EF_LAYERS Gaussian images of image blockIdx.z, H x W each
static __global__ __launch_bounds__(EF_THREADS) void k_ef_detect(const float *__restrict__ pyr, int64_t stride, int H,
                                                                 int W, int oct, float thr, uint64_t *__restrict__ keys,
                                                                 unsigned long long *__restrict__ count, int64_t cap) {
    constexpr int LH = EF_DH + 2, LW = EF_DW + 2;
    __shared__ float sD[EF_LAYERS - 1][LH][LW];
    const float *g = pyr + (int64_t)blockIdx.z * stride;
    const int r0 = blockIdx.y * EF_DH, c0 = blockIdx.x * EF_DW, tid = threadIdx.x;
    const int64_t plane = (int64_t)H * W;
    for (int idx = tid; idx < LH * LW; idx += EF_THREADS) {
        const int rr = idx / LW, cc = idx % LW;
        const int r = r0 + rr - 1, c = c0 + cc - 1;
        const bool in = r >= 0 && r < H && c >= 0 && c < W;
        const int64_t at = in ? (int64_t)r * W + c : 0;
        float prev = in ? g[at] : 0.0f;
#pragma unroll
        for (int l = 0; l < EF_LAYERS - 1; ++l) {
            const float next = in ? g[(l + 1) * plane + at] : 0.0f;
            sD[l][rr][cc] = next - prev;
            prev = next;
        }
    }
    __syncthreads();
    const int rr = tid / EF_DW + 1, cc = tid % EF_DW + 1;
    const int r = r0 + rr - 1, c = c0 + cc - 1;
    if (r < EF_BORDER || r >= H - EF_BORDER || c < EF_BORDER || c >= W - EF_BORDER) return;
#pragma unroll
    for (int l = 1; l <= EF_S; ++l) {
        const float v = sD[l][rr][cc];
        if (!(fabsf(v) > thr)) continue;
        bool gt = true, lt = true;
#pragma unroll
        for (int dl = -1; dl <= 1; ++dl)
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    if (dl == 0 && dr == 0 && dc == 0) continue;
                    const float n = sD[l + dl][rr + dr][cc + dc];
                    gt = gt && v > n;
                    lt = lt && v < n;
                }
        if (gt || lt) {
            const unsigned long long slot = atomicAdd(count, 1ull);
            if ((int64_t)slot < cap) keys[slot] = ef_key(blockIdx.z, oct, l, r, c);
        }
    }
}

struct EfGeom {  // the pyramid of one image as the kernels address it
    int32_t h[EF_MAX_OCTAVES], w[EF_MAX_OCTAVES];
    int64_t off[EF_MAX_OCTAVES];
    int64_t per_image;
};

__device__ __forceinline__ void ef_split(uint64_t k, int &img, int &oct, int &l, int &r, int &c) {
    img = (int)(k >> 40);
    oct = (int)((k >> 36) & 15);
    l = (int)((k >> 34) & 3);
    r = (int)((k >> 17) & 0x1ffff);
    c = (int)(k & 0x1ffff);
}

// ref_ok[k], ref_site[3 k] = final (layer, row, col), ref_val[4 k] = (xc, xr, xs, |D^|) of candidate k
static __global__ __launch_bounds__(EF_THREADS) void k_ef_refine(const float *__restrict__ pyr, EfGeom G,
                                                                 const uint64_t *__restrict__ keys, int64_t n,
                                                                 float ct, float er, uint8_t *__restrict__ ref_ok,
                                                                 int32_t *__restrict__ ref_site,
                                                                 float *__restrict__ ref_val) {
    const int64_t k = (int64_t)blockIdx.x * EF_THREADS + threadIdx.x;
    if (k >= n) return;
    int img, oct, l, r, c;
    ef_split(keys[k], img, oct, l, r, c);
    const int H = G.h[oct], W = G.w[oct];
    const int64_t plane = (int64_t)H * W;
    const float *g = pyr + (int64_t)img * G.per_image + G.off[oct];
    auto D = [&](int ll, int rr, int cc) {
        const int64_t at = (int64_t)rr * W + cc;
        return g[(ll + 1) * plane + at] - g[ll * plane + at];
    };
    bool done = false;
    float xc = 0, xr = 0, xs = 0, v = 0, gx = 0, gy = 0, gs = 0, dxx = 0, dyy = 0, dxy = 0;
    for (int move = 0; move <= 5; ++move) {
        v = D(l, r, c);
        const float xm = D(l, r, c - 1), xp = D(l, r, c + 1), ym = D(l, r - 1, c), yp = D(l, r + 1, c);
        const float sm = D(l - 1, r, c), sp = D(l + 1, r, c);
        gx = (xp - xm) * 0.5f;
        gy = (yp - ym) * 0.5f;
        gs = (sp - sm) * 0.5f;
        const float v2 = v * 2.0f;
        dxx = xp + xm - v2;
        dyy = yp + ym - v2;
        const float dss = sp + sm - v2;
        dxy = (D(l, r + 1, c + 1) - D(l, r + 1, c - 1) - D(l, r - 1, c + 1) + D(l, r - 1, c - 1)) * 0.25f;
        const float dxs = (D(l + 1, r, c + 1) - D(l + 1, r, c - 1) - D(l - 1, r, c + 1) + D(l - 1, r, c - 1)) * 0.25f;
        const float dys = (D(l + 1, r + 1, c) - D(l + 1, r - 1, c) - D(l - 1, r + 1, c) + D(l - 1, r - 1, c)) * 0.25f;
        const float c00 = dyy * dss - dys * dys, c01 = dxs * dys - dxy * dss, c02 = dxy * dys - dxs * dyy;
        const float c11 = dxx * dss - dxs * dxs, c12 = dxy * dxs - dxx * dys, c22 = dxx * dyy - dxy * dxy;
        const float det = dxx * c00 + dxy * c01 + dxs * c02;
        if (!isfinite(det) || det == 0.0f) break;
        const float inv = -1.0f / det;
        xc = (c00 * gx + c01 * gy + c02 * gs) * inv;
        xr = (c01 * gx + c11 * gy + c12 * gs) * inv;
        xs = (c02 * gx + c12 * gy + c22 * gs) * inv;
        if (!(fabsf(xc) < 1000.0f && fabsf(xr) < 1000.0f && fabsf(xs) < 1000.0f)) break;
        if (fabsf(xc) <= 0.5f && fabsf(xr) <= 0.5f && fabsf(xs) <= 0.5f) {
            done = true;
            break;
        }
        if (move == 5) break;
        c += (int)floorf(xc + 0.5f);
        r += (int)floorf(xr + 0.5f);
        l += (int)floorf(xs + 0.5f);
        if (l < 1 || l > EF_S || c < EF_BORDER || c >= W - EF_BORDER || r < EF_BORDER || r >= H - EF_BORDER) break;
    }
    bool ok = done;
    float resp = 0.0f;
    if (ok) {
        resp = fabsf(v + 0.5f * (gx * xc + gy * xr + gs * xs));
        ok = !(resp * (float)EF_S < ct);
    }
    if (ok) {
        const float tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy;
        ok = det2 > 0.0f && tr * tr * er < (er + 1.0f) * (er + 1.0f) * det2;
    }
    ref_ok[k] = ok ? 1 : 0;
    ref_site[3 * k] = ok ? l : 0;
    ref_site[3 * k + 1] = ok ? r : 0;
    ref_site[3 * k + 2] = ok ? c : 0;
    ref_val[4 * k] = ok ? xc : 0.0f;
    ref_val[4 * k + 1] = ok ? xr : 0.0f;
    ref_val[4 * k + 2] = ok ? xs : 0.0f;
    ref_val[4 * k + 3] = ok ? resp : 0.0f;
}

// The orientations of candidate k (16 lanes each).  WRITE == false: n_ori[k].
// WRITE == true: the keypoints at place[k] + 0, 1, .. in ascending bin.
template <bool WRITE>
__global__ __launch_bounds__(EF_THREADS) void k_ef_orient(const float *__restrict__ pyr, EfGeom G,
                                                          const uint64_t *__restrict__ keys, int64_t n, float sigma,
                                                          const uint8_t *__restrict__ ref_ok,
                                                          const int32_t *__restrict__ ref_site,
                                                          const float *__restrict__ ref_val, int32_t *__restrict__ n_ori,
                                                          const int64_t *__restrict__ place, double *__restrict__ kp_xy,
                                                          float *__restrict__ kp_val, int32_t *__restrict__ kp_site) {
    __shared__ float sPart[EF_NBINS][EF_THREADS];
    __shared__ float sA[EF_THREADS / EF_GROUP][EF_NBINS], sB[EF_THREADS / EF_GROUP][EF_NBINS];
    const int tid = threadIdx.x, grp = tid / EF_GROUP, ln = tid % EF_GROUP;
    const int64_t k = (int64_t)blockIdx.x * (EF_THREADS / EF_GROUP) + grp;
    const bool live = k < n && ref_ok[k];
    int img = 0, oct = 0, l = 1, r = 0, c = 0, rad = -1, H = 0, W = 0;
    float xs = 0.0f, s_oct = 1.0f;
    const float *g = pyr;
    if (live) {
        int l0, r0, c0;
        ef_split(keys[k], img, oct, l0, r0, c0);
        l = ref_site[3 * k];
        r = ref_site[3 * k + 1];
        c = ref_site[3 * k + 2];
        xs = ref_val[4 * k + 2];
        H = G.h[oct];
        W = G.w[oct];
        g = pyr + (int64_t)img * G.per_image + G.off[oct] + (int64_t)l * H * W;
        s_oct = sigma * exp2f(((float)l + xs) / (float)EF_S);
        rad = (int)floorf(4.5f * s_oct + 0.5f);
    }
#pragma unroll
    for (int b = 0; b < EF_NBINS; ++b) sPart[b][tid] = 0.0f;
    const float sw = 1.5f * s_oct, den = 2.0f * sw * sw;
    const int side = 2 * rad + 1, total = rad >= 0 ? side * side : 0;
    for (int s = ln; s < total; s += EF_GROUP) {
        const int i = s / side - rad, j = s % side - rad;
        const int y = r + i, x = c + j;
        if (y <= 0 || y >= H - 1 || x <= 0 || x >= W - 1) continue;
        const float dx = g[(int64_t)y * W + x + 1] - g[(int64_t)y * W + x - 1];
        const float dy = g[(int64_t)(y + 1) * W + x] - g[(int64_t)(y - 1) * W + x];
        const float mag = sqrtf(dx * dx + dy * dy);
        float ang = atan2f(dy, dx);
        if (ang < 0.0f) ang += EF_TWO_PI;
        const float wgt = expf(-((float)(i * i + j * j)) / den);
        int b = (int)floorf(ang * ((float)EF_NBINS / EF_TWO_PI) + 0.5f);
        b = b >= EF_NBINS ? b - EF_NBINS : b;
        sPart[b][tid] += wgt * mag;
    }
    __syncthreads();
    for (int b = ln; b < EF_NBINS; b += EF_GROUP) {
        float sum = 0.0f;
#pragma unroll
        for (int q = 0; q < EF_GROUP; ++q) sum += sPart[b][grp * EF_GROUP + q];
        sA[grp][b] = sum;
    }
    __syncthreads();
    auto smooth = [&](const float *h, float *o) {
        for (int b = ln; b < EF_NBINS; b += EF_GROUP) {
            const float m2 = h[(b + EF_NBINS - 2) % EF_NBINS], p2 = h[(b + 2) % EF_NBINS];
            const float m1 = h[(b + EF_NBINS - 1) % EF_NBINS], p1 = h[(b + 1) % EF_NBINS];
            o[b] = (m2 + p2) * (1.0f / 16.0f) + (m1 + p1) * (4.0f / 16.0f) + h[b] * (6.0f / 16.0f);
        }
    };
    smooth(sA[grp], sB[grp]);
    __syncthreads();
    smooth(sB[grp], sA[grp]);
    __syncthreads();
    if (!live || ln != 0) return;
    const float *h = sA[grp];
    float top = 0.0f;
    for (int b = 0; b < EF_NBINS; ++b) top = fmaxf(top, h[b]);
    int cnt = 0;
    for (int b = 0; b < EF_NBINS; ++b) {
        const float lo = h[(b + EF_NBINS - 1) % EF_NBINS], hi = h[(b + 1) % EF_NBINS], hb = h[b];
        if (!(top > 0.0f && hb > lo && hb > hi && hb >= 0.8f * top)) continue;
        if (WRITE) {
            float bi = (float)b + 0.5f * (lo - hi) / (lo - 2.0f * hb + hi);
            bi = bi < 0.0f ? bi + (float)EF_NBINS : (bi >= (float)EF_NBINS ? bi - (float)EF_NBINS : bi);
            const int64_t o = place[k] + cnt;
            const double step = (double)(1 << oct);
            kp_xy[2 * o] = ((double)c + (double)ref_val[4 * k]) * step;
            kp_xy[2 * o + 1] = ((double)r + (double)ref_val[4 * k + 1]) * step;
            kp_val[3 * o] = sigma * (float)(1 << oct) * exp2f(((float)l + xs) / (float)EF_S);
            kp_val[3 * o + 1] = bi * (EF_TWO_PI / (float)EF_NBINS);
            kp_val[3 * o + 2] = ref_val[4 * k + 3];
            kp_site[4 * o] = img;
            kp_site[4 * o + 1] = oct;
            kp_site[4 * o + 2] = l;
            kp_site[4 * o + 3] = (int32_t)k;
        }
        ++cnt;
    }
    if (!WRITE) n_ori[k] = cnt;
}

// selection keys: (image << 32) | ~bits(response), the value the keypoint's index
static __global__ __launch_bounds__(EF_THREADS) void k_ef_sel_keys(const float *__restrict__ kp_val,
                                                                   const int32_t *__restrict__ kp_site, int64_t n,
                                                                   uint64_t *__restrict__ key, int32_t *__restrict__ val,
                                                                   int32_t *__restrict__ img_count) {
    const int64_t i = (int64_t)blockIdx.x * EF_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t img = (uint32_t)kp_site[4 * i];
    key[i] = ((uint64_t)img << 32) | (uint32_t)~__float_as_uint(kp_val[3 * i + 2]);
    val[i] = (int32_t)i;
    atomicAdd(&img_count[img], 1);
}

// keep[val[p]] = rank of position p inside its image < max_kp
static __global__ __launch_bounds__(EF_THREADS) void k_ef_sel_rank(const uint64_t *__restrict__ key,
                                                                   const int32_t *__restrict__ val, int64_t n,
                                                                   const int64_t *__restrict__ img_first, int32_t max_kp,
                                                                   int32_t *__restrict__ keep) {
    const int64_t p = (int64_t)blockIdx.x * EF_THREADS + threadIdx.x;
    if (p >= n) return;
    keep[val[p]] = p - img_first[key[p] >> 32] < max_kp ? 1 : 0;
}

// sel[place[i]] = i for every kept keypoint, and the kept count of its image
static __global__ __launch_bounds__(EF_THREADS) void k_ef_sel_write(const int32_t *__restrict__ keep,
                                                                    const int64_t *__restrict__ place,
                                                                    const int32_t *__restrict__ kp_site, int64_t n,
                                                                    int32_t *__restrict__ sel,
                                                                    int32_t *__restrict__ out_count) {
    const int64_t i = (int64_t)blockIdx.x * EF_THREADS + threadIdx.x;
    if (i >= n || !keep[i]) return;
    sel[place[i]] = (int32_t)i;
    atomicAdd(&out_count[kp_site[4 * i]], 1);
}

// Output row f = keypoint sel[f] (f itself without a selection), f < *n_out
// (n without one): the descriptor, and the keypoint's other outputs.
static __global__ __launch_bounds__(EF_THREADS) void k_ef_describe(
    const float *__restrict__ pyr, EfGeom G, const double *__restrict__ kp_xy, const float *__restrict__ kp_val,
    const int32_t *__restrict__ kp_site, const int32_t *__restrict__ ref_site, const int32_t *__restrict__ sel,
    const int64_t *__restrict__ n_out, int64_t n, double *__restrict__ o_xy, float *__restrict__ o_scale,
    float *__restrict__ o_angle, float *__restrict__ o_resp, uint8_t *__restrict__ o_desc,
    int32_t *__restrict__ o_site) {
    __shared__ unsigned long long sH[EF_THREADS / 64][128];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t f = (int64_t)blockIdx.x * (EF_THREADS / 64) + wave;
    const bool live = f < (n_out ? *n_out : n);
    sH[wave][lane] = 0;
    sH[wave][lane + 64] = 0;
    int64_t i = 0;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1, W = 0;
    float xo = 0, yo = 0, hw = 1, ca = 1, sa = 0, angle = 0;
    const float *g = pyr;
    if (live) {
        i = sel ? sel[f] : f;
        const int img = kp_site[4 * i], oct = kp_site[4 * i + 1], l = kp_site[4 * i + 2];
        const int H = G.h[oct];
        W = G.w[oct];
        g = pyr + (int64_t)img * G.per_image + G.off[oct] + (int64_t)l * H * W;
        const double inv = 1.0 / (double)(1 << oct);
        xo = (float)(kp_xy[2 * i] * inv);
        yo = (float)(kp_xy[2 * i + 1] * inv);
        angle = kp_val[3 * i + 1];
        hw = 3.0f * (kp_val[3 * i] / (float)(1 << oct));
        const int rad = (int)floorf(hw * 3.5355339f + 0.5f) + 1;
        const int cx = (int)floorf(xo + 0.5f), cy = (int)floorf(yo + 0.5f);
        x0 = max(cx - rad, 1);
        x1 = min(cx + rad, W - 2);
        y0 = max(cy - rad, 1);
        y1 = min(cy + rad, H - 2);
        ca = cosf(angle);
        sa = sinf(angle);
    }
    __syncthreads();
    const int nx = x1 - x0 + 1, total = nx > 0 && y1 >= y0 ? nx * (y1 - y0 + 1) : 0;
    for (int s = lane; s < total; s += 64) {
        const int py = y0 + s / nx, px = x0 + s % nx;
        const float dx = (float)px - xo, dy = (float)py - yo;
        const float rx = (ca * dx + sa * dy) / hw, ry = (ca * dy - sa * dx) / hw;
        const float cb = rx + 1.5f, rb = ry + 1.5f;
        if (!(rb > -1.0f && rb < 4.0f && cb > -1.0f && cb < 4.0f)) continue;
        const float gx = g[(int64_t)py * W + px + 1] - g[(int64_t)py * W + px - 1];
        const float gy = g[(int64_t)(py + 1) * W + px] - g[(int64_t)(py - 1) * W + px];
        const float mag = sqrtf(gx * gx + gy * gy) * expf(-(rx * rx + ry * ry) * 0.125f);
        float ob = (atan2f(gy, gx) - angle) * (8.0f / EF_TWO_PI);
        ob -= 8.0f * floorf(ob * 0.125f);
        if (ob >= 8.0f) ob -= 8.0f;
        const float fr0 = floorf(rb), fc0 = floorf(cb), fo0 = floorf(ob);
        const float fr = rb - fr0, fc = cb - fc0, fo = ob - fo0;
        const int ri = (int)fr0, ci = (int)fc0, oi = (int)fo0;
#pragma unroll
        for (int dr = 0; dr < 2; ++dr) {
            const int rr = ri + dr;
            if (rr < 0 || rr >= 4) continue;
            const float wr = dr ? fr : 1.0f - fr;
#pragma unroll
            for (int dc = 0; dc < 2; ++dc) {
                const int cc = ci + dc;
                if (cc < 0 || cc >= 4) continue;
                const float wc = dc ? fc : 1.0f - fc;
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const float v = mag * wr * wc * (d ? fo : 1.0f - fo);
                    const unsigned long long q = (unsigned long long)((double)v * 68719476736.0 + 0.5);  // 2^36
                    atomicAdd(&sH[wave][(rr * 4 + cc) * 8 + ((oi + d) & 7)], q);
                }
            }
        }
    }
    __syncthreads();
    auto wave_sum = [](float v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        return v;
    };
    float a = (float)((double)sH[wave][lane] * (1.0 / 68719476736.0));
    float b = (float)((double)sH[wave][lane + 64] * (1.0 / 68719476736.0));
    float nrm = fmaxf(sqrtf(wave_sum(a * a + b * b)), 1e-12f);
    a = fminf(a / nrm, 0.2f);
    b = fminf(b / nrm, 0.2f);
    nrm = fmaxf(sqrtf(wave_sum(a * a + b * b)), 1e-12f);
    if (!live) return;
    o_desc[f * 128 + lane] = (uint8_t)fminf(255.0f, floorf(512.0f * (a / nrm) + 0.5f));
    o_desc[f * 128 + lane + 64] = (uint8_t)fminf(255.0f, floorf(512.0f * (b / nrm) + 0.5f));
    if (lane == 0) {
        o_xy[2 * f] = kp_xy[2 * i];
        o_xy[2 * f + 1] = kp_xy[2 * i + 1];
        o_scale[f] = kp_val[3 * i];
        o_angle[f] = kp_val[3 * i + 1];
        o_resp[f] = kp_val[3 * i + 2];
        const int64_t k = kp_site[4 * i + 3];
        o_site[4 * f] = kp_site[4 * i + 1];
        o_site[4 * f + 1] = kp_site[4 * i + 2];
        o_site[4 * f + 2] = ref_site[3 * k + 1];
        o_site[4 * f + 3] = ref_site[3 * k + 2];
    }
}

#define EF_LAUNCH(kernel, grid, lds, ...)                                        \
    do {                                                                         \
        hipLaunchKernelGGL(kernel, grid, dim3(EF_THREADS), lds, s, __VA_ARGS__); \
        SFM_HIP(hipGetLastError());                                              \
    } while (0)

static unsigned ef_blocks(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_extract_features(const uint8_t *images, int32_t n_images, int32_t H, int32_t W, int32_t n_octaves,
                                    int32_t max_keypoints, double contrast_threshold, double edge_threshold,
                                    double sigma, int64_t capacity, int64_t *kp_start, double *xy, float *scale,
                                    float *angle, float *response, uint8_t *desc, int32_t *kp_site, float *pyramid,
                                    int64_t cand_capacity, int64_t *cand_start, int32_t *cand, uint8_t *ref_ok,
                                    int32_t *ref_site, float *ref_val, int device) {
    SFM_CHECK_ARG(n_images >= 0 && capacity >= 0 && cand_capacity >= 0, "n_images, capacity or cand_capacity < 0");
    SFM_CHECK_ARG(H >= EF_MIN_SIDE && W >= EF_MIN_SIDE, "H or W below 16");
    SFM_CHECK_ARG(H <= EF_MAX_SIDE && W <= EF_MAX_SIDE, "H or W above 65536");
    SFM_CHECK_ARG(n_octaves >= 0 && n_octaves <= ef_max_octaves(H, W),
                  "n_octaves < 0 or above the octaves that keep the smaller side >= 16");
    SFM_CHECK_ARG(std::isfinite(contrast_threshold) && contrast_threshold > 0.0, "contrast_threshold not finite or <= 0");
    SFM_CHECK_ARG(std::isfinite(edge_threshold) && edge_threshold > 0.0, "edge_threshold not finite or <= 0");
    SFM_CHECK_ARG(std::isfinite(sigma) && sigma > 0.5, "sigma not finite or not above the input's blur 0.5");
    SFM_CHECK_ARG(ef_max_radius(sigma) <= EF_MAX_R, "sigma above 3.2: a blur radius above 25");
    SFM_CHECK_ARG(max_keypoints >= 0, "max_keypoints < 0");
    SFM_CHECK_ARG(capacity >= max_keypoints, "capacity below max_keypoints");
    SFM_CHECK_ARG(kp_start, "null pointer");
    SFM_CHECK_ARG(n_images == 0 || images, "null pointer");
    SFM_CHECK_ARG(n_images == 0 || capacity == 0 || (xy && scale && angle && response && desc), "null pointer");
    const bool want_cand = cand_start || cand || ref_ok || ref_site || ref_val;
    SFM_CHECK_ARG(!want_cand || (cand_start && (cand_capacity == 0 || (cand && ref_ok && ref_site && ref_val))),
                  "null pointer: the candidate diagnostics come together");
    kp_start[0] = 0;
    if (cand_start) cand_start[0] = 0;
    if (n_images == 0) return 0;

    if (n_octaves == 0) n_octaves = ef_max_octaves(H, W);
    const EfLayout L = ef_layout(H, W, n_octaves);
    EfGeom G;
    for (int o = 0; o < EF_MAX_OCTAVES; ++o) {
        G.h[o] = L.h[o];
        G.w[o] = L.w[o];
        G.off[o] = L.off[o];
    }
    G.per_image = L.per_image;
    EfTaps taps[EF_LAYERS];
    for (int l = 0; l < EF_LAYERS; ++l)
        SFM_CHECK_ARG(ef_taps(ef_sigma_inc(sigma, l), taps[l]), "sigma above 3.2: a blur radius above 25");
    const float thr = (float)(0.5 * contrast_threshold / EF_S), ct = (float)contrast_threshold;
    const float er = (float)edge_threshold, sg = (float)sigma;
    const int64_t px = (int64_t)H * W;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    const bool timed = call_timing();
    double t_ms[4] = {0.0, 0.0, 0.0, 0.0};
    std::vector<uint64_t> h_keys;
    std::vector<int32_t> h_count;
    int64_t n_cand_total = 0;

    int64_t chunk = ef_chunk_images(L, H, W, n_images);
    for (int64_t i0 = 0; i0 < n_images;) {
        const int64_t cn = chunk < n_images - i0 ? chunk : n_images - i0;
        const int64_t cand_cap = ef_cand_capacity(L, cn);
        Pack work(c->buf[0]);
        const auto w_img = work.add<uint8_t>(cn * px);
        const auto w_pyr = work.add<float>(cn * L.per_image);
        const auto w_keys = work.add<uint64_t>(cand_cap), w_sorted = work.add<uint64_t>(cand_cap);
        const auto w_cnt = work.add<unsigned long long>(1);
        const auto w_icnt = work.add<int32_t>(2 * cn);
        const auto w_ifirst = work.add<int64_t>(cn + 1);
        SFM_TRY(work.reserve());
        float *d_pyr = work.ptr(w_pyr);
        if (timed) SFM_HIP(hipEventRecord(c->ev[0], s));
        SFM_TRY(work.upload(w_img, images + i0 * px, s));
        if (timed) SFM_HIP(hipEventRecord(c->ev[1], s));

        // the pyramid
        for (int o = 0; o < n_octaves; ++o) {
            const int h = L.h[o], w = L.w[o];
            const dim3 grid(ef_blocks(w, EF_TW), ef_blocks(h, EF_TH), (unsigned)cn);
            for (int l = 0; l < EF_LAYERS; ++l) {
                float *dst = d_pyr + L.off[o] + (int64_t)l * h * w;
                const int R = taps[l].R;
                const size_t lds = sizeof(float) * (size_t)((EF_TH + 2 * R) * (EF_TW + 2 * R) + (EF_TH + 2 * R) * EF_TW);
                if (l == 0 && o == 0) {
                    EF_LAUNCH(k_ef_blur<true>, grid, lds, (const void *)work.ptr(w_img), px, w, dst, L.per_image, h, w,
                              taps[0]);
                } else if (l == 0) {
                    const float *src = d_pyr + L.off[o - 1] + (int64_t)EF_S * L.h[o - 1] * L.w[o - 1];
                    EF_LAUNCH(k_ef_down, dim3(ef_blocks((int64_t)h * w, EF_THREADS), 1, (unsigned)cn), 0, src,
                              L.per_image, L.w[o - 1], dst, h, w);
                } else {
                    EF_LAUNCH(k_ef_blur<false>, grid, lds, (const void *)(dst - (int64_t)h * w), L.per_image, w, dst,
                              L.per_image, h, w, taps[l]);
                }
            }
        }
        if (timed) SFM_HIP(hipEventRecord(c->ev[4], s));
        // the candidates
        SFM_HIP(hipMemsetAsync(work.ptr(w_cnt), 0, sizeof(unsigned long long), s));
        for (int o = 0; o < n_octaves; ++o) {
            const dim3 grid(ef_blocks(L.w[o], EF_DW), ef_blocks(L.h[o], EF_DH), (unsigned)cn);
            EF_LAUNCH(k_ef_detect, grid, 0, d_pyr + L.off[o], L.per_image, L.h[o], L.w[o], o, thr, work.ptr(w_keys),
                      work.ptr(w_cnt), cand_cap);
        }
        unsigned long long found = 0;
        SFM_HIP(hipMemcpyAsync(&found, work.ptr(w_cnt), sizeof(found), hipMemcpyDeviceToHost, s));
        SFM_HIP(hipStreamSynchronize(s));
        if ((int64_t)found > cand_cap) {
            if (cn == 1) {
                set_error("extract_features: an image with more than %lld candidates", (long long)cand_cap);
                return SFM_ERR_NOMEM;
            }
            chunk = cn / 2;  // the same images again, in smaller chunks
            continue;
        }
        const int64_t n_cand = (int64_t)found;
        if (want_cand && n_cand_total + n_cand > cand_capacity) {
            set_error("extract_features: cand_capacity %lld is below the candidates found by image %lld",
                      (long long)cand_capacity, (long long)(i0 + cn - 1));
            return SFM_ERR_CAPACITY;
        }
        int64_t n_kp = 0, n_final = 0;
        h_count.assign((size_t)cn, 0);

        Pack ref(c->buf[1]), kp(c->buf[2]), out(c->buf[3]), tmp(c->buf[4]);
        const auto r_ok = ref.add<uint8_t>(n_cand);
        const auto r_site = ref.add<int32_t>(3 * n_cand);
        const auto r_val = ref.add<float>(4 * n_cand);
        const auto r_nori = ref.add<int32_t>(n_cand + 1);
        const auto r_place = ref.add<int64_t>(n_cand + 1);
        uint64_t *d_keys = work.ptr(w_sorted);
        if (n_cand > 0) {
            size_t tb_sort = 0, tb_scan = 0;
            SFM_HIP(rocprim::radix_sort_keys(nullptr, tb_sort, work.ptr(w_keys), d_keys, (size_t)n_cand, 0, 64, s));
            SFM_HIP(rocprim::exclusive_scan(nullptr, tb_scan, (int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0,
                                            (size_t)n_cand + 1, rocprim::plus<int64_t>(), s));
            const auto t_a = tmp.add<char>(tb_sort > tb_scan ? tb_sort : tb_scan);
            SFM_TRY(tmp.reserve());
            SFM_TRY(ref.reserve());
            SFM_HIP(rocprim::radix_sort_keys(tmp.ptr(t_a), tb_sort, work.ptr(w_keys), d_keys, (size_t)n_cand, 0, 64, s));
            EF_LAUNCH(k_ef_refine, dim3(ef_blocks(n_cand, EF_THREADS)), 0, d_pyr, G, d_keys, n_cand, ct, er,
                      ref.ptr(r_ok), ref.ptr(r_site), ref.ptr(r_val));
            SFM_HIP(hipMemsetAsync(ref.ptr(r_nori), 0, sizeof(int32_t) * (size_t)(n_cand + 1), s));
            const dim3 g_ori(ef_blocks(n_cand, EF_THREADS / EF_GROUP));
            EF_LAUNCH(k_ef_orient<false>, g_ori, 0, d_pyr, G, d_keys, n_cand, sg, ref.ptr(r_ok), ref.ptr(r_site),
                      ref.ptr(r_val), ref.ptr(r_nori), (const int64_t *)nullptr, (double *)nullptr, (float *)nullptr,
                      (int32_t *)nullptr);
            SFM_HIP(rocprim::exclusive_scan(tmp.ptr(t_a), tb_scan, ref.ptr(r_nori), ref.ptr(r_place), (int64_t)0,
                                            (size_t)n_cand + 1, rocprim::plus<int64_t>(), s));
            SFM_HIP(hipMemcpyAsync(&n_kp, ref.ptr(r_place, (size_t)n_cand), sizeof(int64_t), hipMemcpyDeviceToHost, s));
            SFM_HIP(hipStreamSynchronize(s));
            if (n_kp > EF_MAX_KP) {
                if (cn == 1) {
                    set_error("extract_features: an image with more than %lld keypoints", (long long)EF_MAX_KP);
                    return SFM_ERR_NOMEM;
                }
                chunk = cn / 2;
                continue;
            }
        }
        const auto k_xy = kp.add<double>(2 * n_kp);
        const auto k_val = kp.add<float>(3 * n_kp);
        const auto k_site = kp.add<int32_t>(4 * n_kp);
        const auto k_key = kp.add<uint64_t>(n_kp), k_key2 = kp.add<uint64_t>(n_kp);
        const auto k_idx = kp.add<int32_t>(n_kp), k_idx2 = kp.add<int32_t>(n_kp);
        const auto k_keep = kp.add<int32_t>(n_kp + 1);
        const auto k_place = kp.add<int64_t>(n_kp + 1);
        const auto k_sel = kp.add<int32_t>(n_kp);
        const auto o_xy = out.add<double>(2 * n_kp);
        const auto o_scale = out.add<float>(n_kp), o_angle = out.add<float>(n_kp), o_resp = out.add<float>(n_kp);
        const auto o_desc = out.add<uint8_t>(128 * n_kp);
        const auto o_site = out.add<int32_t>(4 * n_kp);
        int32_t *d_icnt = work.ptr(w_icnt), *d_ocnt = work.ptr(w_icnt, (size_t)cn);
        if (n_kp > 0) {
            SFM_TRY(kp.reserve());
            SFM_TRY(out.reserve());
            const dim3 g_ori(ef_blocks(n_cand, EF_THREADS / EF_GROUP)), g_kp(ef_blocks(n_kp, EF_THREADS));
            EF_LAUNCH(k_ef_orient<true>, g_ori, 0, d_pyr, G, d_keys, n_cand, sg, ref.ptr(r_ok), ref.ptr(r_site),
                      ref.ptr(r_val), (int32_t *)nullptr, (const int64_t *)ref.ptr(r_place), kp.ptr(k_xy),
                      kp.ptr(k_val), kp.ptr(k_site));
            SFM_HIP(hipMemsetAsync(d_icnt, 0, sizeof(int32_t) * 2 * (size_t)cn, s));
            EF_LAUNCH(k_ef_sel_keys, g_kp, 0, kp.ptr(k_val), kp.ptr(k_site), n_kp, kp.ptr(k_key), kp.ptr(k_idx), d_icnt);
            const bool select = max_keypoints > 0;
            if (select) {
                size_t tb_sort = 0, tb_s1 = 0, tb_s2 = 0;
                SFM_HIP(rocprim::radix_sort_pairs(nullptr, tb_sort, kp.ptr(k_key), kp.ptr(k_key2), kp.ptr(k_idx),
                                                  kp.ptr(k_idx2), (size_t)n_kp, 0, 64, s));
                SFM_HIP(rocprim::exclusive_scan(nullptr, tb_s1, (int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0,
                                                (size_t)cn + 1, rocprim::plus<int64_t>(), s));
                SFM_HIP(rocprim::exclusive_scan(nullptr, tb_s2, (int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0,
                                                (size_t)n_kp + 1, rocprim::plus<int64_t>(), s));
                size_t tb = tb_sort > tb_s1 ? tb_sort : tb_s1;
                tb = tb > tb_s2 ? tb : tb_s2;
                Pack tmp2(c->buf[5]);
                const auto t_b = tmp2.add<char>(tb);
                SFM_TRY(tmp2.reserve());
                SFM_HIP(rocprim::radix_sort_pairs(tmp2.ptr(t_b), tb_sort, kp.ptr(k_key), kp.ptr(k_key2), kp.ptr(k_idx),
                                                  kp.ptr(k_idx2), (size_t)n_kp, 0, 64, s));
                // d_icnt has cn counts and then the cn zeroed output counts: the scan's extra entry reads a 0
                SFM_HIP(rocprim::exclusive_scan(tmp2.ptr(t_b), tb_s1, d_icnt, work.ptr(w_ifirst), (int64_t)0,
                                                (size_t)cn + 1, rocprim::plus<int64_t>(), s));
                SFM_HIP(hipMemsetAsync(kp.ptr(k_keep, (size_t)n_kp), 0, sizeof(int32_t), s));
                EF_LAUNCH(k_ef_sel_rank, g_kp, 0, kp.ptr(k_key2), kp.ptr(k_idx2), n_kp,
                          (const int64_t *)work.ptr(w_ifirst), max_keypoints, kp.ptr(k_keep));
                SFM_HIP(rocprim::exclusive_scan(tmp2.ptr(t_b), tb_s2, kp.ptr(k_keep), kp.ptr(k_place), (int64_t)0,
                                                (size_t)n_kp + 1, rocprim::plus<int64_t>(), s));
                EF_LAUNCH(k_ef_sel_write, g_kp, 0, kp.ptr(k_keep), kp.ptr(k_place), kp.ptr(k_site), n_kp, kp.ptr(k_sel),
                          d_ocnt);
            }
            EF_LAUNCH(k_ef_describe, dim3(ef_blocks(n_kp, EF_THREADS / 64)), 0, d_pyr, G, kp.ptr(k_xy), kp.ptr(k_val),
                      kp.ptr(k_site), ref.ptr(r_site), select ? (const int32_t *)kp.ptr(k_sel) : nullptr,
                      select ? (const int64_t *)kp.ptr(k_place, (size_t)n_kp) : nullptr, n_kp, out.ptr(o_xy),
                      out.ptr(o_scale), out.ptr(o_angle), out.ptr(o_resp), out.ptr(o_desc), out.ptr(o_site));
            SFM_HIP(hipMemcpyAsync(h_count.data(), select ? d_ocnt : d_icnt, sizeof(int32_t) * (size_t)cn,
                                   hipMemcpyDeviceToHost, s));
        }
        if (timed) SFM_HIP(hipEventRecord(c->ev[2], s));
        SFM_HIP(hipStreamSynchronize(s));

        // the chunk's rows of the outputs
        for (int64_t k = 0; k < cn; ++k) {
            if (h_count[k] > capacity) {
                set_error("extract_features: image %lld has %d keypoints, capacity is %lld per image",
                          (long long)(i0 + k), h_count[k], (long long)capacity);
                return SFM_ERR_CAPACITY;
            }
            kp_start[i0 + k + 1] = kp_start[i0 + k] + h_count[k];
            n_final += h_count[k];
        }
        const size_t at = (size_t)kp_start[i0], nf = (size_t)n_final;
        SFM_TRY(out.download(xy ? xy + 2 * at : nullptr, o_xy, 0, 2 * nf, s));
        SFM_TRY(out.download(scale ? scale + at : nullptr, o_scale, 0, nf, s));
        SFM_TRY(out.download(angle ? angle + at : nullptr, o_angle, 0, nf, s));
        SFM_TRY(out.download(response ? response + at : nullptr, o_resp, 0, nf, s));
        SFM_TRY(out.download(desc ? desc + 128 * at : nullptr, o_desc, 0, 128 * nf, s));
        SFM_TRY(out.download(kp_site ? kp_site + 4 * at : nullptr, o_site, 0, 4 * nf, s));
        SFM_TRY(work.download(pyramid ? pyramid + i0 * L.per_image : nullptr, w_pyr, s));
        if (want_cand && n_cand > 0) {
            h_keys.resize((size_t)n_cand);
            SFM_HIP(hipMemcpyAsync(h_keys.data(), d_keys, sizeof(uint64_t) * (size_t)n_cand, hipMemcpyDeviceToHost, s));
            SFM_TRY(ref.download(ref_ok + n_cand_total, r_ok, s));
            SFM_TRY(ref.download(ref_site + 3 * n_cand_total, r_site, s));
            SFM_TRY(ref.download(ref_val + 4 * n_cand_total, r_val, s));
        }
        if (timed) SFM_HIP(hipEventRecord(c->ev[3], s));
        SFM_HIP(hipStreamSynchronize(s));
        if (want_cand) {
            int64_t k = 0;
            for (int64_t im = 0; im < cn; ++im) {
                for (; k < n_cand && (int64_t)(h_keys[(size_t)k] >> 40) == im; ++k) {
                    int32_t *row = cand + 5 * (n_cand_total + k);
                    ef_unkey(h_keys[(size_t)k], row);
                    row[0] = (int32_t)(i0 + im);
                }
                cand_start[i0 + im + 1] = n_cand_total + k;
            }
            n_cand_total += n_cand;
        }
        for (int p = 0; timed && p < 3; ++p) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, c->ev[p], c->ev[p + 1]);
            t_ms[p] += ms;
        }
        if (timed) {
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[4]);
            t_ms[3] += ms;
        }
        i0 += cn;
    }
    set_timings(t_ms, 4);
    return 0;
}
