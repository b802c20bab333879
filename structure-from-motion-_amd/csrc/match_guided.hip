// Guided descriptor matching: sfm_match_descriptors with the candidates of a
// keypoint restricted to the keypoints of the other image inside a band
// around its epipolar line (include/sfmcore.h).  The pair's F comes from pair
// verification; the gate is vp_inlier of epi_sampson.hpp, bit for bit.
//
// The kernels and the host driver are match_descriptors.hip's
// (match_common.hpp); this file is the gate that k_md_nn is instantiated with.
// vp_inlier splits into what depends on the first image's keypoint alone,
// l = F (x, y, 1) and l0^2 + l1^2, and what depends on the second's alone,
// (u, v) and m0^2 + m1^2 with m = F^T (u, v, 1).  Per element
// e = (u l0 + v l1) + l2, den = (l0^2 + l1^2) + (m0^2 + m1^2) and
// den > 0 && e e < thr2 den are vp_inlier's operations in its order, fp64
// without contraction.  In the swapped pass (nn_rev) the rows are the second
// image's keypoints and carry (u, v, m0^2 + m1^2), the columns the first's and
// carry (l0, l1, l2, l0^2 + l1^2): the same operands in the same roles, so a
// pair of keypoints is a candidate in both passes or in neither.  NaN terms
// (a row or a column past the image's end) fail the gate.  The forward pass
// counts the elements inside per row (n_cand).
//
// Integer minima, a scan and a gate without a reduction: every output is the
// same from run to run.
#include "match_common.hpp"

namespace sfm {

struct MdEpiGate {
    static constexpr bool gated = true;
    // The terms of a row take 8 VGPRs: the kernel is built for two workgroups per CU, and at dim 256 two
    // subtiles per wave do not fit beside the A fragments at that.
    static constexpr int min_blocks = 2;
    static constexpr int ms(int dim) { return dim == 256 ? 1 : MD_MS; }
    static constexpr int row_terms(bool swap) { return swap ? 3 : 4; }
    static constexpr int col_terms(bool swap) { return swap ? 4 : 3; }

    // What vp_inlier computes from the first image's keypoint alone: t = (l0, l1, l2, l0^2 + l1^2) with
    // l = F (x, y, 1).
    static __device__ __forceinline__ void first(const double (&F)[9], double x, double y, double (&t)[4]) {
#pragma clang fp contract(off)
        t[0] = (F[0] * x + F[1] * y) + F[2];
        t[1] = (F[3] * x + F[4] * y) + F[5];
        t[2] = (F[6] * x + F[7] * y) + F[8];
        t[3] = t[0] * t[0] + t[1] * t[1];
    }
    // ... and from the second's alone: t = (u, v, m0^2 + m1^2) with m = F^T (u, v, 1).
    static __device__ __forceinline__ void second(const double (&F)[9], double u, double v, double (&t)[4]) {
#pragma clang fp contract(off)
        const double m0 = (F[0] * u + F[3] * v) + F[6];
        const double m1 = (F[1] * u + F[4] * v) + F[7];
        t[0] = u;
        t[1] = v;
        t[2] = m0 * m0 + m1 * m1;
        t[3] = 0.0;
    }
    // vp_inlier's decision from the two sides' terms
    static __device__ __forceinline__ bool inside(const double *first, const double *second, double thr2) {
#pragma clang fp contract(off)
        const double e = (second[0] * first[0] + second[1] * first[1]) + first[2];
        const double den = first[3] + second[2];
        const double e2 = e * e;
        return den > 0.0 && e2 < thr2 * den;
    }

    // the kernel's rows are the first image's keypoints, its columns the second's; SWAP: the other way round
    template <bool SWAP>
    static __device__ __forceinline__ void row(const double (&F)[9], double2 q, double (&t)[4]) {
        if (SWAP) second(F, q.x, q.y, t);
        else first(F, q.x, q.y, t);
    }
    template <bool SWAP>
    static __device__ __forceinline__ void col(const double (&F)[9], double2 q, double (&t)[4]) {
        row<!SWAP>(F, q, t);
    }
    template <bool SWAP>
    static __device__ __forceinline__ bool in(const double *row, const double *col, double thr2) {
        return SWAP ? inside(col, row, thr2) : inside(row, col, thr2);
    }
};

}  // namespace sfm

using namespace sfm;

extern "C" int sfm_match_descriptors_guided(const uint8_t *desc, const double *xy, int64_t n_kp,
                                            const int64_t *img_start, int32_t n_images, int32_t dim,
                                            const int32_t *pairs, const double *F, int64_t P, double gate, double ratio,
                                            int32_t max_dsq, int32_t cross_check, int64_t capacity,
                                            int64_t *match_start, int32_t *match_a, int32_t *match_b,
                                            int32_t *match_dsq, int32_t *nn, int32_t *d1, int32_t *d2, int32_t *nn_rev,
                                            int32_t *n_cand, int device) {
    return md_run<MdEpiGate>(desc, n_kp, img_start, n_images, dim, pairs, P, ratio, max_dsq, cross_check, capacity,
                             match_start, match_a, match_b, match_dsq, nn, d1, d2, nn_rev, {xy, F, gate, n_cand},
                             device);
}
