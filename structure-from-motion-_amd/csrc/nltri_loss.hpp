// The two-view reprojection loss shared by k_nltri (nltri.hip) and the
// two-view tracks of k_triangulate_tracks (multiview.hip).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace sfm {

struct NlTriLoss {
    const double *P1, *P2;
    double u1, v1, u2, v2;
    // Loss (NonLinearTriangulation.py:5-50).  numpy's 3x4 @ 4 mat-vec sums
    // pairwise, (p0 x0 + p2 x2) + (p1 x1 + p3 * 1); a view whose depth is
    // below 1e-8 in magnitude falls back to the observation (residual 0).
    __device__ __forceinline__ void view(const double *P, const double (&X)[3], double u, double v, double &fu,
                                         double &fv) const {
        const double h0 = (P[0] * X[0] + P[2] * X[2]) + (P[1] * X[1] + P[3]);
        const double h1 = (P[4] * X[0] + P[6] * X[2]) + (P[5] * X[1] + P[7]);
        const double h2 = (P[8] * X[0] + P[10] * X[2]) + (P[9] * X[1] + P[11]);
        double px = u, py = v;
        if (!(fabs(h2) < 1e-8)) {
            px = h0 / h2;
            py = h1 / h2;
        }
        fu = u - px;
        fv = v - py;
    }
    __device__ __forceinline__ void operator()(const double (&X)[3], double (&f)[4]) const {
        view(P1, X, u1, v1, f[0], f[1]);
        view(P2, X, u2, v2, f[2], f[3]);
    }
};

}  // namespace sfm
