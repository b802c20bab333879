// The per-point bodies shared by k_triangulate (sfm_api.hip) and the
// two-view kernels (two_view.hip): one DLT triangulation, one cheirality bit.
#pragma once
#include "sfm_geom.hpp"

namespace sfm {

// LinearTriangulation.py:54-90 for one point: the 4x4 DLT system of the
// projections u (under P1) and v (under Q), the right singular vector of its
// smallest singular value by one-sided Jacobi, dehomogenised where |h3| > 1e-8.
// P1, Q: 3 x 4 row-major.
__device__ __forceinline__ void triangulate_point(const double *P1, const double *Q, const double2 u,
                                                  const double2 v, double (&X)[3]) {
    double a[4][4], V[4][4];  // a[col][row]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        a[c][0] = u.y * P1[8 + c] - P1[4 + c];
        a[c][1] = P1[c] - u.x * P1[8 + c];
        a[c][2] = v.y * Q[8 + c] - Q[4 + c];
        a[c][3] = Q[c] - v.x * Q[8 + c];
    }
    jacobi_onesided<4, 4, 40>(a, V);
    const int j = weakest_column<4, 4>(a);
    const double h0 = V[0][j], h1 = V[1][j], h2 = V[2][j], h3 = V[3][j];
    if (fabs(h3) > 1e-8) {
        X[0] = h0 / h3; X[1] = h1 / h3; X[2] = h2 / h3;
    } else {
        X[0] = h0; X[1] = h1; X[2] = h2;
    }
}

// DisambiguateCameraPose.py:58-70 for one point and one candidate: X lies in
// front of camera 1 (third row r1 of its rotation, centre c1) and of camera 2
// (r2, c2).  With r1 = (0, 0, 1), c1 = 0 the first depth is X[2] itself.
__device__ __forceinline__ bool in_front_of_both(const double *r1, const double *c1, const double *r2,
                                                 const double *c2, const double (&X)[3]) {
#pragma clang fp contract(off)
    const double z1 = r1[0] * (X[0] - c1[0]) + r1[1] * (X[1] - c1[1]) + r1[2] * (X[2] - c1[2]);
    const double z2 = r2[0] * (X[0] - c2[0]) + r2[1] * (X[1] - c2[1]) + r2[2] * (X[2] - c2[2]);
    return z1 > 0 && z2 > 0;
}

}  // namespace sfm
