// The calibrated minimal pose solver of batched view registration
// (register_p3p.hip): every camera pose (R, C), det R = +1, under which three
// world points X_i fall on three unit bearings b_i at positive depth,
// R (X_i - C) = d_i b_i with d_i > 0.  Up to four.  The reference has no
// counterpart.  Plain C++ apart from P3P_FN: one thread solves one sample in
// registers; nothing is indexed by a run-time value, and the solutions leave
// through a functor, so nothing goes to scratch.
//
// Method: the pencil of conics of the three distance constraints (the route
// of Persson and Nordberg's Lambda Twist, ECCV 2018, restated from the
// equations; none of its code).  With a_ij = |X_i - X_j|^2 / extent^2 and
// c_ij = b_i . b_j the depths satisfy
//     d_i^2 + d_j^2 - 2 c_ij d_i d_j = a_ij,            d^T M_ij d = a_ij.
//   p3_pencil    D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 are
//                homogeneous: d^T D1 d = d^T D2 d = 0.  det(D1 + g D2) is a
//                cubic in g (the pair is swapped where that makes the leading
//                coefficient the larger one).
//   p3_cubic     one real root by Newton's method from a bound it approaches
//                monotonically, the other two from the quadratic that is left
//                (real where its discriminant is >= 0), each polished by two
//                Newton steps on the cubic.  No trigonometric call: the device
//                library's argument reduction would bring scratch with it.
//   p3_split     D0 = D1 + g D2 has the eigenvalues s1, s2, 0; it is a pair of
//                real planes where s1 s2 < 0, and of the real roots the one
//                with the smallest s1 s2 / |D0|_F^2 is taken (with four real
//                solutions every root gives real planes; with two, only the
//                one real root does; with none the planes are real and the
//                quadratics below have no real root).  The planes are
//                (sqrt(s1) e1 +- sqrt(-s2) e2) . d = 0 with e_k the null vector
//                of D0 - s_k I, the largest cross product of two of its rows.
//   p3_plane     d = alpha p + beta q spans a plane; d^T E d = 0 for the other
//                member E of the pencil is a homogeneous quadratic in (alpha,
//                beta).  A root counts as real where the discriminant B^2 - A C
//                is >= 0 in fp64.  The scale comes from the sum of the three
//                constraints, the sign from d > 0.
//   p3_polish    P3P_GN Gauss-Newton steps on the three constraints in d.  A
//                solution is kept where d is finite and positive and every
//                constraint holds to P3P_RES (of the normalised a_ij <= 1)
//                afterwards: a root that is real by rounding alone does not
//                converge and is dropped here.
//   p3_pose      both triangles get an orthonormal frame (first edge, normal,
//                their cross product); R maps one to the other, so it is
//                orthogonal with det +1 to rounding; C = mean X - R^T mean Y.
// A sample has no solution where two points lie within P3P_COINCIDE of the
// sample's extent of each other or the triangle's area is below P3P_COLLINEAR
// extent^2.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define P3P_FN __host__ __device__ __forceinline__
#else
#define P3P_FN inline
#endif

#pragma clang fp contract(off)

namespace sfm {

constexpr int P3P_MAX_SOL = 4;
constexpr int P3P_GN = 5;
constexpr int P3P_CUBIC_ITERS = 100;
constexpr double P3P_RES = 1e-10;
constexpr double P3P_COINCIDE = 1e-12;
constexpr double P3P_COLLINEAR = 1e-10;

P3P_FN double p3_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

P3P_FN void p3_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// symmetric 3 x 3 as (00, 01, 02, 11, 12, 22)
P3P_FN double p3_quad(const double (&S)[6], const double (&x)[3], const double (&y)[3]) {
    const double s0 = (S[0] * y[0] + S[1] * y[1]) + S[2] * y[2];
    const double s1 = (S[1] * y[0] + S[3] * y[1]) + S[4] * y[2];
    const double s2 = (S[2] * y[0] + S[4] * y[1]) + S[5] * y[2];
    return (x[0] * s0 + x[1] * s1) + x[2] * s2;
}

P3P_FN double p3_det(const double (&S)[6]) {
    return (S[0] * (S[3] * S[5] - S[4] * S[4]) - S[1] * (S[1] * S[5] - S[4] * S[2])) +
           S[2] * (S[1] * S[4] - S[3] * S[2]);
}

// tr(adj(A) B) for symmetric A, B: the derivative of det(A + g B) at g = 0
P3P_FN double p3_mixed(const double (&A)[6], const double (&B)[6]) {
    const double c00 = A[3] * A[5] - A[4] * A[4], c11 = A[0] * A[5] - A[2] * A[2], c22 = A[0] * A[3] - A[1] * A[1];
    const double c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3], c12 = A[1] * A[2] - A[0] * A[4];
    return ((c00 * B[0] + c11 * B[3]) + c22 * B[5]) + 2.0 * ((c01 * B[1] + c02 * B[2]) + c12 * B[4]);
}

// real roots of x^3 + a x^2 + b x + c; returns 1 or 3
P3P_FN int p3_cubic(double a, double b, double c, double (&x)[3]) {
    // With t = x - xi about the inflection xi = -a / 3 the cubic is t^3 - 3 q t +
    // fi.  Its outermost root on the side where fi has the other sign lies
    // within 2 sqrt(q) + cbrt(|fi|) of xi, and from that bound Newton's method
    // moves towards it monotonically (the cubic and its second derivative have
    // one sign there), so the loop ends when the step no longer changes t.
    const double xi = -a / 3.0, q = (a * a - 3.0 * b) / 9.0;
    const double fi = ((xi + a) * xi + b) * xi + c;
    double t = -copysign(2.0 * sqrt(fmax(q, 0.0)) + cbrt(fabs(fi)), fi);
    if (fi == 0.0) t = 0.0;
    for (int it = 0; it < P3P_CUBIC_ITERS; ++it) {
        const double f = (t * t - 3.0 * q) * t + fi, df = 3.0 * (t * t - q);
        const double tn = t - f / df;
        if (!(df != 0.0) || !std::isfinite(tn) || tn == t) break;
        t = tn;
    }
    x[0] = xi + t;
    // the other two from the quadratic that is left: x^2 + (a + r) x + (b + r (a + r))
    const double pb = a + x[0], pc = b + x[0] * pb;
    const double disc = pb * pb - 4.0 * pc;
    int n = 1;
    x[1] = x[2] = x[0];
    if (disc >= 0.0) {
        const double s = -0.5 * (pb + copysign(sqrt(disc), pb));
        x[1] = s;
        x[2] = s != 0.0 ? pc / s : 0.0;
        n = 3;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const double f = ((x[k] + a) * x[k] + b) * x[k] + c, df = (3.0 * x[k] + 2.0 * a) * x[k] + b;
            const double st = f / df;
            if (df != 0.0 && std::isfinite(st)) x[k] -= st;
        }
    return n;
}

// unit null vector of the symmetric rank-two matrix S: the largest cross
// product of two of its rows
P3P_FN void p3_null(const double (&S)[6], double (&e)[3]) {
    const double r0[3] = {S[0], S[1], S[2]}, r1[3] = {S[1], S[3], S[4]}, r2[3] = {S[2], S[4], S[5]};
    double c01[3], c02[3], c12[3];
    p3_cross(r0, r1, c01);
    p3_cross(r0, r2, c02);
    p3_cross(r1, r2, c12);
    const double n01 = p3_dot(c01, c01), n02 = p3_dot(c02, c02), n12 = p3_dot(c12, c12);
    const bool u01 = n01 >= n02 && n01 >= n12, u02 = !u01 && n02 >= n12;
    const double nn = sqrt(u01 ? n01 : (u02 ? n02 : n12));
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = (u01 ? c01[k] : (u02 ? c02[k] : c12[k])) / nn;
}

struct P3Tri {
    double c12, c13, c23, a12, a13, a23;
};

P3P_FN void p3_residual(const P3Tri &t, const double (&d)[3], double (&f)[3]) {
    f[0] = ((d[0] * d[0] + d[1] * d[1]) - 2.0 * t.c12 * (d[0] * d[1])) - t.a12;
    f[1] = ((d[0] * d[0] + d[2] * d[2]) - 2.0 * t.c13 * (d[0] * d[2])) - t.a13;
    f[2] = ((d[1] * d[1] + d[2] * d[2]) - 2.0 * t.c23 * (d[1] * d[2])) - t.a23;
}

// Gauss-Newton on the three constraints (Cramer's rule on the 3 x 3 Jacobian);
// true where d ends finite, positive and on all three to P3P_RES
P3P_FN bool p3_polish(const P3Tri &t, double (&d)[3]) {
#pragma unroll
    for (int it = 0; it < P3P_GN; ++it) {
        double f[3];
        p3_residual(t, d, f);
        // J = [[j00, j01, 0], [j10, 0, j12], [0, j21, j22]]
        const double j00 = 2.0 * (d[0] - t.c12 * d[1]), j01 = 2.0 * (d[1] - t.c12 * d[0]);
        const double j10 = 2.0 * (d[0] - t.c13 * d[2]), j12 = 2.0 * (d[2] - t.c13 * d[0]);
        const double j21 = 2.0 * (d[1] - t.c23 * d[2]), j22 = 2.0 * (d[2] - t.c23 * d[1]);
        const double det = -(j00 * (j12 * j21)) - j01 * (j10 * j22);
        const double s0 = (f[0] * (-(j12 * j21)) - j01 * (f[1] * j22 - j12 * f[2])) / det;
        const double s1 = (j00 * (f[1] * j22 - j12 * f[2]) - f[0] * (j10 * j22)) / det;
        const double s2 = ((f[0] * (j10 * j21) - j00 * (f[1] * j21)) - j01 * (j10 * f[2])) / det;
        if (!(std::isfinite(s0) && std::isfinite(s1) && std::isfinite(s2))) break;
        d[0] -= s0;
        d[1] -= s1;
        d[2] -= s2;
    }
    double f[3];
    p3_residual(t, d, f);
    const double worst = fmax(fabs(f[0]), fmax(fabs(f[1]), fabs(f[2])));
    return std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && d[0] > 0.0 && d[1] > 0.0 &&
           d[2] > 0.0 && worst <= P3P_RES;
}

// (R, C) from the depths: Y_i = ext d_i b_i = R (X_i - C)
P3P_FN bool p3_pose(const double (&X)[3][3], const double (&b)[3][3], const double (&d)[3], double ext,
                    double (&R)[9], double (&C)[3]) {
    double Y[3][3], u1[3], u2[3], v1[3], v2[3], ux[3][3], vy[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Y[i][k] = (ext * d[i]) * b[i][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u1[k] = X[1][k] - X[0][k];
        u2[k] = X[2][k] - X[0][k];
        v1[k] = Y[1][k] - Y[0][k];
        v2[k] = Y[2][k] - Y[0][k];
    }
    p3_cross(u1, u2, ux[2]);
    p3_cross(v1, v2, vy[2]);
    const double nu1 = sqrt(p3_dot(u1, u1)), nu3 = sqrt(p3_dot(ux[2], ux[2]));
    const double nv1 = sqrt(p3_dot(v1, v1)), nv3 = sqrt(p3_dot(vy[2], vy[2]));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ux[0][k] = u1[k] / nu1;
        ux[2][k] /= nu3;
        vy[0][k] = v1[k] / nv1;
        vy[2][k] /= nv3;
    }
    p3_cross(ux[2], ux[0], ux[1]);
    p3_cross(vy[2], vy[0], vy[1]);
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R[3 * r + c] = (vy[0][r] * ux[0][c] + vy[1][r] * ux[1][c]) + vy[2][r] * ux[2][c];
            fin = fin && std::isfinite(R[3 * r + c]);
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double my[3] = {((Y[0][0] + Y[1][0]) + Y[2][0]) / 3.0, ((Y[0][1] + Y[1][1]) + Y[2][1]) / 3.0,
                              ((Y[0][2] + Y[1][2]) + Y[2][2]) / 3.0};
        const double mx = ((X[0][k] + X[1][k]) + X[2][k]) / 3.0;
        C[k] = mx - ((R[k] * my[0] + R[3 + k] * my[1]) + R[6 + k] * my[2]);
        fin = fin && std::isfinite(C[k]);
    }
    return fin;
}

// One plane w . d = 0 against the conic E: up to two solutions, each polished,
// turned into a pose and handed to emit(k, R, C) with k counted up in n.
template <class Emit>
P3P_FN void p3_plane(const P3Tri &t, const double (&X)[3][3], const double (&b)[3][3], double ext,
                     const double (&w)[3], const double (&E)[6], int &n, Emit &&emit) {
    const double a0 = fabs(w[0]), a1 = fabs(w[1]), a2 = fabs(w[2]);
    const bool j0 = a0 >= a1 && a0 >= a2, j1 = !j0 && a1 >= a2;
    // two vectors across w, built on its largest component
    const double p[3] = {j0 ? -w[1] : (j1 ? w[1] : w[2]), j0 ? w[0] : (j1 ? -w[0] : 0.0), j0 ? 0.0 : (j1 ? 0.0 : -w[0])};
    const double q[3] = {j0 ? -w[2] : 0.0, j0 ? 0.0 : (j1 ? -w[2] : w[2]), j0 ? w[0] : (j1 ? w[1] : -w[1])};
    const double A = p3_quad(E, p, p), B = p3_quad(E, p, q), Cq = p3_quad(E, q, q);
    const double disc = B * B - A * Cq;
    if (!(disc >= 0.0)) return;
    const double tt = -(B + copysign(sqrt(disc), B));
    // the roots (alpha : beta) = (tt : A) and (Cq : tt)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double al = k == 0 ? tt : Cq, be = k == 0 ? A : tt;
        double d[3] = {al * p[0] + be * q[0], al * p[1] + be * q[1], al * p[2] + be * q[2]};
        const double e12 = (d[0] * d[0] + d[1] * d[1]) - 2.0 * t.c12 * (d[0] * d[1]);
        const double e13 = (d[0] * d[0] + d[2] * d[2]) - 2.0 * t.c13 * (d[0] * d[2]);
        const double e23 = (d[1] * d[1] + d[2] * d[2]) - 2.0 * t.c23 * (d[1] * d[2]);
        double s = sqrt(((t.a12 + t.a13) + t.a23) / ((e12 + e13) + e23));
        if (d[0] < 0.0) s = -s;
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] *= s;
        if (!(d[0] > 0.0 && d[1] > 0.0 && d[2] > 0.0)) continue;  // false for a NaN
        if (!p3_polish(t, d)) continue;
        double R[9], C[3];
        if (!p3_pose(X, b, d, ext, R, C)) continue;
        emit(n, R, C);
        ++n;
    }
}

// X[i]: the three world points; b[i]: their unit bearings.  Calls emit(k, R, C)
// for solution k = 0, 1, ... and returns their number, at most P3P_MAX_SOL.
template <class Emit>
P3P_FN int p3p_solve(const double (&X)[3][3], const double (&b)[3][3], Emit &&emit) {
    double u12[3], u13[3], u23[3], nrm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u12[k] = X[1][k] - X[0][k];
        u13[k] = X[2][k] - X[0][k];
        u23[k] = X[2][k] - X[1][k];
    }
    const double l12 = p3_dot(u12, u12), l13 = p3_dot(u13, u13), l23 = p3_dot(u23, u23);
    const double ext2 = fmax(l12, fmax(l13, l23));
    p3_cross(u12, u13, nrm);
    if (!(ext2 > 0.0) || !std::isfinite(ext2)) return 0;
    if (fmin(l12, fmin(l13, l23)) <= (P3P_COINCIDE * P3P_COINCIDE) * ext2) return 0;
    if (!(sqrt(p3_dot(nrm, nrm)) > P3P_COLLINEAR * ext2)) return 0;
    const double ext = sqrt(ext2);
    const P3Tri t{p3_dot(b[0], b[1]), p3_dot(b[0], b[2]), p3_dot(b[1], b[2]), l12 / ext2, l13 / ext2, l23 / ext2};

    double D1[6] = {t.a23, -t.a23 * t.c12, 0.0, t.a23 - t.a12, t.a12 * t.c23, -t.a12};
    double D2[6] = {t.a23, 0.0, -t.a23 * t.c13, -t.a13, t.a13 * t.c23, t.a23 - t.a13};
    double k0 = p3_det(D1), k3 = p3_det(D2);
    if (fabs(k3) < fabs(k0)) {  // the larger determinant leads the cubic
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double s = D1[k];
            D1[k] = D2[k];
            D2[k] = s;
        }
        const double s = k0;
        k0 = k3;
        k3 = s;
    }
    const double k1 = p3_mixed(D1, D2), k2 = p3_mixed(D2, D1);
    if (!(fabs(k3) > 0.0)) return 0;
    double g[3];
    const int ng = p3_cubic(k2 / k3, k1 / k3, k0 / k3, g);

    // the root whose degenerate conic is most clearly a pair of real planes
    double best = 0.0, gam = 0.0, tr = 0.0, mm = 0.0;
    double D0[6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double S[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) S[k] = D1[k] + g[r] * D2[k];
        const double m = ((S[0] * S[3] - S[1] * S[1]) + (S[0] * S[5] - S[2] * S[2])) + (S[3] * S[5] - S[4] * S[4]);
        const double fr = ((S[0] * S[0] + S[3] * S[3]) + S[5] * S[5]) + 2.0 * ((S[1] * S[1] + S[2] * S[2]) + S[4] * S[4]);
        const double ratio = m / fr;
        if (r < ng && ratio < best) {
            best = ratio;
            gam = g[r];
            tr = (S[0] + S[3]) + S[5];
            mm = m;
#pragma unroll
            for (int k = 0; k < 6; ++k) D0[k] = S[k];
        }
    }
    if (!(best < 0.0)) return 0;
    const double sd = sqrt(tr * tr - 4.0 * mm);
    double s1, s2;  // s1 > 0 > s2, s1 s2 = mm
    if (tr >= 0.0) {
        s1 = 0.5 * (tr + sd);
        s2 = mm / s1;
    } else {
        s2 = 0.5 * (tr - sd);
        s1 = mm / s2;
    }
    double e1[3], e2[3];
    {
        const double S1[6] = {D0[0] - s1, D0[1], D0[2], D0[3] - s1, D0[4], D0[5] - s1};
        const double S2[6] = {D0[0] - s2, D0[1], D0[2], D0[3] - s2, D0[4], D0[5] - s2};
        p3_null(S1, e1);
        p3_null(S2, e2);
    }
    const double r1 = sqrt(s1), r2 = sqrt(-s2);
    // on a plane D1 = -gam D2: the member of the pencil that is not nearly D0
    const bool useD2 = fabs(gam) <= 1.0;
    double E[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) E[k] = useD2 ? D2[k] : D1[k];
    int n = 0;
#pragma unroll
    for (int sgn = 0; sgn < 2; ++sgn) {
        const double w[3] = {r1 * e1[0] + (sgn ? -r2 : r2) * e2[0], r1 * e1[1] + (sgn ? -r2 : r2) * e2[1],
                             r1 * e1[2] + (sgn ? -r2 : r2) * e2[2]};
        p3_plane(t, X, b, ext, w, E, n, emit);
    }
    return n;
}

}  // namespace sfm
