// The calibrated two-view model of batched pair verification
// (essential_pairs.hip): the 5-point essential matrix, x2^^T E x1^ = 0 for
// x^ = K^-1 [x; 1], and the five-parameter refit of E = [t]x R.  The reference
// has no counterpart; these functions stand beside epi_sampson.hpp, whose
// design row, unit-norm rule and inlier rule they use.
//
// One thread solves one hypothesis.  The 10 x 20 coefficient matrix of the ten
// cubic constraints (200 doubles) does not fit a thread's registers, so it
// lives with the null-space basis in a workspace of EP_WS doubles, reached as
// w.at(e) = p[e * S]: in LDS with S the number of hypotheses side by side, so
// that neighbouring lanes hit neighbouring banks.  Arrays that are indexed by
// a run-time value are kept there; everything in registers is indexed by
// unrolled loops only, so nothing goes to scratch.
//
//   ep_nullspace    Householder LQ of the 5 x 9 design: the last four columns
//                   of Q are an orthonormal basis X, Y, Z, W of its null space.
//   ep_constraints  E = x X + y Y + z Z + W; det E = 0 and 2 E E^T E - tr(E E^T)
//                   E = 0 expanded over the 20 monomials of degree <= 3.
//   ep_eliminate    Gauss-Jordan with partial pivoting on the ten cubic columns
//                   that hold x or y to a power of two or more.
//   ep_detpoly      rows x^2 z - z x^2, y^2 z - z y^2, x y z - z x y of the
//                   reduced system are B(z) [x, y, 1]^T = 0 with B of degrees
//                   (3, 3, 4) per row; det B is the degree-10 polynomial in z.
//   ep_roots        its ten complex roots by Aberth iteration (Gauss-Seidel
//                   order from fixed starting points, so deterministic), the
//                   real ones polished by Newton steps on the real axis.
//   ep_solve        all of it: up to ten E of unit norm (vp_unit's sign).
#pragma once
#include "epi_sampson.hpp"

#pragma clang fp contract(off)

namespace sfm {

constexpr int EP_WS = 296;      // basis 36 | quadratic forms 60 | constraint matrix 200
constexpr int EP_BASIS = 0, EP_LAM = 36, EP_A = 96;
constexpr int EP_MAX_SOL = 10;
constexpr int EP_ABERTH_ITERS = 64;
constexpr double EP_REAL_TOL = 1e-8;  // a root is real where |Im| <= EP_REAL_TOL max(1, |Re|)

struct EpK {
    double ki[9];  // K^-1, row-major
};

template <int S> struct EpWs {
    double *p;
    __device__ __forceinline__ double &at(int e) const { return p[e * S]; }
};

// x^ = K^-1 [x; 1], dehomogenised
__device__ __forceinline__ void ep_normalise(const EpK &K, double x, double y, double &a, double &b) {
    const double h0 = (K.ki[0] * x + K.ki[1] * y) + K.ki[2];
    const double h1 = (K.ki[3] * x + K.ki[4] * y) + K.ki[5];
    const double h2 = (K.ki[6] * x + K.ki[7] * y) + K.ki[8];
    a = h0 / h2;
    b = h1 / h2;
}

// F = K^-T E K^-1 brought to unit norm by vp_unit
__device__ __forceinline__ void ep_F(const EpK &K, const double (&E)[9], double (&F)[9]) {
    double tmp[9], G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            tmp[3 * i + c] = (E[3 * i] * K.ki[c] + E[3 * i + 1] * K.ki[3 + c]) + E[3 * i + 2] * K.ki[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            G[3 * r + c] = (K.ki[r] * tmp[c] + K.ki[3 + r] * tmp[3 + c]) + K.ki[6 + r] * tmp[6 + c];
    vp_unit(G, F);
}

// (a, b): the five normalised points of the first image, (c, d): of the second.
template <int S>
__device__ __forceinline__ void ep_nullspace(const double (&a)[5], const double (&b)[5], const double (&c)[5],
                                             const double (&d)[5], const EpWs<S> &w) {
    double A[5][9], tau[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) vp_row(a[i], b[i], c[i], d[i], A[i]);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double nrm2 = 0;
#pragma unroll
        for (int j = k; j < 9; ++j) nrm2 += A[k][j] * A[k][j];
        const double nrm = sqrt(nrm2);
        const double alpha = A[k][k] > 0 ? -nrm : nrm;
        A[k][k] -= alpha;
        double vtv = 0;
#pragma unroll
        for (int j = k; j < 9; ++j) vtv += A[k][j] * A[k][j];
        tau[k] = nrm2 > 0 ? 2.0 / vtv : 0.0;
#pragma unroll
        for (int i = k + 1; i < 5; ++i) {
            double dd = 0;
#pragma unroll
            for (int j = k; j < 9; ++j) dd += A[i][j] * A[k][j];
            dd *= tau[k];
#pragma unroll
            for (int j = k; j < 9; ++j) A[i][j] -= dd * A[k][j];
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double n[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) n[j] = j == 5 + m ? 1.0 : 0.0;
#pragma unroll
        for (int k = 4; k >= 0; --k) {
            double dd = 0;
#pragma unroll
            for (int j = k; j < 9; ++j) dd += A[k][j] * n[j];
            dd *= tau[k];
#pragma unroll
            for (int j = k; j < 9; ++j) n[j] -= dd * A[k][j];
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) w.at(EP_BASIS + 9 * m + j) = n[j];
    }
}

// Monomials.  Linear forms: [x, y, z, 1].  Quadratic: [x2, y2, z2, xy, xz, yz, x,
// y, z, 1].  Cubic, the columns of the constraint matrix: [x3, y3, x2y, xy2, x2z,
// x2, y2z, y2, xyz, xy | xz2, xz, x, yz2, yz, y, z3, z2, z, 1].
// ep_i2(a, b): the quadratic monomial of linear a times linear b; ep_i3(q, l):
// the cubic monomial of quadratic q times linear l.
__device__ __forceinline__ int ep_i2(int a, int b) {
    const unsigned char t[16] = {0, 3, 4, 6, 3, 1, 5, 7, 4, 5, 2, 8, 6, 7, 8, 9};
    return t[4 * a + b];
}
__device__ __forceinline__ int ep_i3(int q, int l) {
    const unsigned char t[40] = {0, 2,  4,  5,  3,  1, 6,  7,  10, 13, 16, 17, 2,  3,  8,  9,  4,  8,  10, 11,
                                 8, 6,  13, 14, 5,  9, 11, 12, 9,  7,  14, 15, 11, 14, 17, 18, 12, 15, 18, 19};
    return t[4 * q + l];
}

template <int S> __device__ __forceinline__ void ep_constraints(const EpWs<S> &w) {
    for (int e = 0; e < 200; ++e) w.at(EP_A + e) = 0.0;
    // row 9: det E = E00 c0 + E01 c1 + E02 c2, the cofactors c_m held as quadratic forms
    for (int e = 0; e < 30; ++e) w.at(EP_LAM + e) = 0.0;
    const unsigned char cof[12] = {4, 8, 5, 7, 5, 6, 3, 8, 3, 7, 4, 6};
    for (int m = 0; m < 3; ++m)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b)
                w.at(EP_LAM + 10 * m + ep_i2(a, b)) +=
                    w.at(9 * a + cof[4 * m]) * w.at(9 * b + cof[4 * m + 1]) -
                    w.at(9 * a + cof[4 * m + 2]) * w.at(9 * b + cof[4 * m + 3]);
    for (int m = 0; m < 3; ++m)
        for (int q = 0; q < 10; ++q) {
            const double v = w.at(EP_LAM + 10 * m + q);
            for (int l = 0; l < 4; ++l) w.at(EP_A + 180 + ep_i3(q, l)) += v * w.at(9 * l + m);
        }
    // L = 2 E E^T - tr(E E^T) I as six quadratic forms: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    for (int e = 0; e < 60; ++e) w.at(EP_LAM + e) = 0.0;
    for (int i = 0, u = 0; i < 3; ++i)
        for (int k = i; k < 3; ++k, ++u)
            for (int m = 0; m < 3; ++m)
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b)
                        w.at(EP_LAM + 10 * u + ep_i2(a, b)) += w.at(9 * a + 3 * i + m) * w.at(9 * b + 3 * k + m);
    for (int q = 0; q < 10; ++q) {
        const double tr = (w.at(EP_LAM + q) + w.at(EP_LAM + 30 + q)) + w.at(EP_LAM + 50 + q);
        for (int u = 0; u < 6; ++u) {
            const double v = 2.0 * w.at(EP_LAM + 10 * u + q);
            w.at(EP_LAM + 10 * u + q) = (u == 0 || u == 3 || u == 5) ? v - tr : v;
        }
    }
    // rows 3 i + j: sum_k L_ik E_kj
    const unsigned char pk[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k)
                for (int q = 0; q < 10; ++q) {
                    const double v = w.at(EP_LAM + 10 * pk[3 * i + k] + q);
                    for (int l = 0; l < 4; ++l)
                        w.at(EP_A + 20 * (3 * i + j) + ep_i3(q, l)) += v * w.at(9 * l + 3 * k + j);
                }
}

// Gauss-Jordan on columns 0..9 with partial pivoting.  Rows 4..9 come out fully
// reduced (a one in their own column, zeros in the other nine); rows 0..3 are
// only needed as pivots and are reduced downwards alone.
template <int S> __device__ __forceinline__ void ep_eliminate(const EpWs<S> &w) {
    for (int c = 0; c < 10; ++c) {
        int piv = c;
        double big = fabs(w.at(EP_A + 20 * c + c));
        for (int r = c + 1; r < 10; ++r) {
            const double v = fabs(w.at(EP_A + 20 * r + c));
            if (v > big) { big = v; piv = r; }
        }
        if (piv != c)
            for (int j = c; j < 20; ++j) {
                const double u = w.at(EP_A + 20 * c + j);
                w.at(EP_A + 20 * c + j) = w.at(EP_A + 20 * piv + j);
                w.at(EP_A + 20 * piv + j) = u;
            }
        const double inv = 1.0 / w.at(EP_A + 20 * c + c);
        for (int j = c; j < 20; ++j) w.at(EP_A + 20 * c + j) *= inv;
        for (int r = 0; r < 10; ++r) {
            if (r == c || (r < c && r < 4)) continue;
            const double f = w.at(EP_A + 20 * r + c);
            if (f == 0.0) continue;
            for (int j = c; j < 20; ++j) w.at(EP_A + 20 * r + j) -= f * w.at(EP_A + 20 * c + j);
        }
    }
}

// out += sign * a * b for polynomials of NA and NB coefficients, lowest first
template <int NA, int NB>
__device__ __forceinline__ void ep_pmul(const double (&a)[NA], const double (&b)[NB], double sign,
                                        double (&out)[NA + NB - 1]) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) out[i + j] += sign * (a[i] * b[j]);
}

template <int N> __device__ __forceinline__ double ep_horner(const double (&p)[N], double z) {
    double v = p[N - 1];
#pragma unroll
    for (int j = N - 2; j >= 0; --j) v = v * z + p[j];
    return v;
}

// B(z): row r from the reduced rows (4 + 2 r, 5 + 2 r) as e - z f; coefficients
// lowest first.  Bx, By of degree 3 multiply x and y; B1 of degree 4 is the rest.
struct EpB {
    double x[3][4], y[3][4], o[3][5];
};

template <int S> __device__ __forceinline__ void ep_detpoly(const EpWs<S> &w, EpB &B, double (&c)[11]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double e[10], f[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            e[j] = w.at(EP_A + 20 * (4 + 2 * r) + 10 + j);
            f[j] = w.at(EP_A + 20 * (5 + 2 * r) + 10 + j);
        }
        B.x[r][0] = e[2]; B.x[r][1] = e[1] - f[2]; B.x[r][2] = e[0] - f[1]; B.x[r][3] = -f[0];
        B.y[r][0] = e[5]; B.y[r][1] = e[4] - f[5]; B.y[r][2] = e[3] - f[4]; B.y[r][3] = -f[3];
        B.o[r][0] = e[9]; B.o[r][1] = e[8] - f[9]; B.o[r][2] = e[7] - f[8]; B.o[r][3] = e[6] - f[7];
        B.o[r][4] = -f[6];
    }
    double p1[8], p2[8], p3[7];
#pragma unroll
    for (int j = 0; j < 8; ++j) { p1[j] = 0.0; p2[j] = 0.0; }
#pragma unroll
    for (int j = 0; j < 7; ++j) p3[j] = 0.0;
    ep_pmul<4, 5>(B.y[1], B.o[2], 1.0, p1);
    ep_pmul<4, 5>(B.y[2], B.o[1], -1.0, p1);
    ep_pmul<4, 5>(B.x[1], B.o[2], 1.0, p2);
    ep_pmul<4, 5>(B.x[2], B.o[1], -1.0, p2);
    ep_pmul<4, 4>(B.x[1], B.y[2], 1.0, p3);
    ep_pmul<4, 4>(B.y[1], B.x[2], -1.0, p3);
#pragma unroll
    for (int j = 0; j < 11; ++j) c[j] = 0.0;
    ep_pmul<4, 8>(B.x[0], p1, 1.0, c);
    ep_pmul<4, 8>(B.y[0], p2, -1.0, c);
    ep_pmul<5, 7>(B.o[0], p3, 1.0, c);
}

// The ten roots of c (lowest coefficient first) into w's matrix area: real parts
// at EP_A + k, imaginary parts at EP_A + 10 + k.  False where c is not finite
// or its leading coefficient is 0.
template <int S> __device__ __forceinline__ bool ep_roots(const double (&c)[11], const EpWs<S> &w) {
    bool fin = c[10] != 0.0;
#pragma unroll
    for (int j = 0; j < 11; ++j) fin = fin && isfinite(c[j]);
    if (!fin) return false;
    // starting points: the circle of the roots' geometric mean modulus, spread unevenly
    double r0 = pow(fabs(c[0] / c[10]), 0.1);
    if (!(r0 > 0.0) || !isfinite(r0)) r0 = 1.0;
    const double cs[10] = {0.921, 0.516, -0.086, -0.655, -0.974, -0.921, -0.516, 0.086, 0.655, 0.974};
    const double sn[10] = {0.389, 0.857, 0.996, 0.756, 0.227, -0.389, -0.857, -0.996, -0.756, -0.227};
    for (int k = 0; k < 10; ++k) {
        const double r = r0 * (1.0 + 0.03 * k);
        w.at(EP_A + k) = r * cs[k];
        w.at(EP_A + 10 + k) = r * sn[k];
    }
    for (int it = 0; it < EP_ABERTH_ITERS; ++it) {
        double worst = 0.0;
        for (int k = 0; k < 10; ++k) {
            const double zr = w.at(EP_A + k), zi = w.at(EP_A + 10 + k);
            double pr = c[10], pi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
            for (int j = 9; j >= 0; --j) {
                const double tr = (dr * zr - di * zi) + pr, ti = (dr * zi + di * zr) + pi;
                dr = tr; di = ti;
                const double ur = (pr * zr - pi * zi) + c[j], ui = pr * zi + pi * zr;
                pr = ur; pi = ui;
            }
            const double dn = dr * dr + di * di;
            if ((pr == 0.0 && pi == 0.0) || !(dn > 0.0)) continue;
            const double rr = (pr * dr + pi * di) / dn, ri = (pi * dr - pr * di) / dn;
            double sr = 0.0, si = 0.0;
            for (int j = 0; j < 10; ++j) {
                if (j == k) continue;
                const double ar = zr - w.at(EP_A + j), ai = zi - w.at(EP_A + 10 + j);
                const double an = ar * ar + ai * ai;
                if (an > 0.0) { sr += ar / an; si -= ai / an; }
            }
            const double qr = 1.0 - (rr * sr - ri * si), qi = -(rr * si + ri * sr);
            const double qn = qr * qr + qi * qi;
            double wr = rr, wi = ri;
            if (qn > 0.0) { wr = (rr * qr + ri * qi) / qn; wi = (ri * qr - rr * qi) / qn; }
            if (!(isfinite(wr) && isfinite(wi))) continue;
            w.at(EP_A + k) = zr - wr;
            w.at(EP_A + 10 + k) = zi - wi;
            const double z2 = zr * zr + zi * zi;
            worst = fmax(worst, z2 > 0.0 ? (wr * wr + wi * wi) / z2 : 1.0);
        }
        if (worst <= 1e-30) break;
    }
    return true;
}

// Up to ten solutions of unit norm into E (9 doubles each, stride 1); returns
// how many.  Solutions that are not finite are dropped.
template <int S>
__device__ __forceinline__ int ep_solve(const double (&a)[5], const double (&b)[5], const double (&c)[5],
                                        const double (&d)[5], const EpWs<S> &w, double *E) {
    ep_nullspace(a, b, c, d, w);
    ep_constraints(w);
    ep_eliminate(w);
    EpB B;
    double poly[11];
    ep_detpoly(w, B, poly);
    if (!ep_roots(poly, w)) return 0;
    double dp[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) dp[j] = (j + 1) * poly[j + 1];
    int n = 0;
    for (int k = 0; k < 10; ++k) {
        double z = w.at(EP_A + k);
        const double zi = w.at(EP_A + 10 + k);
        if (!(fabs(zi) <= EP_REAL_TOL * fmax(1.0, fabs(z)))) continue;
        for (int it = 0; it < 3; ++it) {
            const double zn = z - ep_horner(poly, z) / ep_horner(dp, z);
            if (isfinite(zn)) z = zn;
        }
        // [x, y, 1] spans the null space of B(z): the cross product of the two rows that gives the longest one
        double m[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            m[r][0] = ep_horner(B.x[r], z);
            m[r][1] = ep_horner(B.y[r], z);
            m[r][2] = ep_horner(B.o[r], z);
        }
        double v[3] = {0.0, 0.0, 0.0}, vn = -1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int r1 = r == 2 ? 0 : r, r2 = r == 0 ? 1 : 2;  // (0,1) (1,2) (0,2)
            const double cx = m[r1][1] * m[r2][2] - m[r1][2] * m[r2][1];
            const double cy = m[r1][2] * m[r2][0] - m[r1][0] * m[r2][2];
            const double cz = m[r1][0] * m[r2][1] - m[r1][1] * m[r2][0];
            const double nn = (cx * cx + cy * cy) + cz * cz;
            if (nn > vn) { vn = nn; v[0] = cx; v[1] = cy; v[2] = cz; }
        }
        const double x = v[0] / v[2], y = v[1] / v[2];
        double G[9], En[9];
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            G[j] = ((x * w.at(j) + y * w.at(9 + j)) + z * w.at(18 + j)) + w.at(27 + j);
            fin = fin && isfinite(G[j]);
        }
        vp_unit(G, En);
#pragma unroll
        for (int j = 0; j < 9; ++j) fin = fin && isfinite(En[j]);
        if (!fin) continue;
#pragma unroll
        for (int j = 0; j < 9; ++j) E[9 * n + j] = En[j];
        ++n;
    }
    return n;
}

// ------------------------------------------------------------------ the refit's model
__device__ __forceinline__ void ep_cross_mat(const double (&t)[3], const double (&M)[9], double (&out)[9]) {
    // [t]x M
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c] = t[1] * M[6 + c] - t[2] * M[3 + c];
        out[3 + c] = t[2] * M[c] - t[0] * M[6 + c];
        out[6 + c] = t[0] * M[3 + c] - t[1] * M[c];
    }
}

// E = +-s [t]x R with |t| = 1, by the one-sided Jacobi SVD of k_ip_pose: the
// rotation U W V^T (negated where its determinant is negative) and t = u3.  False
// where E is not finite or its second singular value is 0.
__device__ __forceinline__ bool ep_factor(const double (&E)[9], double (&R)[9], double (&t)[3]) {
    bool fin = true;
    double a[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[r][c] = E[3 * r + c];
            fin = fin && isfinite(E[3 * r + c]);
        }
    if (!fin) return false;
    jacobi_onesided<3, 3, 40>(a, V);
    const int z = weakest_column<3, 3>(a);
    const int i1 = (z + 1) % 3, i2 = (z + 2) % 3;
    double v1[3], v2[3], u1[3], u2[3], u3[3], n1 = 0.0, n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v1[k] = i1 == 0 ? a[0][k] : (i1 == 1 ? a[1][k] : a[2][k]);
        v2[k] = i2 == 0 ? a[0][k] : (i2 == 1 ? a[1][k] : a[2][k]);
        u1[k] = i1 == 0 ? V[k][0] : (i1 == 1 ? V[k][1] : V[k][2]);
        u2[k] = i2 == 0 ? V[k][0] : (i2 == 1 ? V[k][1] : V[k][2]);
        u3[k] = z == 0 ? V[k][0] : (z == 1 ? V[k][1] : V[k][2]);
        n1 += v1[k] * v1[k];
        n2 += v2[k] * v2[k];
    }
    n1 = sqrt(n1);
    n2 = sqrt(n2);
    if (!(isfinite(n1) && isfinite(n2) && n1 > 0.0 && n2 > 0.0)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) { v1[k] = v1[k] / n1; v2[k] = v2[k] / n2; }
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                       R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (det < 0.0)
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = -R[k];
    double tn = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) tn += u3[k] * u3[k];
    tn = sqrt(tn);
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = u3[k] / tn;
    return isfinite(tn) && tn > 0.0;
}

// The tangent plane of the unit sphere at t: b1 = t x e_k / |t x e_k| for the axis
// k of the smallest |t_k| (the first of equals), b2 = t x b1.
__device__ __forceinline__ void ep_tangent(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
    int k = 0;
    double m = fabs(t[0]);
    if (fabs(t[1]) < m) { m = fabs(t[1]); k = 1; }
    if (fabs(t[2]) < m) { k = 2; }
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double c[3] = {t[1] * e[2] - t[2] * e[1], t[2] * e[0] - t[0] * e[2], t[0] * e[1] - t[1] * e[0]};
    const double n = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) b1[j] = c[j] / n;
    b2[0] = t[1] * b1[2] - t[2] * b1[1];
    b2[1] = t[2] * b1[0] - t[0] * b1[2];
    b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// G = K^-T M K^-1, not normalised
__device__ __forceinline__ void ep_conj(const EpK &K, const double (&M)[9], double (&G)[9]) {
    double tmp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            tmp[3 * i + c] = (M[3 * i] * K.ki[c] + M[3 * i + 1] * K.ki[3 + c]) + M[3 * i + 2] * K.ki[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            G[3 * r + c] = (K.ki[r] * tmp[c] + K.ki[3 + r] * tmp[3 + c]) + K.ki[6 + r] * tmp[6 + c];
}

// The pixel-space matrix G = K^-T [t]x R K^-1 of the pose and its derivatives by
// the five parameters: the rotation increment w (R <- exp([w]x) R, dE = [t]x
// [e_j]x R) and the two tangent coordinates of t (dE = [b_j]x R).
struct EpModel {
    double G[9], dG[5][9];
};

__device__ __forceinline__ void ep_model(const EpK &K, const double (&R)[9], const double (&t)[3], EpModel &m) {
    double E[9], M[9], b1[3], b2[3];
    ep_cross_mat(t, R, E);
    ep_conj(K, E, m.G);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        ep_cross_mat(e, R, M);
        ep_cross_mat(t, M, E);
        ep_conj(K, E, m.dG[j]);
    }
    ep_tangent(t, b1, b2);
    ep_cross_mat(b1, R, E);
    ep_conj(K, E, m.dG[3]);
    ep_cross_mat(b2, R, E);
    ep_conj(K, E, m.dG[4]);
}

constexpr int EP_NV = 22;  // J^T J (15, upper, row-major packed) | J^T r (5) | cost | bad

// One correspondence's Sampson residual r = e / sqrt(den) in pixels and its row
// of the Jacobian, added to s.  One whose den is not positive and finite counts
// as bad (the cost is then +inf).
__device__ __forceinline__ void ep_accum(const EpModel &m, double x, double y, double u, double v,
                                         double (&s)[EP_NV]) {
    const double *F = m.G;
    const double l0 = (F[0] * x + F[1] * y) + F[2];
    const double l1 = (F[3] * x + F[4] * y) + F[5];
    const double l2 = (F[6] * x + F[7] * y) + F[8];
    const double m0 = (F[0] * u + F[3] * v) + F[6];
    const double m1 = (F[1] * u + F[4] * v) + F[7];
    const double e = (u * l0 + v * l1) + l2;
    const double den = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1);
    if (!(den > 0.0) || !isfinite(den) || !isfinite(e)) {
        s[21] += 1.0;
        return;
    }
    const double sq = sqrt(den), r = e / sq;
    s[20] += r * r;
    double J[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double *D = m.dG[j];
        const double d0 = (D[0] * x + D[1] * y) + D[2];
        const double d1 = (D[3] * x + D[4] * y) + D[5];
        const double d2 = (D[6] * x + D[7] * y) + D[8];
        const double g0 = (D[0] * u + D[3] * v) + D[6];
        const double g1 = (D[1] * u + D[4] * v) + D[7];
        const double de = (u * d0 + v * d1) + d2;
        const double dden = 2.0 * ((l0 * d0 + l1 * d1) + (m0 * g0 + m1 * g1));
        J[j] = de / sq - (r * dden) / (2.0 * den);
        s[15 + j] += J[j] * r;
    }
    int q = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = a; b < 5; ++b) s[q++] += J[a] * J[b];
}

__device__ __forceinline__ int ep_pk(int a, int b) {  // packed upper, row-major, a <= b
    return a * 5 - a * (a - 1) / 2 + (b - a);
}

// (A + lam diag(A)) d = -g by Cholesky; false where the damped matrix is not
// positive definite or the step is not finite
__device__ __forceinline__ bool ep_solve5(const double (&A)[15], const double (&g)[5], double lam, double (&d)[5]) {
    double L[5][5];  // upper factor: L^T L = G
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double dj = A[ep_pk(j, j)] + lam * A[ep_pk(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= L[k][j] * L[k][j];
        ok = ok && dj > 0.0;
        dj = sqrt(dj);
        L[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < 5; ++i) {
            double v = A[ep_pk(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[k][j] * L[k][i];
            L[j][i] = v / dj;
        }
    }
    if (!ok) return false;
    double y[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {  // L^T y = -g
        double t = -g[i];
#pragma unroll
        for (int j = 0; j < i; ++j) t -= L[j][i] * y[j];
        y[i] = t / L[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {  // L d = y
        double t = y[i];
#pragma unroll
        for (int j = i + 1; j < 5; ++j) t -= L[i][j] * d[j];
        d[i] = t / L[i][i];
        ok = ok && isfinite(d[i]);
    }
    return ok;
}

// Levenberg-Marquardt on (R, t) as rv_lm runs it on (R, C): Marquardt's scaling,
// lambda 1e-3, / 10 on an accepted step and x 10 on a rejected one, a step
// accepted only where the cost falls; MINPACK's stop tests at 1e-8 (1 ftol, 2
// xtol, 3 both, 4 gtol, 5 max_nfev).  The size of the parameter vector in the
// xtol test is sqrt(angle(R)^2 + |t|^2).  eval(R, t, A, g, cost) gives the sums
// over the current inliers.  -4: cost at the start not finite (pose kept).
template <class Eval>
__device__ __forceinline__ int ep_lm(const Eval &eval, double (&R)[9], double (&t)[3], int max_nfev) {
    const double tol = 1e-8;
    double A[15], g[5], c0;
    eval(R, t, A, g, c0);
    if (!isfinite(c0)) return -4;
    int nfev = 1, info = 0;
    double lam = 1e-3;
    while (info == 0) {
        double gn = 0.0;
        if (c0 != 0.0) {
            const double fn = sqrt(c0);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const double a = A[ep_pk(j, j)];
                if (a > 0.0) gn = fmax(gn, fabs(g[j]) / (sqrt(a) * fn));
            }
        }
        if (gn <= tol) {
            info = 4;
            break;
        }
        bool accepted = false;
        while (!accepted && info == 0) {
            if (nfev >= max_nfev) {
                info = 5;
                break;
            }
            ++nfev;
            double d[5];
            if (!ep_solve5(A, g, lam, d)) {
                lam *= 10.0;
                continue;
            }
            double dR[9], Rt[9], b1[3], b2[3], tt[3];
            rotvec_to_R(d[0], d[1], d[2], dR);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Rt[3 * r + c] = (dR[3 * r] * R[c] + dR[3 * r + 2] * R[6 + c]) + dR[3 * r + 1] * R[3 + c];
            ep_tangent(t, b1, b2);
            double tn = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                tt[k] = (t[k] + d[3] * b1[k]) + d[4] * b2[k];
                tn += tt[k] * tt[k];
            }
            tn = sqrt(tn);
#pragma unroll
            for (int k = 0; k < 3; ++k) tt[k] = tt[k] / tn;
            double A1[15], g1[5], c1;
            eval(Rt, tt, A1, g1, c1);
            // the linear model's reduction |r|^2 - |r + J d|^2
            double gd = 0.0, dAd = 0.0, pn = 0.0;
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                gd += g[a] * d[a];
                double Ad = 0.0;
#pragma unroll
                for (int b = 0; b < 5; ++b) Ad += A[a <= b ? ep_pk(a, b) : ep_pk(b, a)] * d[b];
                dAd += d[a] * Ad;
                pn += d[a] * d[a];
            }
            const double prered = -(2.0 * gd + dAd) / c0;
            const double actred = 1.0 - c1 / c0;
            const double pnorm = sqrt(pn);
            if (c1 < c0) {
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = Rt[j];
#pragma unroll
                for (int j = 0; j < 3; ++j) t[j] = tt[j];
                c0 = c1;
#pragma unroll
                for (int j = 0; j < 15; ++j) A[j] = A1[j];
#pragma unroll
                for (int j = 0; j < 5; ++j) g[j] = g1[j];
                lam = fmax(lam * 0.1, 1e-15);
                accepted = true;
            } else {
                lam *= 10.0;
            }
            const double sx = R[7] - R[5], sy = R[2] - R[6], sz = R[3] - R[1];
            const double ang = atan2(0.5 * sqrt(sx * sx + sy * sy + sz * sz), 0.5 * ((R[0] + R[4] + R[8]) - 1.0));
            const double xnorm = sqrt(ang * ang + ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]));
            const bool fhit = fabs(actred) <= tol && prered <= tol && 0.5 * actred <= prered;
            const bool xhit = pnorm <= tol * xnorm;
            if (fhit) info = 1;
            if (xhit) info = fhit ? 3 : 2;
        }
    }
    return info;
}

}  // namespace sfm
