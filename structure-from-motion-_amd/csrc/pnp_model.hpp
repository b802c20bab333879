// The camera-model pieces of PnP shared by pnp.hip (the reference's 4-point
// drop-ins) and register_views.hip (batched 6-point registration): the DLT
// rows of a correspondence, LinearPnP's post-processing of a null vector into
// (C, R), the projection K [R | -R C] and the 6 x 6 Cholesky factor.
// numpy evaluates the small products through OpenBLAS; the operation orders
// are the measured ones (oracle/sfm_oracle_pnp.c header), with FP contraction
// off (lm_small.hpp) and explicit fma() where BLAS fuses.
#pragma once
#include "lm_small.hpp"
#include "sfm_common.hpp"

namespace sfm {

struct Cam3 {
    double k[9];
};

// ------------------------------------------------------------ LAPACK bits
__device__ __forceinline__ double dlapy2_d(double x, double y) {
    const double xa = fabs(x), ya = fabs(y);
    const double w = xa > ya ? xa : ya, z = xa < ya ? xa : ya;
    if (z == 0.0) return w;
    const double q = z / w;
    return w * sqrt(1.0 + q * q);
}

// dlarfg on (alpha; x[0..n-2]) held in registers; returns tau, rewrites
// alpha := beta and x := v tail
template <int L>
__device__ __forceinline__ double dlarfg_d(int n, double &alpha, double (&x)[L], int lo) {
    // x[lo .. lo+n-2] is the vector below/right of alpha
    if (n <= 1) return 0.0;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < L; ++i)
        if (i >= lo && i < lo + n - 1) s += x[i] * x[i];
    const double xnorm = sqrt(s);
    if (xnorm == 0.0) return 0.0;
    const double beta = -copysign(dlapy2_d(alpha, xnorm), alpha);
    const double tau = (beta - alpha) / beta;
    const double sc = 1.0 / (alpha - beta);
#pragma unroll
    for (int i = 0; i < L; ++i)
        if (i >= lo && i < lo + n - 1) x[i] *= sc;
    alpha = beta;
    return tau;
}

// ----------------------------------------------- LinearPnP post-processing
__device__ __forceinline__ double det3_d(const double (&M)[9]) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) +
           M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// column-major 3x3 Householder step on column i of a[col][row]
__device__ __forceinline__ double house_col(double (&a)[3][3], int i) {
    double alpha = a[i][i];
    double x[3] = {a[i][0], a[i][1], a[i][2]};
    const double tau = dlarfg_d<3>(3 - i, alpha, x, i + 1);
    a[i][i] = alpha;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (r > i) a[i][r] = x[r];
    return tau;
}

// apply (I - tau v v^T), v = (.., 1 at i, a[i][i+1..]), to columns c > i
__device__ __forceinline__ void house_apply_left(double (&a)[3][3], int i, double tau) {
    const double aii = a[i][i];
    a[i][i] = 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c <= i) continue;
        double w = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r >= i) w += a[i][r] * a[c][r];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r >= i) a[c][r] -= tau * a[i][r] * w;
    }
    a[i][i] = aii;
}

// LAPACK-path emulation of R := U diag(1,1,-1) Vt for an orthogonal R with
// det < 0 (LinearPnP.py:84-87); see oracle/sfm_oracle_pnp.c flip_last_singular
__device__ void flip_last_singular_d(double (&R)[9]) {
    double a[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c][r] = R[r * 3 + c];
    double tauq[3], d[3], taup0 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        tauq[i] = house_col(a, i);
        d[i] = a[i][i];
        house_apply_left(a, i, tauq[i]);
        if (i == 0) {  // G(0) on row 0, columns 1..2
            double alpha = a[1][0];
            double x[3] = {0.0, 0.0, a[2][0]};
            taup0 = dlarfg_d<3>(2, alpha, x, 2);
            a[1][0] = alpha;
            a[2][0] = x[2];
            const double e = a[1][0];
            a[1][0] = 1.0;
#pragma unroll
            for (int r = 1; r < 3; ++r) {
                double w = 0;
#pragma unroll
                for (int c = 1; c < 3; ++c) w += a[c][r] * a[c][0];
#pragma unroll
                for (int c = 1; c < 3; ++c) a[c][r] -= taup0 * w * a[c][0];
            }
            a[1][0] = e;
        }
    }
    double U[3][3], P[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) { U[c][r] = r == c ? 1.0 : 0.0; P[c][r] = r == c ? 1.0 : 0.0; }
#pragma unroll
    for (int i = 1; i >= 0; --i) {
        double v[3] = {0, 0, 0};
        v[i] = 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r > i) v[r] = a[i][r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double w = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (r >= i) w += v[r] * U[c][r];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (r >= i) U[c][r] -= tauq[i] * v[r] * w;
        }
    }
    {
        const double v[3] = {0.0, 1.0, a[2][0]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double w = 0;
#pragma unroll
            for (int r = 1; r < 3; ++r) w += v[r] * P[c][r];
#pragma unroll
            for (int r = 1; r < 3; ++r) P[c][r] -= taup0 * v[r] * w;
        }
    }
    int ord[3] = {0, 1, 2};
    double sv[3], sg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { sg[i] = d[i] < 0 ? -1.0 : 1.0; sv[i] = fabs(d[i]); }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int isub = 0;
        double smin = sv[ord[0]];
        for (int j = 1; j < 3 - i; ++j)
            if (sv[ord[j]] <= smin) { isub = j; smin = sv[ord[j]]; }
        if (isub != 2 - i) { const int t = ord[isub]; ord[isub] = ord[2 - i]; ord[2 - i] = t; }
    }
    const int k = ord[2];
    double u[3], w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u[r] = k == 0 ? U[0][r] : (k == 1 ? U[1][r] : U[2][r]);
        w[r] = sg[k] * (k == 0 ? P[0][r] : (k == 1 ? P[1][r] : P[2][r]));
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r * 3 + c] -= 2.0 * u[r] * w[c];
}

// LinearPnP.py:61-96 from the null vector p (P = p.reshape(3, 4)).
// Returns the LAPACK-noise branch flag.
__device__ int pnp_post(const double (&p)[12], double (&C)[3], double (&R)[9]) {
    double M[9] = {p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]};
    double t[3] = {p[3], p[7], p[11]};
    if (det3_d(M) < 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = -M[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = -t[k];
    }
    double a[3][3];  // M^T, column-major: a[c][r] = M^T[r][c] = M[c][r]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) a[c][r] = M[c * 3 + r];
    double tau[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        tau[i] = house_col(a, i);
        house_apply_left(a, i, tau[i]);
    }
    double q[3][3];  // Q = H0 H1 H2 I, q[col][row]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) q[c][r] = r == c ? 1.0 : 0.0;
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        double v[3] = {0, 0, 0};
        v[i] = 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r > i) v[r] = a[i][r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double w = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (r >= i) w += v[r] * q[c][r];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (r >= i) q[c][r] -= tau[i] * v[r] * w;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = q[r][c];  // R = Q.T
    double scale = ((a[0][0] + a[1][1]) + a[2][2]) / 3.0;
    if (scale < 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = -R[k];
        scale = -scale;
    }
    int branch = 0;
    if (det3_d(R) < 0) {
        flip_last_singular_d(R);
        branch = 1;
    }
    const double tn[3] = {t[0] / scale, t[1] / scale, t[2] / scale};
#pragma unroll
    for (int i = 0; i < 3; ++i) C[i] = fma(-R[6 + i], tn[2], fma(-R[3 + i], tn[1], (-R[i]) * tn[0]));
    return branch;
}

// normalised image point: inv(K) @ [u, v, 1] (LinearPnP.py:36-39)
__device__ __forceinline__ void pnp_xn(const Cam3 &K, double u, double v, double &xn, double &yn) {
    const double i0 = 1.0 / K.k[0], i4 = 1.0 / K.k[4];
    const double k02 = -(K.k[2] * i0), k12 = -(K.k[5] * i4);
    xn = fma(k02, 1.0, fma(-0.0, v, i0 * u));
    yn = fma(k12, 1.0, fma(i4, v, 0.0 * u));
}

__device__ __forceinline__ void pnp_rows(double Xw, double Yw, double Zw, double xn, double yn, double (&r0)[12],
                                         double (&r1)[12]) {
    r0[0] = Xw; r0[1] = Yw; r0[2] = Zw; r0[3] = 1.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = 0.0; r0[7] = 0.0;
    r0[8] = -xn * Xw; r0[9] = -xn * Yw; r0[10] = -xn * Zw; r0[11] = -xn;
    r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = 0.0; r1[4] = Xw; r1[5] = Yw; r1[6] = Zw; r1[7] = 1.0;
    r1[8] = -yn * Xw; r1[9] = -yn * Yw; r1[10] = -yn * Zw; r1[11] = -yn;
}

// P = K @ hstack([R, -R @ C.reshape(3, 1)]) in numpy's orders
__device__ __forceinline__ void pnp_projection(const Cam3 &K, const double (&C)[3], const double (&R)[9],
                                               double *P) {
    double B[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a0 = -R[r * 3], a1 = -R[r * 3 + 1], a2 = -R[r * 3 + 2];
        B[r * 4 + 3] = fma(a2, C[2], fma(a0, C[0], a1 * C[1]));
#pragma unroll
        for (int c = 0; c < 3; ++c) B[r * 4 + c] = R[r * 3 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            P[r * 4 + c] = fma(K.k[r * 3 + 2], B[8 + c], fma(K.k[r * 3 + 1], B[4 + c], K.k[r * 3] * B[c]));
}

// Cholesky of a 6 x 6 SPD matrix given as its upper triangle (21, row-major
// packed); R upper with R^T R = G.  false on a non-positive pivot.
__device__ __forceinline__ bool chol6(const double *G, double (&R)[6][6]) {
    double A[6][6];
    int u = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { A[i][j] = G[u++]; A[j][i] = A[i][j]; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= R[k][j] * R[k][j];
        ok = ok && d > 0.0;
        d = sqrt(d);
        R[j][j] = d;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i < j) R[j][i] = 0.0;
            if (i <= j) continue;
            double v = A[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= R[k][j] * R[k][i];
            R[j][i] = v / d;
        }
    }
    return ok;
}

}  // namespace sfm
