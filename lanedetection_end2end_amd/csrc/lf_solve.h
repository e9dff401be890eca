// In-register inverses of the fit's (order + 1) x (order + 1) normal matrix and the solve from the summed moments: shared by the
// solve kernels of lf_fit.hip (wls_solve_kernel, gels_solve_kernel) and the segmentation-mode step criterion's seg_finish_kernel
// (lf_seg_step.hip): ONE text, so the two routes give the same bits.
#pragma once
#include "lf_common.h"

namespace {

// In-register inverse of a DxD matrix (Gauss-Jordan, partial pivoting = what LAPACK getrf/getri
// amount to for torch.inverse).  Returns 0 ok, 1 singular (zero / non-finite pivot).
template <int D>
__device__ int invert_lu(double (&A)[D][D], double (&Ai)[D][D]) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) Ai[i][j] = (i == j) ? 1.0 : 0.0;
    int bad = 0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        int piv = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            const double a = fabs(A[r][c]);
            if (a > best) { best = a; piv = r; }
        }
#pragma unroll
        for (int r = c + 1; r < D; ++r) {   // swap rows without dynamic register indexing
            if (r == piv) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    double t = A[c][j]; A[c][j] = A[r][j]; A[r][j] = t;
                    t = Ai[c][j]; Ai[c][j] = Ai[r][j]; Ai[r][j] = t;
                }
            }
        }
        const double p = A[c][c];
        if (!(fabs(p) > 0.0) || !isfinite(p)) bad = 1;
        const double ip = 1.0 / p;
#pragma unroll
        for (int j = 0; j < D; ++j) { A[c][j] *= ip; Ai[c][j] *= ip; }
#pragma unroll
        for (int r = 0; r < D; ++r) {
            if (r == c) continue;
            const double f = A[r][c];
#pragma unroll
            for (int j = 0; j < D; ++j) { A[r][j] = fma(-f, A[c][j], A[r][j]); Ai[r][j] = fma(-f, Ai[c][j], Ai[r][j]); }
        }
    }
    return bad;
}

// Cholesky-based inverse (the GELS path).  Returns 0 ok, 2 when A is not positive definite.
template <int D>
__device__ int invert_chol(double (&A)[D][D], double (&Ai)[D][D]) {
    double L[D][D];
    int bad = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) L[i][j] = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !isfinite(d)) bad = 2;
        const double ljj = sqrt(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < D; ++i) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c) {   // solve L L^T x = e_c
        double y[D], x[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = D - 1; i >= 0; --i) {
            double s = y[i];
#pragma unroll
            for (int k = i + 1; k < D; ++k) s -= L[k][i] * x[k];
            x[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = 0; i < D; ++i) Ai[i][c] = x[i];
    }
    return bad;
}

// The fit of one (image, lane) from its summed moments mom = [m_0 .. m_2d, q_0 .. q_d] (Moments<ORDER>'s layout): the Hankel normal
// matrix Z (+ reg on the diagonal, both solvers: BEV/Networks/LSQ_layer.py:120-126), Zi = Z^-1 by `solver`, b = Zi X, highest power
// first.  Returns the inverse's status.
template <int ORDER>
__device__ __forceinline__ int lf_solve_moments(const double* mom, double reg, int solver, double (&b)[ORDER + 1],
                                                double (&Zi)[ORDER + 1][ORDER + 1]) {
    constexpr int D = ORDER + 1, NM = 2 * ORDER + 1;
    double Z[D][D], X[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) Z[i][j] = mom[(ORDER - i) + (ORDER - j)] + (i == j ? reg : 0.0);
        X[i] = mom[NM + (ORDER - i)];
    }
    const int st = (solver == LF_SOLVE_CHOLESKY) ? invert_chol<D>(Z, Zi) : invert_lu<D>(Z, Zi);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) s = fma(Zi[i][j], X[j], s);
        b[i] = s;
    }
    return st;
}

}  // namespace
