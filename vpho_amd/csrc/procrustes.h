// Procrustes pieces shared by the hand metric kernels (metrics.hip) and the hand benchmark kernels (hand_bench.hip): both files call the
// same functions, so an aligned point has the same fp64 bits wherever it is formed.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace vpho {

// eigen-decomposition of a symmetric 3x3 (cyclic Jacobi); eigenvalues descending, eigenvectors in the columns of V
__device__ inline void sym3_eig(double A[3][3], double w[3], double V[3][3]) {
    // all indices are compile-time constants (unrolled pairs, a three-element sorting network on whole columns): registers, no scratch
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        if (!(off > 1e-300)) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (!(fabs(A[p][q]) > 1e-300)) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double a = A[k][p], b = A[k][q]; A[k][p] = c * a - s * b; A[k][q] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double a = A[p][k], b = A[q][k]; A[p][k] = c * a - s * b; A[q][k] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
            }
    }
    // eigenvalues descending with their columns: the exchanges of the former index sort (0,1), (0,2), (1,2), each on a strict ">"
    w[0] = A[0][0]; w[1] = A[1][1]; w[2] = A[2][2];
    auto cswap = [&](auto I, auto J) {
        constexpr int i = decltype(I)::value, j = decltype(J)::value;
        const bool sw = w[j] > w[i];
        const double wi = w[i], wj = w[j];
        w[i] = sw ? wj : wi; w[j] = sw ? wi : wj;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double a = V[k][i], b = V[k][j]; V[k][i] = sw ? b : a; V[k][j] = sw ? a : b; }
    };
    cswap(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    cswap(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
    cswap(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
}

__device__ inline double wave_sum(double v) {
    // xor butterfly: every lane adds the same two operands at every level, so all lanes end with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// similarity transform of rigid_transform_3D_AtoB (transform_fn.py:43-58) from the centred cross-covariance H, the one solve of all
// three PA kernels: eigen of H^T H gives V and S^2, U from H V, R = V U^T with the reflection fix; T = [c R | cB - c R cA]
__device__ inline void similarity_from_cov(const double H[3][3], const double cA[3], const double cB[3], double varA, double T[12]) {
    double M[3][3], w[3], V[3][3], U[3][3], s[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { M[i][j] = 0; for (int k = 0; k < 3; ++k) M[i][j] += H[k][i] * H[k][j]; }
    sym3_eig(M, w, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = sqrt(w[k] > 0 ? w[k] : 0.0);
    // U is orthonormal by construction.  Jacobi on H^T H separates v2 from v3 only to eps * w1 / (w2 - w3): with a rank-1 H (s2/s1 ~ 1e-7,
    // a collinear ground truth) H v3 keeps a component along u2 far above any threshold on |H v3|, and normalising it gave a U with two
    // parallel columns.  So: U0 = H v1 / |H v1|; U1 = H v2 orthogonalised against U0 (any perpendicular if nothing is left of it);
    // U2 = +-(U0 x U1), the sign from H v3 where |H v3| is significant (it decides a reflection), else by the determinant rule below.
    double u[3][3], nu[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { u[i][k] = 0; for (int j = 0; j < 3; ++j) u[i][k] += H[i][j] * V[j][k]; }
        nu[k] = sqrt(u[0][k] * u[0][k] + u[1][k] * u[1][k] + u[2][k] * u[2][k]);
    }
    const double tiny = 1e-12 * (s[0] + 1e-300);
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][0] = u[i][0] / (nu[0] > 0 ? nu[0] : 1.0);
    const double d01 = U[0][0] * u[0][1] + U[1][0] * u[1][1] + U[2][0] * u[2][1];
    double g[3] = {u[0][1] - d01 * U[0][0], u[1][1] - d01 * U[1][0], u[2][1] - d01 * U[2][0]};
    double ng = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    if (!(ng > tiny)) {   // rank 1 to rounding: U0 x e, e the axis U0 is least along
        const double a0 = fabs(U[0][0]), a1 = fabs(U[1][0]), a2 = fabs(U[2][0]);
        const bool p0 = a0 <= a1 && a0 <= a2, p1 = !p0 && a1 <= a2;
        const double e0 = p0 ? 1.0 : 0.0, e1 = p1 ? 1.0 : 0.0, e2 = (p0 || p1) ? 0.0 : 1.0;
        g[0] = U[1][0] * e2 - U[2][0] * e1;
        g[1] = U[2][0] * e0 - U[0][0] * e2;
        g[2] = U[0][0] * e1 - U[1][0] * e0;
        ng = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][1] = g[i] / (ng > 0 ? ng : 1.0);
    {
        double x[3] = {U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1], U[0][0] * U[1][1] - U[1][0] * U[0][1]};
        const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        const double sgn = (nu[2] > tiny && u[0][2] * x[0] + u[1][2] * x[1] + u[2][2] * x[2] < 0) ? -1.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) U[i][2] = sgn * (x[i] / (nx > 0 ? nx : 1.0));
    }
    auto build = [&](double R[3][3]) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { R[i][j] = 0; for (int k = 0; k < 3; ++k) R[i][j] += V[i][k] * U[j][k]; }
    };
    double R[3][3];
    build(R);
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0) {
        s[2] = -s[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) V[i][2] = -V[i][2];
        build(R);
    }
    const double c = (s[0] + s[1] + s[2]) / varA;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double t = cB[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) { T[i * 3 + j] = c * R[i][j]; t -= c * R[i][j] * cA[j]; }
        T[9 + i] = t;
    }
}

}  // namespace vpho
