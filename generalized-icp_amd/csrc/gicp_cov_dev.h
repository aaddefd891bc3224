// gicp_cov_dev.h — the per-point surface covariance from a neighbourhood's shifted sums (gicp.py:11-35), shared by
// k_knn_cov (gicp_cov.hip) and k_batch_cov (gicp_batch.hip): the sums, the smallest eigenvector, the descriptor
// C = a I - m m^T.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace gicp {

// ---------------------------------------------------------------------------
// surface covariance: k nearest (self included, < d_n), shifted sums, eigen
// ---------------------------------------------------------------------------
template <int D>
struct CovSums {
    double n;
    double s[D];
    double ss[D * (D + 1) / 2];
};

template <int D>
__device__ __forceinline__ void cov_add(CovSums<D>& A, const double* d) {
    A.n += 1.0;
    int k = 0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        A.s[a] += d[a];
#pragma unroll
        for (int b = a; b < D; ++b) A.ss[k++] += d[a] * d[b];
    }
}

// Symmetric 3x3 eigenvector of the smallest eigenvalue (cyclic Jacobi, fp64).  The sweeps are one text; the
// eigenvector is picked as V[k][m] with m found at run time, which puts V into a scratch frame (k_knn_cov carries
// one), or, with Select, by selects over the three columns (k_batch_cov: no scratch).  The same bits either way.
template <bool Select = false>
__device__ __forceinline__ void smallest_eigvec3(double A[3][3], double* n) {
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off == 0.0) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0;
            const int qq = pq == 0 ? 1 : 2;
            const double apq = A[p][qq];
            if (apq == 0.0) continue;
            const double theta = (A[qq][qq] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) {  // A <- J^T A J
                const double akp = A[k][p], akq = A[k][qq];
                A[k][p] = c * akp - s * akq;
                A[k][qq] = s * akp + c * akq;
            }
            for (int k = 0; k < 3; ++k) {
                const double apk = A[p][k], aqk = A[qq][k];
                A[p][k] = c * apk - s * aqk;
                A[qq][k] = s * apk + c * aqk;
            }
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k][p], vkq = V[k][qq];
                V[k][p] = c * vkp - s * vkq;
                V[k][qq] = s * vkp + c * vkq;
            }
        }
    }
    if constexpr (Select) {
        const bool m1 = A[1][1] < A[0][0];
        const double am = m1 ? A[1][1] : A[0][0];
        const bool m2 = A[2][2] < am;
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = m2 ? V[k][2] : (m1 ? V[k][1] : V[k][0]);
    } else {
        int m = 0;
        if (A[1][1] < A[m][m]) m = 1;
        if (A[2][2] < A[m][m]) m = 2;
        for (int k = 0; k < 3; ++k) n[k] = V[k][m];
    }
}

// C = a I - m m^T from the neighbourhood sums (gicp.py:11-16 / SURVEY.md §8.A); Select: smallest_eigvec3's pick
template <int D, bool Select = false>
__device__ __forceinline__ double4 cov_descriptor(const CovSums<D>& A, int min_nb, double eps_a, double m_scale) {
    double4 out;
    out.x = 1.0;
    out.y = out.z = out.w = 0.0;  // identity (gicp.py:33-34)
    if (A.n < (double)min_nb) return out;
    const double n = A.n;
    double C[D][D];
    int k = 0;
    for (int a = 0; a < D; ++a)
        for (int b = a; b < D; ++b) {
            C[a][b] = C[b][a] = (A.ss[k] - A.s[a] * A.s[b] / n) / (n - 1.0);
            ++k;
        }
    out.x = eps_a;
    if (D == 2) {
        // principal eigenvector at 0.5 atan2(2 cxy, cxx - cyy); thin direction is its normal
        const double phi = 0.5 * atan2(2.0 * C[0][1], C[0][0] - C[1][1]);
        double sp, cp;
        sincos(phi, &sp, &cp);
        out.y = -sp * m_scale;
        out.z = cp * m_scale;
    } else {
        double M[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) M[a][b] = C[a % D][b % D];
        double nv[3];
        smallest_eigvec3<Select>(M, nv);
        out.y = nv[0] * m_scale;
        out.z = nv[1] * m_scale;
        out.w = nv[2] * m_scale;
    }
    return out;
}

}  // namespace gicp
