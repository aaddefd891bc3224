// gicp_sor.h — statistical outlier removal: the arithmetic shared by the device kernels
// (gicp_sor.hip) and the host yardstick (gicp_hostmath.cpp sor_points_host), and the kernels' arguments.
//
// Every operation is fp64 and rounded on its own (no FMA; sqrt and the division are correctly rounded), and every
// sum has one fixed order, so NumPy, the host and the device give the same bits:
//   mean_i  = (sum of sqrt(d2) over the n_i = min(k, M - 1) smallest d2(p_i, p_j), j != i, ascending) / n_i
//   T(v)    = the pairwise tree sum of v in original row order, padded with +0.0 to a power of two
//   mu      = T(mean) / M,  sigma = sqrt(T((mean_i - mu)^2) / (M - 1)),  thr = mu + std_ratio sigma
//   keep i iff mean_i <= thr
#pragma once
#include <stdint.h>

#include <cmath>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace gicp {

// (contraction is off in each of these: inlined into one another the compiler would fuse a product into the sum
// that follows it)

// the mean of the n >= 1 ascending values d2[0 .. n): sequential sum of the roots, one division
__host__ __device__ inline double sor_mean(const double* d2, int n) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int m = 0; m < n; ++m) s = s + sqrt(d2[m]);
    return s / (double)n;
}

// the tree's combine step
__host__ __device__ inline double sor_add(double a, double b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return a + b;
}

// mu of the tree sum t of the M means
__host__ __device__ inline double sor_mu(double t, int64_t M) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return t / (double)M;
}

// the second tree's leaf: (mean_i - mu)^2
__host__ __device__ inline double sor_dev2(double mean, double mu) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double dev = mean - mu;
    return dev * dev;
}

// sigma of the tree sum t2 of the leaves above (the two-pass sample deviation)
__host__ __device__ inline double sor_sigma(double t2, int64_t M) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return sqrt(t2 / (double)(M - 1));
}

// the threshold, product first
__host__ __device__ inline double sor_thr(double mu, double std_ratio, double sigma) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double p = std_ratio * sigma;
    return mu + p;
}

// the bound is inclusive, as every bound of the library
__host__ __device__ inline bool sor_keeps(double mean, double thr) { return mean <= thr; }

constexpr int kSorMaxK = 31;      // the self-query asks for k + 1 rows (kKnnMaxK - 1)
constexpr int kSorStats = 4;      // result doubles: T(mean), mu, sigma, thr

// SOR stage (launch_sor) after the self-query: in [n][dim] -> out [M][dim], rows in their order.
struct SorArgs {
    const double* in;
    int64_t n;
    int32_t dim;
    int32_t k;                // the setting's k: the lists hold k + 1 entries a row, entry 0 the row's own zero
    double std_ratio;
    const double* d2;         // [n][k + 1] the self-query's lists, original row order
    const int32_t* cnt;       // [n] entries of each list (min(k + 1, n))
    double* mean;             // [n] mean_i, original row order
    double* part;             // [2 ceil(n / 256) + 8] scratch: the trees' partials, level after level
    double* sums;             // [2] scratch: T(mean), T(dev^2)
    double* stats;            // [kSorStats]
    int32_t* keep;            // [n] scratch: keep flags
    int32_t* pos1;            // [n] scratch: their inclusive scan
    void* tmp;                // rocPRIM scratch (voxel_temp_bytes)
    size_t tmp_bytes;
    double* out;              // [n][dim]
    int32_t* idx_out;         // [n] input row of each kept row (nullable)
    unsigned long long* res;  // [kVoxelRes]: ordered-integer min[3], max[3] of the kept rows, M
};

}  // namespace gicp
