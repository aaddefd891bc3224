// gicp_sor.hip — statistical outlier removal on the MI355X (gfx950), DESIGN.md §3s.  The arithmetic is gicp_sor.h's,
// the functions the host yardstick calls.
//
//   k_knn_query      (gicp_knn.hip) the self-query of the stage's rows for k + 1 neighbours: exact fp64 d2 lists in
//                    the order (d2, original index); entry 0 is the row's own zero (or a coincident row's)
//   k_sor_mean       one lane per row: the sequential sum of the roots of entries 1 .. n_i, one division
//   k_sor_tree       the tree sum T(v): a wave's xor-butterfly over 64 consecutive rows, (w0 + w1) + (w2 + w3) per
//                    256 aligned rows, then the same kernel over the partials until one value is left.  Used twice:
//                    over the means, and with (mean_i - mu)^2 formed in the leaves
//   k_sor_flags      mu, sigma, thr from the two sums (every lane the same three operations), the keep flags, and
//                    the reset of the result words
//   rocPRIM, k_filter_compact   (gicp_filter.hip) as for the crop: survivors in their order, exact bounds, M
//
// No floating-point atomics and one fixed order for every sum: the output is bit-identical from call to call, from
// context to context, and to the host's.
#include <hip/hip_runtime.h>

#include "gicp_internal.h"
#include "gicp_sor.h"

namespace gicp {

hipError_t launch_filter_compact(const double*, int64_t, int, int32_t*, int32_t*, void*, size_t, const int32_t*, double*,
                                 int32_t*, unsigned long long*, hipStream_t);   // gicp_filter.hip

namespace {

__global__ void __launch_bounds__(256) k_sor_mean(SorArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    // (a list holds min(k + 1, n) >= 2 entries; fewer would be a broken query: 0 / 0, and the sum is refused)
    A.mean[i] = sor_mean(A.d2 + i * (A.k + 1) + 1, A.cnt[i] - 1);
}

// One level of the tree: v [n] -> out [ceil(n / 256)].  Lanes past n add +0.0, which for summands >= 0 is the
// carried odd element.  Dev2: the leaves are (v_i - mu)^2 with mu = sums[0] / rows.
template <bool Dev2>
__global__ void __launch_bounds__(256) k_sor_tree(const double* __restrict__ v, int64_t n, const double* __restrict__ sums,
                                                  int64_t rows, double* __restrict__ out) {
    __shared__ double s_w[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double x = 0.0;
    if (i < n) x = Dev2 ? sor_dev2(v[i], sor_mu(sums[0], rows)) : v[i];
    // after the step with mask s, lane l holds the sum of the aligned group of 2 s lanes it lies in: the pairwise
    // tree (a + b and b + a are the same bits)
    for (int s = 1; s < 64; s <<= 1) x = sor_add(x, __shfl_xor(x, s));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = sor_add(sor_add(s_w[0], s_w[1]), sor_add(s_w[2], s_w[3]));
}

__global__ void __launch_bounds__(256) k_sor_flags(SorArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double mu = sor_mu(A.sums[0], A.n);
    const double sigma = sor_sigma(A.sums[1], A.n);
    const double thr = sor_thr(mu, A.std_ratio, sigma);
    if (i == 0) {   // (stream order: long before k_filter_compact's atomics)
        A.stats[0] = A.sums[0];
        A.stats[1] = mu;
        A.stats[2] = sigma;
        A.stats[3] = thr;
        for (int a = 0; a < 3; ++a) {
            A.res[a] = ~0ull;
            A.res[3 + a] = 0ull;
        }
        A.res[6] = A.res[7] = 0ull;
    }
    if (i >= A.n) return;
    A.keep[i] = sor_keeps(A.mean[i], thr) ? 1 : 0;
}

// T(v) into *total: level after level through A.part
template <bool Dev2>
hipError_t tree_sum(const SorArgs& A, double* total, hipStream_t st) {
    const double* src = A.mean;
    double* dst = A.part;
    int64_t n = A.n;
    bool leaf = true;
    for (;;) {
        const unsigned g = grid256(n);
        double* o = g == 1 ? total : dst;
        if (leaf && Dev2) hipLaunchKernelGGL(k_sor_tree<true>, dim3(g), dim3(256), 0, st, src, n, (const double*)A.sums, A.n, o);
        else hipLaunchKernelGGL(k_sor_tree<false>, dim3(g), dim3(256), 0, st, src, n, (const double*)nullptr, (int64_t)0, o);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || g == 1) return e;
        leaf = false;
        src = dst;
        dst += g;
        n = g;
    }
}

}  // namespace

// The partials of one tree of n rows, all levels together (SorArgs::part)
size_t sor_part_count(int64_t n) { return (size_t)(2 * ((n + 255) / 256) + 8); }

// Statistical outlier removal on `st`, after the self-query (launch_knn_query) filled A.d2 and A.cnt:
// A.in [n][dim] -> A.out [M][dim], A.idx_out, A.mean, A.stats, A.res (bounds of the kept rows, M in res[6]).
hipError_t launch_sor(const SorArgs& A, hipStream_t st) {
    clear_foreign_error();
    if (A.n < 2 || (A.dim != 2 && A.dim != 3) || A.k < 1 || A.k > kSorMaxK || !A.in || !A.d2 || !A.cnt || !A.mean ||
        !A.part || !A.sums || !A.stats || !A.keep || !A.pos1 || !A.out || !A.res)
        return hipErrorInvalidValue;
    const unsigned g = grid256(A.n);
    hipLaunchKernelGGL(k_sor_mean, dim3(g), dim3(256), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = tree_sum<false>(A, A.sums, st);
    if (e != hipSuccess) return e;
    e = tree_sum<true>(A, A.sums + 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sor_flags, dim3(g), dim3(256), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_filter_compact(A.in, A.n, A.dim, A.keep, A.pos1, A.tmp, A.tmp_bytes, nullptr, A.out, A.idx_out, A.res, st);
}

}  // namespace gicp
