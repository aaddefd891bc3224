// gicp_sweep.hip — motion compensation on the MI355X (gfx950): de-skew a sweep in place.
//
//   k_deskew_init    the result words: min = all ones, max = 0
//   k_deskew<D>      one lane per point: p' = Exp((tau - ref) xi) p in fp64 (gicp_sweep.h sweep_point), stored
//                    over p; the exact min / max per axis of the de-skewed points by a wave reduction and one
//                    ordered-integer atomic per wave and axis
//
// The twist and ref are kernel arguments: wave-uniform, held in scalar registers.  No floating-point atomics:
// integer min / max do not depend on the order of arrival, so the bounds -- and everything built from them --
// are the same bits on every call.
#include <hip/hip_runtime.h>

#include "gicp_bounds_dev.h"
#include "gicp_internal.h"
#include "gicp_sweep.h"

namespace gicp {

namespace {

__global__ void __launch_bounds__(64) k_deskew_init(unsigned long long* res) {
    if (threadIdx.x < 6) res[threadIdx.x] = threadIdx.x < 3 ? ~0ull : 0ull;
}

template <int D>
__global__ void __launch_bounds__(256) k_deskew(SweepArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < A.n;
    unsigned long long mn[D], mx[D];
    for (int a = 0; a < D; ++a) mn[a] = ~0ull, mx[a] = 0ull;
    if (in) {
        double p[D], q[D];
        for (int a = 0; a < D; ++a) p[a] = A.pts[i * D + a];
        sweep_point<D>(A.xi, A.stamps[i] - A.ref, p, q);
        for (int a = 0; a < D; ++a) {
            A.pts[i * D + a] = q[a];
            mn[a] = mx[a] = enc_ordered(q[a]);
        }
    }
    // (every wave holds a point: the grid is ceil(n / 256) blocks, and waves past n exit here)
    if (__ballot(in) == 0) return;
    for (int a = 0; a < D; ++a) {
        GICP_WAVE_BOUNDS(mn[a], mx[a])
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&A.res[a], mn[a]);
            atomicMax(&A.res[3 + a], mx[a]);
        }
    }
}

}  // namespace

// De-skew A.pts [n][dim] in place on `st`; A.res[0..5] receive the ordered-integer bounds of the result.
hipError_t launch_deskew(const SweepArgs& A, hipStream_t st) {
    clear_foreign_error();
    if (A.n <= 0 || (A.dim != 2 && A.dim != 3) || !A.pts || !A.stamps || !A.res) return hipErrorInvalidValue;
    const unsigned g = grid256(A.n);
    hipLaunchKernelGGL(k_deskew_init, dim3(1), dim3(64), 0, st, A.res);
    if (A.dim == 3) hipLaunchKernelGGL(k_deskew<3>, dim3(g), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_deskew<2>, dim3(g), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace gicp
