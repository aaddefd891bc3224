// gicp_bounds_dev.h — the exact per-axis bounds of a cloud the device just wrote (gicp_voxel.hip, gicp_sweep.hip,
// gicp_filter.hip): doubles as ordered integers, reduced over the wave; each kernel publishes the wave's result
// with integer atomics in its own way.  No floating-point atomics: integer min / max do not depend on the order
// of arrival, so the bounds are the same bits on every call.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "gicp_internal.h"

namespace gicp {

// doubles as unsigned integers of the same order (-0.0 < +0.0; gicp_hostmath.cpp dec_ordered is the inverse)
__device__ __forceinline__ unsigned long long enc_ordered(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// The wave's min of mn and max of mx (unsigned long long lvalues), in every lane: an xor butterfly.  A macro, as
// GICP_WAVE_REDUCE is: as a function (taking the two by reference, by value, or as arrays and an axis) it is
// inlined at another point of the compiler's pipeline and the callers' shuffles are scheduled differently.  Its
// locals carry the wb_ prefix; a statement, used without a semicolon.
#define GICP_WAVE_BOUNDS(mn, mx)                                                         \
    _Pragma("unroll") for (int wb_o_ = 1; wb_o_ < kWave; wb_o_ <<= 1) {                  \
        const unsigned long long wb_lo_ = __shfl_xor(mn, wb_o_);                         \
        const unsigned long long wb_hi_ = __shfl_xor(mx, wb_o_);                         \
        mn = wb_lo_ < mn ? wb_lo_ : mn;                                                  \
        mx = wb_hi_ > mx ? wb_hi_ : mx;                                                  \
    }

}  // namespace gicp
