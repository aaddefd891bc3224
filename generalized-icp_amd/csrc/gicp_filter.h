// gicp_filter.h — the input filters: range crop and radius outlier removal.  The per-pair and
// per-point predicates, shared by the device kernels (gicp_filter.hip) and the host yardstick
// (gicp_hostmath.cpp filter_points_host), and the kernels' arguments.
//
// All arithmetic is fp64 with every product and every sum rounded on its own (no FMA): the squared distance is
//   d2(a, b) = ((dx dx + dy dy) + dz dz),  dx = a_x - b_x,  the z term dropped in 2-D,
// the same bits in either direction and the bits NumPy's expression gives.
//   crop   keep p iff d2(p, c) >= min_range^2 (min_range > 0) and d2(p, c) <= max_range^2 (max_range > 0)
//   ROR    keep survivor i iff #{ j != i, j a survivor : d2(p_i, p_j) <= radius^2 } >= min_neighbors
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace gicp {

// (contraction is off for these operators: the compiler would fuse them into FMAs and move d2 by an ulp)
template <int D>
__host__ __device__ inline double filter_d2(const double* a, const double* b) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double dx = a[0] - b[0], dy = a[1] - b[1];
    double d2 = dx * dx + dy * dy;
    if constexpr (D == 3) {
        const double dz = a[2] - b[2];
        d2 = d2 + dz * dz;
    }
    return d2;
}

// lo2 = min_range^2, hi2 = max_range^2 (one rounded product each); a limit of 0 is no limit
__host__ __device__ inline bool crop_keeps(double d2, double lo2, double hi2) {
    return (lo2 > 0.0 ? d2 >= lo2 : true) && (hi2 > 0.0 ? d2 <= hi2 : true);
}

// r2 = radius^2; the bound is inclusive, as d_c is
__host__ __device__ inline bool ror_near(double d2, double r2) { return d2 <= r2; }

// The ROR grid's cell edge: radius (1 + 2^-16), not radius itself.  d2(p_i, p_j) <= radius^2 bounds the ROUNDED
// difference of two coordinates by radius, the exact one by radius (1 + 2^-53), and the quotients x / edge are
// rounded again (2^-22 of a cell at the 2^31st cell): with edge = radius the two cells can differ by 2 (radius 1,
// x_i = 1 - 2^-53, x_j = 2), with this edge by at most 1 for every coordinate below 2^35 cells.
constexpr double kRorEdge = 1.0 + 1.0 / 65536.0;

// Crop stage (launch_crop): in [n][dim] -> out [M][dim], rows in their order.
struct CropArgs {
    const double* in;
    int64_t n;
    int32_t dim;
    double center[3];
    double lo2, hi2;
    int32_t* keep;            // [n] scratch: keep flags
    int32_t* pos1;            // [n] scratch: their inclusive scan
    void* tmp;                // rocPRIM scratch (voxel_temp_bytes)
    size_t tmp_bytes;
    double* out;              // [n][dim]
    int32_t* idx_out;         // [n] input row of each kept row (nullable)
    unsigned long long* res;  // [kVoxelRes]: ordered-integer min[3], max[3] of the kept rows, M
};

// ROR stage (launch_ror): in [n][dim] (the crop's survivors) -> out [M][dim], rows in their order.  The cells are
// those of the voxel filter's absolute grid with leaf = radius kRorEdge; V carries the key layout and the sort's
// scratch (raw = in, n, dim, leaf, cmin, bits, end_bit, keys, keys_s, idx, idx_s, tmp, tmp_bytes, res).
struct RorArgs {
    int64_t cmax[3];          // highest cell per axis relative to cmin
    double r2;
    int32_t min_neighbors;
    int32_t full;             // 1: count to the end (cnt_out wanted); 0: a point stops counting at min_neighbors
    double* packed;           // [n][dim] scratch: the points in key order
    int32_t* keep;            // [n] scratch: keep flags, original rows
    int32_t* pos1;            // [n] scratch: their inclusive scan
    const int32_t* idx_in;    // [n] row of each `in` row in the caller's cloud (nullable: the row itself)
    int32_t* cnt_out;         // caller's rows: count_i (nullable)
    double* out;              // [n][dim]
    int32_t* idx_out;         // [n] caller's row of each kept row (nullable)
};

}  // namespace gicp
