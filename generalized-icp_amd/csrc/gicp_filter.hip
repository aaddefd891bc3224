// gicp_filter.hip — the input filters on the MI355X (gfx950): range crop and radius outlier removal
// (DESIGN.md §3o).  The predicates are gicp_filter.h's, the ones the host yardstick runs.
//
//   k_crop_flags     one lane per row: keep flag from d2(p, centre) against min_range^2 / max_range^2
//   rocPRIM          inclusive scan of the flags -> output row + 1
//   k_filter_compact kept rows to their output rows (their order is kept), the input row of each, the exact
//                    min / max per axis by a wave reduction and one ordered-integer atomic per wave and axis, M
//   ROR, on the crop's survivors:
//   k_voxel_key      (gicp_voxel.hip) cell of every point on the absolute grid of edge radius kRorEdge, one key
//   rocPRIM          stable radix sort of (key, row)
//   k_ror_gather     the points in key order, packed: the pair loop reads contiguous rows
//   k_ror_count<D>   the hot kernel: one lane per point IN KEY ORDER, so a wave's lanes share cells and their
//                    candidate loads hit the same lines.  The key packs x high and the last axis low, so the cells
//                    (c_x, c_y, c_z - 1 .. c_z + 1) are one run of sorted keys: 9 runs (2-D: 3) cover the 27 (9)
//                    neighbour cells, each found by a lower and an upper bound and clipped at the axis ends -- a
//                    run never reaches into the row (c_x, c_y +- 1), cells outside the grid are skipped, not
//                    wrapped.  Integer counts; the keep flag and the count go back to the point's original row
//   rocPRIM, k_filter_compact   as for the crop
//
// No floating-point atomics and no order-dependent sums: flags, counts and bounds are integers, so the output is
// bit-identical from call to call and from context to context.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gicp_bounds_dev.h"
#include "gicp_filter.h"
#include "gicp_internal.h"
#include "gicp_runs_dev.h"

namespace gicp {

hipError_t launch_voxel_keys(const VoxelArgs& A, hipStream_t st);   // gicp_voxel.hip

namespace {

template <int D>
__global__ void __launch_bounds__(256) k_crop_flags(CropArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {   // (stream order: long before k_filter_compact's atomics)
        for (int a = 0; a < 3; ++a) {
            A.res[a] = ~0ull;
            A.res[3 + a] = 0ull;
        }
        A.res[6] = A.res[7] = 0ull;
    }
    if (i >= A.n) return;
    double p[D];
    for (int a = 0; a < D; ++a) p[a] = A.in[i * D + a];
    A.keep[i] = crop_keeps(filter_d2<D>(p, A.center), A.lo2, A.hi2) ? 1 : 0;
}

// res[0..5] hold min = all ones, max = 0 and res[6] = 0 when this runs (k_crop_flags, k_voxel_key)
template <int D>
__global__ void __launch_bounds__(256) k_filter_compact(const double* __restrict__ in, int64_t n,
                                                        const int32_t* __restrict__ keep, const int32_t* __restrict__ pos1,
                                                        const int32_t* __restrict__ idx_in, double* __restrict__ out,
                                                        int32_t* __restrict__ idx_out, unsigned long long* res) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    unsigned long long mn[D], mx[D];
    for (int a = 0; a < D; ++a) mn[a] = ~0ull, mx[a] = 0ull;
    if (k) {
        const int64_t m = pos1[i] - 1;
        for (int a = 0; a < D; ++a) {
            const double v = in[i * D + a];
            out[m * D + a] = v;
            mn[a] = mx[a] = enc_ordered(v);
        }
        if (idx_out) idx_out[m] = idx_in ? idx_in[i] : (int32_t)i;
    }
    if (i == n - 1) res[6] = (unsigned long long)pos1[i];   // M
    if (__ballot(k) == 0) return;
    for (int a = 0; a < D; ++a) {
        GICP_WAVE_BOUNDS(mn[a], mx[a])
        // A wave whose bounds cannot improve the words as it reads them sends no atomic.  The words only ever
        // tighten, so a stale read is a looser bound and costs an atomic it did not need, never a skipped one:
        // without the test every wave's six atomics queue on one line (1M rows: 94k of them, ~1 ms)
        if ((threadIdx.x & 63) == 0) {
            if (mn[a] < __atomic_load_n(&res[a], __ATOMIC_RELAXED)) atomicMin(&res[a], mn[a]);
            if (mx[a] > __atomic_load_n(&res[3 + a], __ATOMIC_RELAXED)) atomicMax(&res[3 + a], mx[a]);
        }
    }
}

template <int D>
__global__ void __launch_bounds__(256) k_ror_gather(const double* __restrict__ in, const int32_t* __restrict__ idx_s,
                                                    int64_t n, double* __restrict__ packed) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t o = idx_s[j];
    for (int a = 0; a < D; ++a) packed[j * D + a] = in[o * D + a];
}

// One lane per point in key order.  Full = false: a lane stops at min_neighbors (its count is then a lower
// bound that decides the same keep flag).
template <int D, bool Full>
__global__ void __launch_bounds__(256) k_ror_count(VoxelArgs V, RorArgs R) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= V.n) return;
    const uint64_t* __restrict__ ks = V.keys_s;
    const double* __restrict__ pk = R.packed;
    const uint64_t key = ks[j];
    double p[D];
    for (int a = 0; a < D; ++a) p[a] = pk[j * D + a];
    int32_t count = 0;
    neighbour_runs<D, false>(ks, V.n, key, V.bits, R.cmax, [&](int64_t b, int64_t e) {
        for (int64_t t = b; t < e; ++t) {
            if (t == j) continue;
            double q[D];
            for (int a = 0; a < D; ++a) q[a] = pk[t * D + a];
            count += ror_near(filter_d2<D>(p, q), R.r2) ? 1 : 0;
            if (!Full && count >= R.min_neighbors) return true;
        }
        return false;
    });
    const int64_t o = V.idx_s[j];
    R.keep[o] = count >= R.min_neighbors ? 1 : 0;
    if (Full && R.cnt_out) R.cnt_out[R.idx_in ? R.idx_in[o] : o] = count;
}

template <int D>
hipError_t compact(const double* in, int64_t n, int32_t* keep, int32_t* pos1, void* tmp, size_t tmp_bytes,
                   const int32_t* idx_in, double* out, int32_t* idx_out, unsigned long long* res, hipStream_t st) {
    size_t tb = tmp_bytes;
    hipError_t e = rocprim::inclusive_scan(tmp, tb, keep, pos1, (size_t)n, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_filter_compact<D>, dim3(grid256(n)), dim3(256), 0, st, in, n, (const int32_t*)keep,
                       (const int32_t*)pos1, idx_in, out, idx_out, res);
    return hipGetLastError();
}

// The grid both neighbour stages walk: keys of V.raw's rows, (key, row) sorted, the points packed in key order
template <int D>
hipError_t grid_sort(const VoxelArgs& V, double* packed, hipStream_t st) {
    hipError_t e = launch_voxel_keys(V, st);   // (also resets the result words)
    if (e != hipSuccess) return e;
    size_t tb = V.tmp_bytes;
    e = rocprim::radix_sort_pairs(V.tmp, tb, V.keys, V.keys_s, V.idx, V.idx_s, (size_t)V.n, 0u, (unsigned)V.end_bit, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ror_gather<D>, dim3(grid256(V.n)), dim3(256), 0, st, V.raw, (const int32_t*)V.idx_s, V.n, packed);
    return hipGetLastError();
}

template <int D>
hipError_t ror(const VoxelArgs& V, const RorArgs& R, hipStream_t st) {
    const int64_t n = V.n;
    const unsigned g = grid256(n);
    hipError_t e = grid_sort<D>(V, R.packed, st);
    if (e != hipSuccess) return e;
    if (R.full) hipLaunchKernelGGL((k_ror_count<D, true>), dim3(g), dim3(256), 0, st, V, R);
    else hipLaunchKernelGGL((k_ror_count<D, false>), dim3(g), dim3(256), 0, st, V, R);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return compact<D>(V.raw, n, R.keep, R.pos1, V.tmp, V.tmp_bytes, R.idx_in, R.out, R.idx_out, V.res, st);
}

}  // namespace

// The crop on `st`: A.in [n][dim] -> A.out [M][dim], A.idx_out, A.res (bounds of the kept rows, M in res[6]).
hipError_t launch_crop(const CropArgs& A, hipStream_t st) {
    (void)hipGetLastError();
    if (A.n <= 0 || (A.dim != 2 && A.dim != 3) || !A.in || !A.out || !A.keep || !A.pos1 || !A.res) return hipErrorInvalidValue;
    const unsigned g = grid256(A.n);
    if (A.dim == 3) {
        hipLaunchKernelGGL(k_crop_flags<3>, dim3(g), dim3(256), 0, st, A);
        return compact<3>(A.in, A.n, A.keep, A.pos1, A.tmp, A.tmp_bytes, nullptr, A.out, A.idx_out, A.res, st);
    }
    hipLaunchKernelGGL(k_crop_flags<2>, dim3(g), dim3(256), 0, st, A);
    return compact<2>(A.in, A.n, A.keep, A.pos1, A.tmp, A.tmp_bytes, nullptr, A.out, A.idx_out, A.res, st);
}

// Radius outlier removal on `st`: V.raw [n][dim] -> R.out [M][dim], R.idx_out, R.cnt_out, V.res as for the crop.
hipError_t launch_ror(const VoxelArgs& V, const RorArgs& R, hipStream_t st) {
    (void)hipGetLastError();
    if (V.n <= 0 || (V.dim != 2 && V.dim != 3) || V.end_bit < 1 || V.end_bit > 64 || !V.raw || !R.out || !R.packed ||
        !R.keep || !R.pos1 || !V.res || R.min_neighbors < 1)
        return hipErrorInvalidValue;
    return V.dim == 3 ? ror<3>(V, R, st) : ror<2>(V, R, st);
}

// The stages' last step for a filter of another file (gicp_sor.hip): keep flags -> scan -> k_filter_compact.  The
// result words hold min = all ones, max = 0, M = 0 when this runs.
hipError_t launch_filter_compact(const double* in, int64_t n, int dim, int32_t* keep, int32_t* pos1, void* tmp,
                                 size_t tmp_bytes, const int32_t* idx_in, double* out, int32_t* idx_out,
                                 unsigned long long* res, hipStream_t st) {
    if (n <= 0 || (dim != 2 && dim != 3) || !in || !out || !keep || !pos1 || !res) return hipErrorInvalidValue;
    return dim == 3 ? compact<3>(in, n, keep, pos1, tmp, tmp_bytes, idx_in, out, idx_out, res, st)
                    : compact<2>(in, n, keep, pos1, tmp, tmp_bytes, idx_in, out, idx_out, res, st);
}

// ... and the steps before and between for Euclidean cluster extraction (gicp_cluster.hip): the sorted grid of
// radius outlier removal (keys, sort, k_ror_gather; the result words are reset), and the scan alone
hipError_t launch_grid_sort(const VoxelArgs& V, double* packed, hipStream_t st) {
    if (V.n <= 0 || (V.dim != 2 && V.dim != 3) || V.end_bit < 1 || V.end_bit > 64 || !V.raw || !packed || !V.res) return hipErrorInvalidValue;
    return V.dim == 3 ? grid_sort<3>(V, packed, st) : grid_sort<2>(V, packed, st);
}

hipError_t launch_flag_scan(const int32_t* flags, int32_t* pos1, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t st) {
    if (n <= 0 || !flags || !pos1) return hipErrorInvalidValue;
    size_t tb = tmp_bytes;
    return rocprim::inclusive_scan(tmp, tb, flags, pos1, (size_t)n, rocprim::plus<int32_t>(), st);
}

}  // namespace gicp
