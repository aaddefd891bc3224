// gicp_runs_dev.h — the neighbour cells of a point on the sorted absolute grid (gicp_voxel.hip's keys), as runs of the
// sorted keys.  Shared by radius outlier removal (gicp_filter.hip) and Euclidean cluster extraction
// (gicp_cluster.hip, §3t): one copy of the bounds search and of the clipping at the axis ends.
//
// The key packs x high and the last axis low, so the cells (c_x, c_y, c_z - 1 .. c_z + 1) are one contiguous run of
// sorted keys: 9 runs (2-D: 3) cover the 27 (9) neighbour cells.  A run is clipped at the ends of the last axis -- it
// never reaches into the row (c_x, c_y +- 1) -- and a row whose c_x or c_y lies below 0 or above the axis maximum is
// skipped, not wrapped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gicp {

// first sorted key >= k (Upper: > k) in ks[0 .. n)
template <bool Upper>
__device__ __forceinline__ int64_t key_bound(const uint64_t* __restrict__ ks, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = ks[mid];
        if (Upper ? v <= k : v < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// f(b, e) for every run [b, e) of sorted keys that holds neighbour cells of the cell of `key`; f returns true to
// stop.  bits: key bits per axis, cmax: the highest cell per axis relative to the grid's lowest.  Forward: only the
// runs that do not lie wholly before the key's own (the own row of cells and the rows after it: 5 of 9, 2 of 3) --
// for a symmetric relation that the lane of the earlier key settles.
template <int D, bool Forward, class F>
__device__ __forceinline__ void neighbour_runs(const uint64_t* __restrict__ ks, int64_t n, uint64_t key, const int32_t (&bits)[3],
                                               const int64_t (&cmax)[3], F&& f) {
    // the cells, relative to cmin: the last axis in the low bits
    const int bl = bits[D - 1], bm = D == 3 ? bits[1] : 0;
    const int64_t cl = (int64_t)(key & ((1ull << bl) - 1ull));
    const int64_t cm = D == 3 ? (int64_t)((key >> bl) & ((1ull << bm) - 1ull)) : 0;
    const int64_t ch = (int64_t)(key >> (bl + bm));
    const int64_t l0 = cl > 0 ? cl - 1 : 0, l1 = cl < cmax[D - 1] ? cl + 1 : cl;   // (clipped at the axis ends)
    for (int dh = Forward ? 0 : -1; dh <= 1; ++dh) {
        const int64_t h = ch + dh;
        if (h < 0 || h > cmax[0]) continue;
        for (int dm = (D == 3 ? -1 : 0); dm <= (D == 3 ? 1 : 0); ++dm) {
            if (Forward && dh == 0 && dm < 0) continue;
            const int64_t m = cm + dm;
            if (D == 3 && (m < 0 || m > cmax[1])) continue;
            const uint64_t row = (((uint64_t)h << bm) | (uint64_t)m) << bl;
            const int64_t b = key_bound<false>(ks, n, row | (uint64_t)l0);
            const int64_t e = key_bound<true>(ks, n, row | (uint64_t)l1);
            if (f(b, e)) return;
        }
    }
}

}  // namespace gicp
