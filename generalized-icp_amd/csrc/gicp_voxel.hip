// gicp_voxel.hip — voxel-grid downsampling on the MI355X (gfx950): one centroid per occupied cell of an
// absolute grid of edge `leaf`.
//
//   k_voxel_key      cell of every point, c_a = floor(x_a / leaf) (fp64, correctly rounded division), packed
//                    relative to the cloud's lowest cell into one 64-bit key, x most significant
//   rocPRIM          stable radix sort of (key, original index) over the bits in use
//   k_voxel_heads    head flag where the sorted key changes; rocPRIM inclusive scan -> voxel id + 1
//   k_voxel_reduce   the hot kernel: one wave per 64 sorted points, segmented scan of (x, y, z, 1) keyed by the
//                    head flags; voxels inside a wave are finished there, the rest leave per-wave carries
//   k_voxel_stitch   voxels that span waves, from the carries in wave order
//   k_voxel_keep     count >= min_points; rocPRIM inclusive scan -> output row + 1
//   k_voxel_compact  surviving centroids in key order, their counts, exact min / max per axis, M
//
// The local voxel map merges a posed scan into its rows (cell, sums, count) with the same pieces:
//   k_map_key        the map's rows and the scan's points moved to the world frame, keyed by their cell relative to
//                    the window's lowest corner (rows outside the window: the invalid key), values staged 4-wide
//   rocPRIM, k_voxel_heads, scan   as above
//   k_map_reduce / k_map_stitch    the same segmented scan over the staged rows, storing sums and counts
//   k_map_cells      the new rows' cells decoded from the keys, the number of rows
//   k_map_keep / k_map_centroids   the map as a cloud: sum / count of the rows with count >= min_points
//
// No floating-point atomics anywhere: the order in which a voxel's points are summed is a function of their
// sorted positions only, so the output is bit-identical from run to run and from context to context.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gicp_bounds_dev.h"
#include "gicp_internal.h"

namespace gicp {

namespace {

__global__ void __launch_bounds__(256) k_voxel_key(VoxelArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {   // (stream order: long before k_voxel_compact's atomics)
        for (int a = 0; a < 3; ++a) {
            A.res[a] = ~0ull;
            A.res[3 + a] = 0ull;
        }
        A.res[6] = A.res[7] = 0ull;
    }
    if (i >= A.n) return;
    uint64_t key = 0;
    for (int a = 0; a < A.dim; ++a) {
        const double c = floor(__ddiv_rn(A.raw[i * A.dim + a], A.leaf));
        key = (key << A.bits[a]) | (uint64_t)(int64_t)(c - A.cmin[a]);   // (exact: integers below 2^52)
    }
    A.keys[i] = key;
    A.idx[i] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_voxel_heads(const uint64_t* __restrict__ ks, int64_t n, int32_t* flag) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    flag[j] = (j == 0 || ks[j] != ks[j - 1]) ? 1 : 0;
}

// One wave per 64 consecutive sorted points.  Lane l's segment starts at lane s = its voxel's head if that
// lies in this wave, else 0 (the voxel began in an earlier wave).  Step d of the scan adds lane l - d's
// partial sum when l - d >= s, so after the steps 1, 2, .. 32 lane l holds the sum of lanes s .. l, added in
// a tree that depends on (s, l) alone.  A voxel whose head and end both lie in the wave is finished by its
// last lane.  Per wave, two carries go to k_voxel_stitch: `first`, the sum of the lanes before the wave's
// first head (a voxel continued from earlier waves; zero if lane 0 is a head), and `last`, the sum of the
// wave's final segment when it started at a head of this wave.
//
// Map = true is the local map's weighted variant (k_map_reduce): a sorted row's value is the staged 4-wide row
// vals[o] -- a map row's (sx, sy, sz, count) or a new point's (x, y, z, 1) -- and a finished voxel stores its
// sums and count to sums[vid] instead of a centroid.  The scan itself is the same code.
template <bool Map>
__device__ __forceinline__ void voxel_reduce_body(const VoxelArgs& A, const double* __restrict__ vals,
                                                  double* __restrict__ sums) {
    const int l = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    const int64_t j0 = w * kWave;
    if (j0 >= A.n) return;
    const int nv = (int)(A.n - j0 < kWave ? A.n - j0 : kWave);   // valid lanes 0 .. nv - 1
    const bool valid = l < nv;
    const int64_t j = j0 + l;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    bool head = false;
    int32_t vid = -1;
    if (valid) {
        head = A.flag[j] != 0;
        vid = A.vid1[j] - 1;
        const int64_t o = A.idx_s[j];
        if constexpr (Map) {
            for (int c = 0; c < 4; ++c) v[c] = vals[o * 4 + c];
        } else {
            for (int a = 0; a < A.dim; ++a) v[a] = A.raw[o * A.dim + a];
            v[3] = 1.0;
        }
    }
    const unsigned long long hb = __ballot(head);
    const unsigned long long below = hb & (l == 63 ? ~0ull : ((2ull << l) - 1ull));   // heads at lanes <= l
    const int s = below ? 63 - __clzll((long long)below) : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double t = __shfl_up(v[c], d);
            if (l - d >= s) v[c] += t;
        }
    }
    const int first_head = hb ? __ffsll((long long)hb) - 1 : kWave;
    const int pre = first_head < nv ? first_head : nv;   // lanes of the head-less prefix
    if (pre == 0 ? l == 0 : l == pre - 1) {
        double* cf = A.cfirst + w * 4;
        for (int c = 0; c < 4; ++c) cf[c] = pre == 0 ? 0.0 : v[c];
    }
    if (l == nv - 1) {
        if (hb) {
            double* cl = A.clast + w * 4;
            for (int c = 0; c < 4; ++c) cl[c] = v[c];
        }
        A.cmeta[w] = make_int2(hb ? 1 : 0, hb ? vid : -1);
    } else if (valid && below && ((hb >> (l + 1)) & 1ull)) {   // head and end inside the wave
        if constexpr (Map) {
            for (int c = 0; c < 4; ++c) sums[(int64_t)vid * 4 + c] = v[c];
        } else {
            for (int a = 0; a < 3; ++a) A.cent[(int64_t)vid * 3 + a] = __ddiv_rn(v[a], v[3]);
            A.cnt[vid] = (int32_t)v[3];
        }
    }
}

__global__ void __launch_bounds__(256) k_voxel_reduce(VoxelArgs A) { voxel_reduce_body<false>(A, nullptr, nullptr); }

__global__ void __launch_bounds__(256) k_map_reduce(VoxelArgs A, const double* __restrict__ vals, double* __restrict__ sums) {
    voxel_reduce_body<true>(A, vals, sums);
}

// One wave per wave of k_voxel_reduce that holds a head: its final segment's voxel is `last` of that wave
// plus `first` of the following waves up to and including the next one with a head -- 64 waves per step,
// summed by a fixed butterfly, the steps in wave order.
template <bool Map>
__device__ __forceinline__ void voxel_stitch_body(const VoxelArgs& A, int64_t nwaves, double* __restrict__ sums) {
    const int l = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (w0 >= nwaves) return;
    const int2 m0 = A.cmeta[w0];
    if (!m0.x) return;   // (wave-uniform)
    double acc[4];
    for (int c = 0; c < 4; ++c) acc[c] = A.clast[w0 * 4 + c];
    for (int64_t b = w0 + 1; b < nwaves; b += kWave) {
        const int64_t wv = b + l;
        const bool in = wv < nwaves;
        const unsigned long long hm = __ballot(in && A.cmeta[wv].x != 0);
        const int f = hm ? __ffsll((long long)hm) - 1 : kWave - 1;
        const bool take = in && l <= f;
        double c4[4];
        for (int c = 0; c < 4; ++c) c4[c] = take ? A.cfirst[wv * 4 + c] : 0.0;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1)
#pragma unroll
            for (int c = 0; c < 4; ++c) c4[c] += __shfl_xor(c4[c], o);
        for (int c = 0; c < 4; ++c) acc[c] += c4[c];
        if (hm) break;
    }
    if (l == 0) {
        if constexpr (Map) {
            for (int c = 0; c < 4; ++c) sums[(int64_t)m0.y * 4 + c] = acc[c];
        } else {
            for (int a = 0; a < 3; ++a) A.cent[(int64_t)m0.y * 3 + a] = __ddiv_rn(acc[a], acc[3]);
            A.cnt[m0.y] = (int32_t)acc[3];
        }
    }
}

__global__ void __launch_bounds__(256) k_voxel_stitch(VoxelArgs A, int64_t nwaves) { voxel_stitch_body<false>(A, nwaves, nullptr); }

__global__ void __launch_bounds__(256) k_map_stitch(VoxelArgs A, int64_t nwaves, double* __restrict__ sums) {
    voxel_stitch_body<true>(A, nwaves, sums);
}

__global__ void __launch_bounds__(256) k_voxel_keep(VoxelArgs A, int32_t* keep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= A.n) return;
    const int32_t V = A.vid1[A.n - 1];
    keep[v] = (v < V && A.cnt[v] >= A.min_points) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_voxel_compact(VoxelArgs A, const int32_t* __restrict__ keep,
                                                       const int32_t* __restrict__ pos1) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool k = v < A.n && keep[v] != 0;
    unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    if (k) {
        const int64_t m = pos1[v] - 1;
        for (int a = 0; a < A.dim; ++a) {
            const double c = A.cent[v * 3 + a];
            A.out_xyz[m * A.dim + a] = c;
            mn[a] = mx[a] = enc_ordered(c);
        }
        A.out_cnt[m] = A.cnt[v];
    }
    if (v == 0) {
        A.res[6] = (unsigned long long)pos1[A.n - 1];   // M (flags past the last voxel are 0)
        A.res[7] = (unsigned long long)A.vid1[A.n - 1];
    }
    if (__ballot(k) == 0) return;
    for (int a = 0; a < A.dim; ++a) {
        GICP_WAVE_BOUNDS(mn[a], mx[a])
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&A.res[a], mn[a]);
            atomicMax(&A.res[3 + a], mx[a]);
        }
    }
}

// the cloud's points in its original order: out[perm[i]] = the position of record i
__global__ void __launch_bounds__(256) k_points_out(const PointRec* __restrict__ rec, const int32_t* __restrict__ perm,
                                                    int64_t n, int dim, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t o = perm[i];
    const RecPos p = rec_pos(rec + i);
    const double pv[3] = {p.x, p.y, p.z};
    for (int a = 0; a < dim; ++a) out[o * dim + a] = pv[a];
}

// ---- local voxel map --------------------------------------------------------------------

// Coordinate a of a scan point in the world frame: ((R_a0 x + R_a1 y) + R_a2 z) + t_a, the z term dropped in
// 2-D.  Every product and sum is rounded on its own: contraction is off for these operators (__dmul_rn and
// __dadd_rn are plain operators to the compiler, which fuses them into FMAs and moves the result by an ulp).
__device__ __forceinline__ double map_world(const double* __restrict__ R, double t, const double* __restrict__ p, int dim) {
#pragma clang fp contract(off)
    double w = R[0] * p[0] + R[1] * p[1];
    if (dim == 3) w = w + R[2] * p[2];
    return w + t;
}

// Keys and staged values of one insert.  Rows 0 .. m_old - 1 are the map's: key from the stored cell, value the
// stored sums and count.  Rows m_old .. m_old + n - 1 are the scan's points in their original order, moved to the
// world frame as ((R_a0 x + R_a1 y) + R_a2 z) + t_a with every product and sum rounded on its own (no FMA:
// NumPy's expression gives the same bits), value (x, y, z, 1).  A row outside the window takes kMapInvalid.
__global__ void __launch_bounds__(256) k_map_key(VoxelArgs A, MapArgs M) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0)   // (stream order: long before k_map_cells / k_map_centroids write them)
        for (int a = 0; a < kVoxelRes; ++a) A.res[a] = a < 3 ? ~0ull : 0ull;
    if (i >= A.n) return;
    double v[4] = {0.0, 0.0, 0.0, 1.0};
    int64_t rel[3] = {0, 0, 0};
    bool in = true;
    if (i < M.m_old) {
        for (int c = 0; c < 4; ++c) v[c] = M.sums_old[i * 4 + c];
        for (int a = 0; a < M.dim; ++a) {
            rel[a] = (int64_t)M.cells_old[i * 3 + a] - M.lo[a];
            in = in && rel[a] >= 0 && rel[a] <= M.span;
        }
    } else {
        const double* p = M.pts + (i - M.m_old) * M.dim;
        for (int a = 0; a < M.dim; ++a) {
            const double w = map_world(M.R + a * 3, M.t[a], p, M.dim);
            v[a] = w;
            const double r = floor(__ddiv_rn(w, M.leaf)) - (double)M.lo[a];   // (exact inside the window)
            const bool ok = r >= 0.0 && r <= (double)M.span;                  // (false for NaN)
            in = in && ok;
            rel[a] = ok ? (int64_t)r : 0;
        }
    }
    uint64_t key = 0;
    for (int a = 0; a < M.dim; ++a) key = (key << M.bits) | (uint64_t)rel[a];
    A.keys[i] = in ? key : kMapInvalid;
    A.idx[i] = (int32_t)i;
    for (int c = 0; c < 4; ++c) M.vals[i * 4 + c] = v[c];
}

// The cells of the new rows, decoded from the sorted keys at the head of every valid voxel (valid keys sort
// before kMapInvalid, so voxel id = row), and the number of rows.
__global__ void __launch_bounds__(256) k_map_cells(VoxelArgs A, MapArgs M) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= A.n) return;
    const uint64_t key = A.keys_s[j];
    if (j == A.n - 1) A.res[6] = (unsigned long long)(A.vid1[j] - (key == kMapInvalid ? 1 : 0));
    if (!A.flag[j] || key == kMapInvalid) return;
    const int64_t row = A.vid1[j] - 1;
    const uint64_t mask = M.bits ? (1ull << M.bits) - 1ull : 0ull;
    for (int a = 0; a < 3; ++a) {
        const int sh = (M.dim - 1 - a) * M.bits;
        M.cells_new[row * 3 + a] = a < M.dim ? (int32_t)(M.lo[a] + (int64_t)((key >> sh) & mask)) : 0;
    }
}

__global__ void __launch_bounds__(256) k_map_keep(const double* __restrict__ sums, int64_t m, int32_t min_points,
                                                  int32_t* __restrict__ keep, unsigned long long* res) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v == 0)
        for (int a = 0; a < kVoxelRes; ++a) res[a] = a < 3 ? ~0ull : 0ull;
    if (v >= m) return;
    keep[v] = sums[v * 4 + 3] >= (double)min_points ? 1 : 0;
}

// Map -> cloud: the centroid sum / count (one correctly rounded division) of every kept row, in key order, their
// exact min / max per axis and their number.
__global__ void __launch_bounds__(256) k_map_centroids(const double* __restrict__ sums, int64_t m, int dim,
                                                       const int32_t* __restrict__ keep, const int32_t* __restrict__ pos1,
                                                       double* __restrict__ out_xyz, unsigned long long* res) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool k = v < m && keep[v] != 0;
    unsigned long long mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    if (k) {
        const int64_t r = pos1[v] - 1;
        const double cnt = sums[v * 4 + 3];
        for (int a = 0; a < dim; ++a) {
            const double c = __ddiv_rn(sums[v * 4 + a], cnt);
            out_xyz[r * dim + a] = c;
            mn[a] = mx[a] = enc_ordered(c);
        }
    }
    if (v == m - 1) res[6] = (unsigned long long)pos1[v];
    if (__ballot(k) == 0) return;
    for (int a = 0; a < dim; ++a) {
        GICP_WAVE_BOUNDS(mn[a], mx[a])
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&res[a], mn[a]);
            atomicMax(&res[3 + a], mx[a]);
        }
    }
}

}  // namespace

// bytes of rocPRIM scratch launch_voxel needs for n points sorted on `end_bit` key bits
hipError_t voxel_temp_bytes(int64_t n, int end_bit, size_t* bytes, hipStream_t st) {
    (void)hipGetLastError();
    size_t b_sort = 0, b_scan = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr,
                                             (int32_t*)nullptr, (size_t)n, 0u, (unsigned)end_bit, st);
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(nullptr, b_scan, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, rocprim::plus<int32_t>(),
                                st);
    if (e != hipSuccess) return e;
    *bytes = b_sort > b_scan ? b_sort : b_scan;
    return hipSuccess;
}

// The keys alone (radius outlier removal, gicp_filter.hip, sorts the same grid): A.raw, n, dim, leaf, cmin, bits ->
// A.keys, A.idx = 0 .. n - 1; A.res is reset as launch_voxel resets it.
hipError_t launch_voxel_keys(const VoxelArgs& A, hipStream_t st) {
    (void)hipGetLastError();
    if (A.n <= 0 || (A.dim != 2 && A.dim != 3) || !A.raw || !A.keys || !A.idx || !A.res) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_voxel_key, dim3(grid256(A.n)), dim3(256), 0, st, A);
    return hipGetLastError();
}

// The whole filter on `st`: A.raw [n][dim] -> A.out_xyz [M][dim], A.out_cnt [M], A.res (kVoxelRes words:
// ordered-integer min[3], max[3] of the surviving centroids, M, the number of occupied voxels).
hipError_t launch_voxel(const VoxelArgs& A, hipStream_t st) {
    (void)hipGetLastError();
    const int64_t n = A.n;
    if (n <= 0 || (A.dim != 2 && A.dim != 3) || A.end_bit < 1 || A.end_bit > 64) return hipErrorInvalidValue;
    const unsigned g = grid256(n);
    hipLaunchKernelGGL(k_voxel_key, dim3(g), dim3(256), 0, st, A);
    size_t tb = A.tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(A.tmp, tb, A.keys, A.keys_s, A.idx, A.idx_s, (size_t)n, 0u,
                                             (unsigned)A.end_bit, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxel_heads, dim3(g), dim3(256), 0, st, (const uint64_t*)A.keys_s, n, A.flag);
    tb = A.tmp_bytes;
    e = rocprim::inclusive_scan(A.tmp, tb, A.flag, A.vid1, (size_t)n, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    const int64_t nwaves = (n + kWave - 1) / kWave;
    const unsigned gw = (unsigned)((nwaves + kWavesPerWG - 1) / kWavesPerWG);
    hipLaunchKernelGGL(k_voxel_reduce, dim3(gw), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_voxel_stitch, dim3(gw), dim3(256), 0, st, A, nwaves);
    // the head flags and the unsorted indices are dead now: their buffers take the keep flags and their scan
    int32_t* keep = A.flag;
    int32_t* pos1 = A.idx;
    hipLaunchKernelGGL(k_voxel_keep, dim3(g), dim3(256), 0, st, A, keep);
    tb = A.tmp_bytes;
    e = rocprim::inclusive_scan(A.tmp, tb, keep, pos1, (size_t)n, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxel_compact, dim3(g), dim3(256), 0, st, A, (const int32_t*)keep, (const int32_t*)pos1);
    return hipGetLastError();
}

// One map insert on `st`.  A carries the filter's scratch for A.n = M.m_old + M.n rows and
// A.end_bit = max(1, dim * M.bits); M the old rows, the scan, the pose, the window and the output buffers.
// A.res[6] receives the number of rows of the new map.
hipError_t launch_map_insert(const VoxelArgs& A, const MapArgs& M, hipStream_t st) {
    (void)hipGetLastError();
    const int64_t n = A.n;
    if (n <= 0 || n != M.m_old + M.n || (M.dim != 2 && M.dim != 3) || A.end_bit < 1 || A.end_bit > 64 || M.bits < 0 ||
        M.dim * M.bits > 63)
        return hipErrorInvalidValue;
    const unsigned g = grid256(n);
    hipLaunchKernelGGL(k_map_key, dim3(g), dim3(256), 0, st, A, M);
    size_t tb = A.tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(A.tmp, tb, A.keys, A.keys_s, A.idx, A.idx_s, (size_t)n, 0u,
                                             (unsigned)A.end_bit, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_voxel_heads, dim3(g), dim3(256), 0, st, (const uint64_t*)A.keys_s, n, A.flag);
    tb = A.tmp_bytes;
    e = rocprim::inclusive_scan(A.tmp, tb, A.flag, A.vid1, (size_t)n, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    const int64_t nwaves = (n + kWave - 1) / kWave;
    const unsigned gw = (unsigned)((nwaves + kWavesPerWG - 1) / kWavesPerWG);
    hipLaunchKernelGGL(k_map_reduce, dim3(gw), dim3(256), 0, st, A, (const double*)M.vals, M.sums_new);
    hipLaunchKernelGGL(k_map_stitch, dim3(gw), dim3(256), 0, st, A, nwaves, M.sums_new);
    hipLaunchKernelGGL(k_map_cells, dim3(g), dim3(256), 0, st, A, M);
    return hipGetLastError();
}

// The map's rows with count >= min_points as a cloud: centroids [M][dim] in key order into out_xyz, and into
// res the filter's result words (ordered-integer min[3], max[3], M).  keep / pos1: [m] scratch.
hipError_t launch_map_centroids(const double* sums, int64_t m, int dim, int min_points, int32_t* keep, int32_t* pos1,
                                void* tmp, size_t tmp_bytes, double* out_xyz, unsigned long long* res, hipStream_t st) {
    (void)hipGetLastError();
    if (m <= 0 || (dim != 2 && dim != 3)) return hipErrorInvalidValue;
    const unsigned g = grid256(m);
    hipLaunchKernelGGL(k_map_keep, dim3(g), dim3(256), 0, st, sums, m, (int32_t)min_points, keep, res);
    size_t tb = tmp_bytes;
    hipError_t e = rocprim::inclusive_scan(tmp, tb, keep, pos1, (size_t)m, rocprim::plus<int32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_centroids, dim3(g), dim3(256), 0, st, sums, m, dim, (const int32_t*)keep, (const int32_t*)pos1,
                       out_xyz, res);
    return hipGetLastError();
}

hipError_t launch_points_out(const PointRec* rec, const int32_t* perm, int64_t n, int dim, double* out, hipStream_t st) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_points_out, dim3(grid256(n)), dim3(256), 0, st, rec, perm, n, dim, out);
    return hipGetLastError();
}

}  // namespace gicp
