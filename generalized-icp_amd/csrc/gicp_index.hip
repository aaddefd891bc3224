// gicp_index.hip — the spatial index of a cloud on the MI355X (gfx950): Morton codes, tiles of <= 64 points
// with their boxes and sub-boxes, the two levels of blocks above them, and the reset of the per-tile search
// state.  The reference has no counterpart: it answers its neighbour queries with a KD-tree
// (gicp.py:19-20, gicp.py:126-127); this index is what k_knn_cov and k_corr search instead.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gicp_internal.h"
#include "gicp_search_dev.h"   // morton_code: k_corr's seed lookup codes a query with the function k_morton sorts by
#include "gicp_wave_dev.h"

namespace gicp {

// ---------------------------------------------------------------------------
// index build
// ---------------------------------------------------------------------------
__global__ void k_morton(const double* __restrict__ xyz, int64_t n, int dim, DevCloud fr, uint32_t* codes,
                         int32_t* idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[3] = {0, 0, 0};
    for (int a = 0; a < dim; ++a) p[a] = xyz[i * dim + a];
    codes[i] = morton_code(p, dim, fr.lo, fr.scale, fr.bits);
    idx[i] = (int32_t)i;
}

// One wave per tile: gather the tile's points (original order -> sorted), fp64 AABB,
// centre, fp32 relative coordinates, half-extents and radius.
// Order of the rows inside a tile: a recursive median split instead of the Morton order the tile
// was cut from.  Rows 0-31 / 32-63 are the halves along the tile's longest axis, each half is split
// along its own longest axis, and so on down to the sub-tile size, so the sub-tiles are compact
// boxes (a Morton run can straddle a cell boundary and span the whole tile).  Rows carry no meaning beyond the
// sub-tile boxes (ties are resolved on original indices), so only the culling changes.
__device__ __forceinline__ void split_order(double (&p)[3], int& o, int dim, bool v) {
    const int l = lane_id();
    const int cnt = __popcll(__ballot(v));   // valid rows are lanes 0 .. cnt-1, and stay there
    const bool vv = l < cnt;
    // each level halves every segment of `seg` rows along that segment's own longest axis
    for (int seg = kTile; seg > kSubRows; seg >>= 1) {
        double mn[3], mx[3];
        for (int a = 0; a < 3; ++a) {
            mn[a] = vv ? p[a] : 1e300;
            mx[a] = vv ? p[a] : -1e300;
            for (int s = 1; s < seg; s <<= 1) {   // xor offsets below seg stay inside the segment
                mn[a] = fmin(mn[a], __shfl_xor(mn[a], s));
                mx[a] = fmax(mx[a], __shfl_xor(mx[a], s));
            }
        }
        int ax = 0;
        for (int a = 1; a < dim; ++a)
            if (mx[a] - mn[a] > mx[ax] - mn[ax]) ax = a;
        const double span = mx[ax] - mn[ax];
        const float t = span > 0.0 ? (float)((p[ax] - mn[ax]) / span) : 0.f;
        float key = vv ? (float)(2 * (l / seg)) + t : 3e38f;   // segment s keeps keys in [2s, 2s + 1]
        int src = l;
        wave_sort64(key, src);
        for (int a = 0; a < 3; ++a) p[a] = __shfl(p[a], src);
        o = __shfl(o, src);
    }
}

__global__ void __launch_bounds__(256) k_build_tiles(const double* __restrict__ xyz_in, int dim,
                                                      int32_t* __restrict__ perm, TileInfo* tiles, TileBox* boxes,
                                                      int ntiles, PointRec* rec, float4* rel32, int32_t* inv,
                                                      unsigned* rho_bits) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int T = blockIdx.x * kWavesPerWG + w;
    if (T >= ntiles) return;
    const int start = tiles[T].start, count = tiles[T].count;
    const bool v = l < count;
    const int i = start + l;
    double p[3] = {0, 0, 0};
    int o = 0;
    if (v) {
        o = perm[i];
        for (int a = 0; a < dim; ++a) p[a] = xyz_in[(int64_t)o * dim + a];
    }
    split_order(p, o, dim, v);   // valid rows stay in lanes 0 .. count-1
    if (v) {
        perm[i] = o;
        inv[o] = i;
        // the point's record: its position, and m marked "not computed" until k_knn_cov writes it (a sharded
        // build computes the covariances of its own tiles only, gicp_get_covariances reads the others as NaN)
        const double nc = __longlong_as_double((long long)kRecNotComputed);
        double2* const r2 = reinterpret_cast<double2*>(rec + i);
        r2[0] = make_double2(p[0], p[1]);
        r2[1] = make_double2(p[2], nc);
        r2[2] = make_double2(nc, nc);
    }
    double c[3];
    for (int a = 0; a < 3; ++a) {
        const double mn = wave_mind(v ? p[a] : 1e300);
        const double mx = wave_maxd(v ? p[a] : -1e300);
        c[a] = a < dim ? 0.5 * (mn + mx) : 0.0;
    }
    float r[3];
    for (int a = 0; a < 3; ++a) r[a] = v ? (float)(p[a] - c[a]) : 0.0f;
    if (v) rel32[i] = make_float4(r[0], r[1], r[2], 0.0f);
    float h[3];
    for (int a = 0; a < 3; ++a) h[a] = wave_maxf(fabsf(r[a]));
    const float rad = wave_maxf(sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
    // sub-tile boxes (min/max over each kSubRows-lane segment of the wave)
    float smn[3], smx[3];
    for (int a = 0; a < 3; ++a) {
        smn[a] = v ? r[a] : 3e38f;
        smx[a] = v ? r[a] : -3e38f;
        for (int o = 1; o < kSubRows; o <<= 1) {
            smn[a] = fminf(smn[a], __shfl_xor(smn[a], o));
            smx[a] = fmaxf(smx[a], __shfl_xor(smx[a], o));
        }
    }
    if (l % kSubRows == 0) {
        const int g = l / kSubRows;
        TileInfo& t = tiles[T];
        for (int a = 0; a < 3; ++a) {
            const bool empty = smn[a] > smx[a];
            const float cc = empty ? 0.f : 0.5f * (smn[a] + smx[a]);
            // half-extent rounded up so the box covers both extremes exactly
            const float hh = empty ? -1e30f : fmaxf(smx[a] - cc, cc - smn[a]) * (1.0f + 2.4e-7f);
            t.sc[a][g] = cc;
            t.sh[a][g] = hh;
        }
    }
    if (l == 0) {
        TileInfo& t = tiles[T];
        for (int a = 0; a < 3; ++a) {
            t.c[a] = c[a];
            t.h[a] = h[a];
        }
        t.radius = rad;
        TileBox& b = boxes[T];
        for (int a = 0; a < 3; ++a) {
            b.c[a] = c[a];
            b.h[a] = h[a];
        }
        b.start = start;
        b.count = count;
        b.pad = 0;
        atomicMax(rho_bits, __float_as_uint(rad));
    }
}

// One wave per block of 64 tiles: fp64 AABB over the tiles' boxes.
// One level of the box hierarchy: box B covers children [64 B, 64 B + 64) of the level below
// (tiles -> blocks; blocks -> super-blocks, stored after the blocks in the same array).
template <class Child>
__global__ void __launch_bounds__(256) k_build_blocks(const Child* __restrict__ kids, int nkids, BlockInfo* blocks,
                                                       int nblocks, int dim) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int B = blockIdx.x * kWavesPerWG + w;
    if (B >= nblocks) return;
    const int t = B * kBlockTiles + l;
    const bool v = t < nkids;
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = v ? kids[t].c[a] - (double)kids[t].h[a] : 1e300;
        hi[a] = v ? kids[t].c[a] + (double)kids[t].h[a] : -1e300;
        lo[a] = wave_mind(lo[a]);
        hi[a] = wave_maxd(hi[a]);
    }
    if (l == 0) {
        BlockInfo& b = blocks[B];
        for (int a = 0; a < 3; ++a) {
            const double c = a < dim ? 0.5 * (lo[a] + hi[a]) : 0.0;
            const double hh = a < dim ? 0.5 * (hi[a] - lo[a]) : 0.0;
            b.c[a] = c;
            b.h[a] = __double2float_ru(hh) * (1.0f + 1e-6f);
        }
        b.first = B * kBlockTiles;
        b.ntiles = min(kBlockTiles, nkids - B * kBlockTiles);
        b.pad = 0.f;
    }
}

// reset_tile_state's per-source-tile and per-point resets in one launch
// pose0: slot 0 of the pose ring.  Pass ids restart at 1, so the first pass's "displacement over the last pass"
// (k_corr disp_since(pass - 1)) reads slot 0, which no pass since the reset has written: it is zeroed here, what a
// fresh allocation holds, so that the first lists' skin does not depend on what the memory held before.
__global__ void __launch_bounds__(256) k_reset_tiles(int32_t* hint, int32_t* list_len, float* list_rcert,
                                                     int32_t* cert_pass, int nt, int32_t* cert_j, int64_t n, double* pose0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && pose0)
        for (int k = 0; k < 12; ++k) pose0[k] = 0.0;
    if (i < nt) {
        hint[i] = -1;
        list_len[i] = 0;
        list_rcert[i] = 0.f;
        if (cert_pass) cert_pass[i] = -1;
    }
    if (i < n) cert_j[i] = -1;
}

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------
hipError_t launch_morton(const double* xyz, int64_t n, int dim, const DevCloud& fr, uint32_t* codes, int32_t* idx,
                         hipStream_t st) {
    clear_foreign_error();
    hipLaunchKernelGGL(k_morton, dim3(grid256(n)), dim3(256), 0, st, xyz, n, dim, fr, codes, idx);
    return hipGetLastError();
}

hipError_t launch_build_tiles(const double* xyz_in, int dim, int32_t* perm, TileInfo* tiles, TileBox* boxes,
                              int ntiles, PointRec* rec, float4* rel32, int32_t* inv, unsigned* rho_bits,
                              hipStream_t st) {
    clear_foreign_error();
    const unsigned g = (unsigned)((ntiles + kWavesPerWG - 1) / kWavesPerWG);
    hipLaunchKernelGGL(k_build_tiles, dim3(g), dim3(256), 0, st, xyz_in, dim, perm, tiles, boxes, ntiles, rec,
                       rel32, inv, rho_bits);
    return hipGetLastError();
}

hipError_t launch_build_blocks(const TileInfo* tiles, int ntiles, BlockInfo* blocks, int nblocks, int dim,
                               hipStream_t st) {
    clear_foreign_error();
    const unsigned g = (unsigned)((nblocks + kWavesPerWG - 1) / kWavesPerWG);
    hipLaunchKernelGGL(k_build_blocks<TileInfo>, dim3(g), dim3(256), 0, st, tiles, ntiles, blocks, nblocks, dim);
    const int nsuper = (nblocks + kBlockTiles - 1) / kBlockTiles;   // super-blocks at blocks[nblocks..]
    const unsigned g2 = (unsigned)((nsuper + kWavesPerWG - 1) / kWavesPerWG);
    hipLaunchKernelGGL(k_build_blocks<BlockInfo>, dim3(g2), dim3(256), 0, st, (const BlockInfo*)blocks, nblocks,
                       blocks + nblocks, nsuper, dim);
    return hipGetLastError();
}

hipError_t launch_reset_tiles(int32_t* hint, int32_t* list_len, float* list_rcert, int32_t* cert_pass, int nt,
                              int32_t* cert_j, int64_t n, double* pose0, hipStream_t st) {
    clear_foreign_error();
    const int64_t m = std::max<int64_t>(nt, n);
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reset_tiles, dim3(grid256(m)), dim3(256), 0, st, hint, list_len, list_rcert,
                       cert_pass, nt, cert_j, n, pose0);
    return hipGetLastError();
}

}  // namespace gicp
