// gicp_search_dev.h — the query and traversal machinery shared by k_knn_cov (gicp_cov.hip) and k_corr
// (gicp_corr.hip): the wave's query, the culled walks over the box hierarchy, the per-wave LDS image and the
// fp32 row scan.  It answers for the neighbour searches of the reference: the k nearest of
// compute_covariance_matrix (gicp.py:19-20) and the nearest target of the outer loop (gicp.py:126-127).
//
// Design: one wave = one query tile of <= 64 Morton-coherent points.
// Database tiles are culled with a three-level AABB hierarchy (super-blocks of 64 blocks of 64 tiles, tested
// one per lane, ballot), staged through LDS as fp32 SoA and scanned with a
// broadcast read; lanes keep packed (d2 | row) keys.  The fp32 screen carries an
// explicit error bound: a lane whose winner is within that bound of a rival (or of
// the d_n / d_c cut) is re-resolved exactly in fp64, so indices match an fp64
// KD-tree exactly.  No MFMA: there is no dense contraction in this path.
// Device code only: types, __device__ __forceinline__ functions and templates; the kernels declare the LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "gicp_internal.h"
#include "gicp_wave_dev.h"

namespace gicp {

// the Morton code k_morton sorts a cloud by; k_corr codes a query with it to find its seed tile
__device__ __forceinline__ uint32_t spread2(uint32_t x) {
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
__device__ __forceinline__ uint32_t spread3(uint32_t x) {
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
__device__ __forceinline__ uint32_t morton_code(const double* p, int dim, const double* lo, double scale, int bits) {
    const double maxc = (double)((1u << bits) - 1u);
    uint32_t q[3] = {0, 0, 0};
    for (int a = 0; a < dim; ++a) {
        double v = (p[a] - lo[a]) * scale;
        v = fmin(fmax(v, 0.0), maxc);
        q[a] = (uint32_t)v;
    }
    return dim == 3 ? (spread3(q[0]) | (spread3(q[1]) << 1) | (spread3(q[2]) << 2))
                    : (spread2(q[0]) | (spread2(q[1]) << 1));
}

// ---------------------------------------------------------------------------
// traversal
// ---------------------------------------------------------------------------
template <int D>
struct Query {
    double ow[D];   // wave origin (query tile centre, transformed), uniform
    float ew[D];    // half-extents of the query tile around ow, uniform, conservative
    float pw[D];    // lane point relative to ow, fp32
    double p64[D];  // lane point, fp64 (transformed)
    bool valid;
};

// squared gap between the wave box (ow +- ew) and a box (c +- h); conservative in fp32
template <int D>
__device__ __forceinline__ float gap2_box(const Query<D>& q, const double* c, const float* h) {
    float g2 = 0.f;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float dl = fabsf((float)(q.ow[a] - c[a]));
        float g = dl - q.ew[a] - h[a];
        g -= (dl + q.ew[a] + h[a]) * 9.5367431640625e-7f;  // 2^-20 slack
        g = fmaxf(g, 0.f);
        g2 = fmaf(g, g, g2);
    }
    return g2;
}

// The query box of the lanes where `on` holds (the wave's lanes still searching): their fp32 offsets
// pw lie within ow' +- ew' (conservative: the centre is rounded, the half-extent padded).  A list
// walk or fallback tests candidate tiles against it instead of the whole source tile's box, so a
// wave with a few searching lanes visits only the tiles near them (the list, built for the whole
// box, covers any subset of its lanes).  Values are shifted by 2 ew (>= |pw|) to use the
// non-negative wave max; lanes with on = false pass the negative marker.
template <int D>
__device__ __forceinline__ Query<D> active_box(const Query<D>& q, bool on) {
    Query<D> qa = q;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const float B = 2.f * q.ew[a] + 1e-30f;
        const float hi = wave_maxf(on ? q.pw[a] + B : -1.f) - B;
        const float lo = B - wave_maxf(on ? B - q.pw[a] : -1.f);
        const float mid = 0.5f * (lo + hi);
        qa.ow[a] = q.ow[a] + (double)mid;
        qa.ew[a] = 0.5f * (hi - lo) + 4.8e-7f * (fabsf(lo) + fabsf(hi) + B) + 1e-30f;
    }
    return qa;
}

// Two-level culled walk over the database tiles.  `visit(T)` returns true when it
// processed the tile (the wave's bound then shrinks); `wave_bound()` is the max over
// lanes of the squared search radius still needed.
// With skin > 0 every tile whose box lies within sqrt(wb) + skin of the wave box is also passed
// to collect(T) (wb as it stands when the tile is tested; wb only shrinks, so at the end the
// collected set holds every tile within sqrt(wb_final) + skin).
struct NoCount {
    __device__ __forceinline__ void count(int, unsigned = 1) {}
};
template <int D, class Visit, class WB, class Collect, class Cnt = NoCount>
__device__ __forceinline__ void traverse_c(const DevCloud& db, const Query<D>& q, int seed, Visit&& visit,
                                           WB&& wave_bound, float skin, Collect&& collect, Cnt* cnt = nullptr) {
    const int l = lane_id();
    auto infl = [&](float w) -> float {
        if (skin <= 0.f || w < 0.f) return w;
        const float r = __builtin_amdgcn_sqrtf(w) * 1.0001f + skin;
        return r * r;
    };
    float wb = wave_bound();
    float wbi = infl(wb);
    if (seed >= 0) {
        collect(seed);
        if (visit(seed)) {
            wb = wave_bound();
            wbi = infl(wb);
        }
    }
    // super-blocks (64 blocks each, stored after the blocks): a round of 64 block tests is one
    // super-block, skipped whole when its box (scalar loads, uniform test) is out of reach.  It contains
    // its blocks' boxes, so the visited tiles and their order are unchanged.
    typedef __attribute__((address_space(4))) const BlockInfo* ConstBlocks;
    const ConstBlocks cb0 = (ConstBlocks)(uintptr_t)db.blocks + db.nblocks;
    for (int b0 = 0; b0 < db.nblocks; b0 += kWave) {
        {
            const ConstBlocks sb = cb0 + (b0 / kWave);
            const double c[3] = {sb->c[0], sb->c[1], sb->c[2]};
            const float h[3] = {sb->h[0], sb->h[1], sb->h[2]};
            if (!__builtin_amdgcn_readfirstlane((int)(gap2_box<D>(q, c, h) <= wbi))) continue;   // uniform
        }
        if (cnt) cnt->count(5);
        const int b = b0 + l;
        bool cb = false;
        if (b < db.nblocks) cb = gap2_box<D>(q, db.blocks[b].c, db.blocks[b].h) <= wbi;
        uint64_t bm = __ballot(cb);
        while (bm) {
            const int bb = b0 + __ffsll((unsigned long long)bm) - 1;
            bm &= bm - 1;
            const int first = db.blocks[bb].first, nt = db.blocks[bb].ntiles;
            if (cnt) cnt->count(6);
            const int t = first + l;
            bool ct = false, cv = false;
            if (l < nt && t != seed) {
                const float g2 = gap2_box<D>(q, db.tiles[t].c, db.tiles[t].h);
                ct = g2 <= wbi;
                cv = g2 <= wb;
            }
            if (skin > 0.f) {
                uint64_t cm = __ballot(ct);
                while (cm) {
                    collect(first + __ffsll((unsigned long long)cm) - 1);
                    cm &= cm - 1;
                }
            }
            uint64_t tm = __ballot(cv);
            while (tm) {
                const int T = first + __ffsll((unsigned long long)tm) - 1;
                tm &= tm - 1;
                if (visit(T)) {
                    wb = wave_bound();
                    wbi = infl(wb);
                }
            }
        }
    }
}

template <int D, class Visit, class WB>
__device__ __forceinline__ void traverse(const DevCloud& db, const Query<D>& q, int seed, Visit&& visit,
                                         WB&& wave_bound) {
    traverse_c<D>(db, q, seed, visit, wave_bound, 0.f, [](int) {});
}

// per-wave LDS: tile staging during the walk, statistics transpose afterwards (same bytes)
struct WaveStage {
    float x[kTile], y[kTile], z[kTile];           // fp32 screen coordinates, SoA
    double x64[kTile], y64[kTile], z64[kTile];    // fp64 coordinates (covariance sums, fallback)
    int32_t perm[kTile];                          // original indices (fallback tie-break)
};
// statistics transpose image of 32 points (half a wave): u[term][point] and v[term][point], rows padded
// to 33 doubles.  A term's 32 points are written by 32 lanes to consecutive words.  An MFMA operand read
// takes row l & 15 at column c + (l >> 4); the compiler pairs the reads of two MFMAs into ds_read2_b64
// (banks of 4 B modulo 32, conflicts within 16 consecutive lanes, which share l >> 4): rows r = 0..15 at
// doubles 33 r + const fall on the bank pairs 2 r + const, all distinct.  An even stride collides: 34 put
// rows r and r + 8 on one bank (SQ_LDS_BANK_CONFLICT 124 cycles per wave against 6 at 33 and at the former
// 17, profiles/epilogue/README.md); lone ds_read_b64 (modulo 64, 32-lane halves) would want 34 instead.
// Only the rows of terms in use are stored (12 u and 10 v terms in 3-D): the MFMA lanes of the unused
// rows read a duplicate of the last row, whose products land in output rows / columns nobody reads.
// 22 x 33 doubles (5808 B) per wave: two transposes per wave instead of four, at 22.7 KB of LDS per
// workgroup -- the six workgroups that 80 VGPRs allow on a CU take 136 of its 160 KiB.
constexpr int kStatRow = 33;
constexpr int kStatU = 12, kStatV = 10;
struct WaveStat {
    double u[kStatU * kStatRow];
    double v[kStatV * kStatRow];
};
union __attribute__((aligned(16))) WaveLds {
    WaveStage t;
    WaveStat st;
};

// Lane point relative to database tile T, and the per-lane squared gap to T's box.
template <int D>
__device__ __forceinline__ float lane_gap2(const Query<D>& q, const TileInfo& ti, float* pr) {
    float g2 = 0.f;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        pr[a] = q.pw[a] + (float)(q.ow[a] - ti.c[a]);
        const float ap = fabsf(pr[a]);
        float g = ap - ti.h[a] - (ap + ti.h[a]) * 9.5367431640625e-7f;
        g = fmaxf(g, 0.f);
        g2 = fmaf(g, g, g2);
    }
    return g2;
}

// uniform copy of a tile's metadata through the constant address space: scalar s_load_dwordx*
// into SGPRs (a generic pointer here compiles to ten vector loads + readfirstlane)
typedef __attribute__((address_space(4))) const TileInfo* ConstTiles;
__device__ __forceinline__ TileInfo tile_meta(const DevCloud& db, int T) {
    const ConstTiles ct = (ConstTiles)(uintptr_t)db.tiles + __builtin_amdgcn_readfirstlane(T);
    TileInfo t;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t.c[a] = ct->c[a];
        t.h[a] = ct->h[a];
    }
    t.start = ct->start;
    t.count = ct->count;
    t.radius = ct->radius;
#pragma unroll
    for (int g = 0; g < kSub; ++g)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            t.sc[a][g] = ct->sc[a][g];
            t.sh[a][g] = ct->sh[a][g];
        }
    return t;
}

// stage a tile's fp32 coordinates (padding rows at 1e30: their distance is +inf)
__device__ __forceinline__ void stage_f32(const DevCloud& db, const TileInfo& ti, WaveLds& L) {
    const int l = lane_id();
    float4 v = make_float4(1e30f, 1e30f, 1e30f, 0.f);
    if (l < ti.count) v = db.rel32[ti.start + l];
    L.t.x[l] = v.x;
    L.t.y[l] = v.y;
    L.t.z[l] = v.z;
    wave_sync();
}
__device__ __forceinline__ float4 load_rel(const DevCloud& db, int start, int count) {
    const int l = lane_id();
    float4 v = make_float4(1e30f, 1e30f, 1e30f, 0.f);
    if (l < count) v = db.rel32[start + l];
    return v;
}
__device__ __forceinline__ void stage_f32_from(const float4& v, WaveLds& L) {
    const int l = lane_id();
    L.t.x[l] = v.x;
    L.t.y[l] = v.y;
    L.t.z[l] = v.z;
    wave_sync();
}
// k_corr's full walk: traverse_c's order and culling, but each lane of a candidate block holds its
// tile's box gap and (start, count), so a candidate's coordinates are requested together with its
// metadata (visit_pre(T, &coords): one memory round trip per visited tile instead of two), and
// candidates the shrinking bound has put out of reach are dropped before they are visited (the test the
// block entry applied, repeated with the current bound; a tile it drops could not have been within
// any lane's bound).
template <int D, class VisitPre, class WB, class Collect, class Cnt = NoCount>
__device__ __forceinline__ void walk_c(const DevCloud& db, const Query<D>& q, int seed, VisitPre&& visit_pre,
                                       WB&& wave_bound, float skin, Collect&& collect, Cnt* cnt = nullptr) {
    const int l = lane_id();
    auto infl = [&](float w) -> float {
        if (skin <= 0.f || w < 0.f) return w;
        const float r = __builtin_amdgcn_sqrtf(w) * 1.0001f + skin;
        return r * r;
    };
    float wb = wave_bound();
    float wbi = infl(wb);
    if (seed >= 0) {
        collect(seed);
        if (visit_pre(seed, nullptr)) {
            wb = wave_bound();
            wbi = infl(wb);
        }
    }
    // super-blocks (64 blocks each, stored after the blocks): lane s tests super-block s0 + s, all of a
    // round of 64 requested at once (one memory round trip instead of one per super-block); a candidate
    // super-block's 64 blocks are tested by the lanes, a candidate block's 64 tiles likewise from the
    // compact TileBox records (block b's tiles are 64 b .. 64 b + 63).  Same tiles, same order as the
    // one-super-block-at-a-time walk.
    const int nsuper = (db.nblocks + kWave - 1) / kWave;
    for (int s0 = 0; s0 < nsuper; s0 += kWave) {
        float sg = 3e38f;
        if (s0 + l < nsuper) sg = gap2_box<D>(q, db.blocks[db.nblocks + s0 + l].c, db.blocks[db.nblocks + s0 + l].h);
        uint64_t sm = __ballot(sg <= wbi);
        while (sm) {
            const int sl = __ffsll((unsigned long long)sm) - 1;
            sm &= sm - 1;
            const int b0 = (s0 + sl) * kWave;
            if (cnt) cnt->count(5);
            const int b = b0 + l;
            bool cb = false;
            if (b < db.nblocks) cb = gap2_box<D>(q, db.blocks[b].c, db.blocks[b].h) <= wbi;
            uint64_t bm = __ballot(cb);
            while (bm) {
                const int bb = b0 + __ffsll((unsigned long long)bm) - 1;
                bm &= bm - 1;
                const int first = bb * kBlockTiles, nt = min(kBlockTiles, db.ntiles - first);
                if (cnt) cnt->count(6);
                const int t = first + l;
                bool ct = false;
                float g2 = 3e38f;
                int tst = 0, tcnt = 0;   // the tile's start, count
                if (l < nt && t != seed) {
                    const TileBox tb = db.boxes[t];
                    g2 = gap2_box<D>(q, tb.c, tb.h);
                    ct = g2 <= wbi;
                    tst = tb.start;
                    tcnt = tb.count;
                }
                if (skin > 0.f) {
                    uint64_t cm = __ballot(ct);
                    while (cm) {
                        collect(first + __ffsll((unsigned long long)cm) - 1);
                        cm &= cm - 1;
                    }
                }
                uint64_t tm = __ballot(g2 <= wb);
                auto pick = [&]() -> int { return tm ? __ffsll((unsigned long long)tm) - 1 : -1; };
                auto coords = [&](int kk) {
                    return load_rel(db, __builtin_amdgcn_readlane(tst, kk), __builtin_amdgcn_readlane(tcnt, kk));
                };
                for (int k = pick(); k >= 0; k = pick()) {
                    tm &= ~(1ull << k);
                    const float4 pv = coords(k);   // in flight with the tile's metadata load in visit_pre
                    if (visit_pre(first + k, &pv)) {
                        wb = wave_bound();
                        wbi = infl(wb);
                        tm &= __ballot(g2 <= wb);
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ void stage_f64(const DevCloud& db, const TileInfo& ti, WaveLds& L) {
    const int l = lane_id();
    RecPos v;
    v.x = v.y = v.z = 1e150;
    if (l < ti.count) v = rec_pos(db.rec + (ti.start + l));
    L.t.x64[l] = v.x;
    L.t.y64[l] = v.y;
    L.t.z64[l] = v.z;
    wave_sync();
}

typedef float f2v __attribute__((ext_vector_type(2)));

// squared screen distance of the lane point to two database rows at once (v_pk_* fp32);
// bit-identical to fmaf(dz, dz, fmaf(dy, dy, dx * dx)) per row
template <int D>
__device__ __forceinline__ f2v pair_d2(const float* pr, f2v qx, f2v qy, f2v qz) {
    const f2v dx = f2v{pr[0], pr[0]} - qx;
    const f2v dy = f2v{pr[1], pr[1]} - qy;
    f2v d2 = __builtin_elementwise_fma(dy, dy, dx * dx);
    if (D == 3) {
        const f2v dz = f2v{pr[2], pr[2]} - qz;
        d2 = __builtin_elementwise_fma(dz, dz, d2);
    }
    return d2;
}

// 0xFFFFFFC0 held in a VGPR so (d2 & mask) | row is one v_and_or_b32 (row stays an SGPR)
__device__ __forceinline__ unsigned key_mask() {
    unsigned m;
    asm volatile("v_mov_b32 %0, 0xffffffc0" : "=v"(m));
    return m;
}

// One group of 4 rows at compile-time offset J: 3 ds_read_b128 (SoA x/y/z), 2 packed pairs.
template <int J, int D, class Row>
__device__ __forceinline__ void scan_group(const WaveLds& L, const float* pr, unsigned M, Row& row) {
    const float4 X = *reinterpret_cast<const float4*>(L.t.x + J);
    const float4 Y = *reinterpret_cast<const float4*>(L.t.y + J);
    float4 Z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (D == 3) Z = *reinterpret_cast<const float4*>(L.t.z + J);
    const f2v a = pair_d2<D>(pr, f2v{X.x, X.y}, f2v{Y.x, Y.y}, f2v{Z.x, Z.y});
    const f2v b = pair_d2<D>(pr, f2v{X.z, X.w}, f2v{Y.z, Y.w}, f2v{Z.z, Z.w});
    row((__float_as_uint(a.x) & M) | (unsigned)J, J);
    row((__float_as_uint(a.y) & M) | (unsigned)(J + 1), J + 1);
    row((__float_as_uint(b.x) & M) | (unsigned)(J + 2), J + 2);
    row((__float_as_uint(b.y) & M) | (unsigned)(J + 3), J + 3);
}

template <int D, class Row, int... G>
__device__ __forceinline__ void scan_groups(const WaveLds& L, int n4, unsigned sub, const float* pr, unsigned M,
                                            Row& row, std::integer_sequence<int, G...>) {
    // short-circuit fold: group G runs only while 4G < n4; skipped when its sub-tile is not needed
    (void)((4 * G < n4 ? (((sub >> (4 * G / kSubRows)) & 1u) ? scan_group<4 * G, D>(L, pr, M, row) : void(), true) : false) &&
           ...);
}

// Per-lane squared gap to each sub-box of the staged tile; bit g of the result is set when
// some lane within its bound needs sub-tile g.  Same conservative slack as lane_gap2.
template <int D>
__device__ __forceinline__ unsigned sub_mask(const TileInfo& ti, const float* pr, bool valid, float bound) {
    unsigned m = 0;
#pragma unroll
    for (int g = 0; g < kSub; ++g) {
        if (kSubRows * g >= ti.count) break;
        float g2 = 0.f;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const float dl = fabsf(pr[a] - ti.sc[a][g]);
            float gg = dl - ti.sh[a][g] - (dl + ti.sh[a][g] + fabsf(pr[a])) * 9.5367431640625e-7f;
            gg = fmaxf(gg, 0.f);
            g2 = fmaf(gg, gg, g2);
        }
        if (__any(valid && g2 <= bound)) m |= 1u << g;
    }
    return m;
}

// k_corr's forms of lane_gap2 / sub_mask: no per-axis rounding slack; the caller compares against a
// bound inflated once by the launch-uniform slack S (CorrArgs::gap_slack: rounding of coordinates
// of magnitude <= sqrt(search2) + 2 rho_t, the only ones whose test can matter)
template <int D>
__device__ __forceinline__ float lane_gap2_ns(const Query<D>& q, const TileInfo& ti, float* pr) {
    float g2 = 0.f;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        pr[a] = q.pw[a] + (float)(q.ow[a] - ti.c[a]);
        const float g = fmaxf(fabsf(pr[a]) - ti.h[a], 0.f);
        g2 = fmaf(g, g, g2);
    }
    return g2;
}
template <int D>
__device__ __forceinline__ unsigned sub_mask_ns(const TileInfo& ti, const float* pr, float bound /* < 0: lane off */) {
    // two sub-boxes per packed op (sc/sh are axis-major, so boxes g and g+1 of an axis are adjacent):
    // g = max(max(d, -d) - sh, 0), g2 += g * g
    typedef float f2v __attribute__((ext_vector_type(2)));
    unsigned m = 0;
#pragma unroll
    for (int g = 0; g < kSub; g += 2) {
        if (kSubRows * g >= ti.count) break;
        f2v g2 = {0.f, 0.f};
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const f2v d = f2v{pr[a], pr[a]} - f2v{ti.sc[a][g], ti.sc[a][g + 1]};
            const f2v ad = __builtin_elementwise_max(d, -d);
            const f2v gg = __builtin_elementwise_max(ad - f2v{ti.sh[a][g], ti.sh[a][g + 1]}, f2v{0.f, 0.f});
            g2 = __builtin_elementwise_fma(gg, gg, g2);
        }
        if (wave_any(g2.x <= bound)) m |= 1u << g;
        if (kSubRows * (g + 1) < ti.count && wave_any(g2.y <= bound)) m |= 2u << g;
    }
    return m;
}

__device__ __forceinline__ int rows_scanned(unsigned sub, int count) {
    int r = 0;
#pragma unroll
    for (int g = 0; g < kSub; ++g)
        if ((sub >> g) & 1u) r += min(kSubRows, max(0, ((count + 3) & ~3) - kSubRows * g));
    return r;
}

// Scan one staged tile: row(key, j) for every row of the sub-tiles in `sub`; key = (d2 bits & ~63) | row.
template <int D, class Row>
__device__ __forceinline__ void scan_tile(const WaveLds& L, int count, const float* pr, Row&& row,
                                          unsigned sub = 0xFFFFFFFFu) {
    const unsigned M = key_mask();
    scan_groups<D>(L, (count + 3) & ~3, sub, pr, M, row, std::make_integer_sequence<int, kTile / 4>{});
}

// The wave's query for split build kernels: wave `wid` takes part g = wid % split of query tile
// T = first + wid / split.  Lanes keep their points relative to the tile centre (the screen's error model
// is unchanged); the culling box `qb` is the part's sub-box (centre c + sc, half-extents sh) when split.
// Returns the tile index, -1 if the wave has no rows.
template <int D>
__device__ __forceinline__ int split_query(const DevCloud& cl, int first, int last, int split, int sh_n, int sh_r,
                                          TileInfo& qt, Query<D>& q, Query<D>& qb, int& i) {
    const int wid = (int)blockIdx.x * kWavesPerWG + ((int)threadIdx.x >> 6), l = (int)threadIdx.x & 63;
    const int Tl = first + wid / split, g = wid % split;
    if (Tl >= last) return -1;
    constexpr int kChunkTiles = kShardChunk * kCorrWaves;   // tiles per shard chunk (k_corr's split)
    const int T = sh_n > 1 ? ((Tl / kChunkTiles) * sh_n + sh_r) * kChunkTiles + Tl % kChunkTiles : Tl;
    if (T >= cl.ntiles) return -1;
    qt = tile_meta(cl, T);
    const int rows = kTile / split, r0 = g * rows, r1 = min(qt.count, r0 + rows);
    if (r0 >= r1) return -1;
    q.valid = l < r1 - r0;
    i = qt.start + r0 + min(l, r1 - r0 - 1);
    const float4 rel = cl.rel32[i];
    const RecPos p4 = rec_pos(cl.rec + i);
    const float relv[3] = {rel.x, rel.y, rel.z};
    const double p4v[3] = {p4.x, p4.y, p4.z};
#pragma unroll
    for (int a = 0; a < D; ++a) {
        q.ow[a] = qt.c[a];
        q.ew[a] = qt.h[a];
        q.pw[a] = relv[a];
        q.p64[a] = p4v[a];
    }
    qb = q;
    if (split > 1) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
            qb.ow[a] = qt.c[a] + (double)qt.sc[a][g];
            qb.ew[a] = qt.sh[a][g] * (1.0f + 4.8e-7f) + 1e-30f;
        }
    }
    return T;
}

}  // namespace gicp
