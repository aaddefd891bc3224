// gicp_knn.hip — exact k-nearest-neighbour queries against an indexed cloud on the MI355X (gfx950), DESIGN.md §3r.
//
// The reference has no counterpart of its own: it asks a KD-tree (gicp.py:19-20, gicp.py:126-127).  This is that
// question for the caller, answered from the index k_knn_cov and k_corr search, with their traversal
// (gicp_search_dev.h) and their screen helpers (gicp_wave_dev.h).  The contract (include/gicp_hip.h): fp64
// d2 with every operation rounded on its own, rows ordered by (d2, original index), the first k of them.
#include <hip/hip_runtime.h>

#include "gicp_filter.h"   // filter_d2: the contract's d2 with contraction off, the function the host yardstick calls
#include "gicp_internal.h"
#include "gicp_search_dev.h"
#include "gicp_wave_dev.h"

namespace gicp {

// A wave's exact lists: entry m of lane l at [m][l] (lane-minor: a lane's walk over its own list touches one bank
// column, 64 lanes 64 consecutive words), d2 and the original index apart, 12 B per entry.
template <int K>
struct KnnList {
    double d2[K][kWave];
    int32_t idx[K][kWave];
};

// One wave = one query tile of <= 64 Morton-coherent queries, one per lane; four independent waves per workgroup.
//   phase 1  fp32 screen: the lane keeps the K smallest packed (d2 | row) keys (k_knn_cov's umed3 chain) and the
//            wave's bound shrinks with them.  Of the K keys the k-th bounds the k-th true distance: at least k rows
//            screen below the top of its truncation bucket s, so their true d2 <= B = s + 8 marg(s) (Margin is
//            stated in the true d2; solving it for d2 given the screened value costs at most a^2 + 2 marg(s)
//            <= 6 marg(s)).
//   phase 2  exact: every row a lane screens within B + 2 marg(B) -- a superset of the rows with true d2 <= B,
//            hence of the answer -- gets the contract's d2 in fp64 and its original index, and goes into the lane's list,
//            ordered by (d2, original index) and never longer than k.  The screen only picks candidates (a bit per
//            row of the staged tile); each lane then walks its own candidates, so a lane's fp64 work is its own
//            candidate count, not the wave's.  Every entry emitted is exact: there is no ambiguous-lane path.
// A lane that found fewer than k keys (a small database, a tight max_distance) takes the whole limit as B.
template <int D, int K>
__global__ void __launch_bounds__(256) k_knn_query(KnnArgs A) {
    __shared__ WaveLds s_lds[kWavesPerWG];
    __shared__ KnnList<K> s_list[kWavesPerWG];   // (K = 1 keeps its one entry in registers: not referenced, not allocated)
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    WaveLds& L = s_lds[w];
    const DevCloud& db = A.db;
    TileInfo qt;
    Query<D> q, qb;
    int i = 0;
    const int T = split_query<D>(A.qc, 0, A.qc.ntiles, 1, 1, 0, qt, q, qb, i);
    if (T < 0) return;  // waves are independent (no workgroup barrier here)
    const int k = A.k;

    // seed tile: the wave's own (self-query), else the database tile of the query tile centre's Morton code
    int seed = T;
    if (!A.self) {
        const uint32_t code = morton_code(q.ow, D, db.lo, db.scale, db.bits);
        const uint32_t b = code >> db.seed_shift;
        int lo = db.seed_tab[b], hi = db.seed_tab[b + 1];
        while (lo < hi) {  // last tile whose first code <= code
            const int mid = (lo + hi + 1) >> 1;
            if (db.tile_code[mid] <= code) lo = mid;
            else hi = mid - 1;
        }
        seed = __builtin_amdgcn_readfirstlane(lo);
    }

    // ---- phase 1: fp32 screen for the K smallest keys ------------------------
    // keys start at the limit; without one at the largest finite fp32 (a screened d2 beyond it, an overflow, is
    // never listed: such a lane stays short of k keys and phase 2 takes every row for it)
    const bool limited = A.search2 < 3.0e38f;
    const unsigned init = __float_as_uint(limited ? A.search2 : 3.0e38f) | 63u;
    unsigned lk[K];
#pragma unroll
    for (int m = 0; m < K; ++m) lk[m] = init;
    auto lane_bound = [&]() -> float {
        if (!q.valid) return -1.f;
        return lk[K - 1] >= init ? A.search2 : key_d2(lk[K - 1]);
    };
    auto visit1 = [&](int Tt) -> bool {
        const TileInfo ti = tile_meta(db, Tt);
        float pr[D];
        const bool need = lane_gap2<D>(q, ti, pr) <= lane_bound();
        if (!__any(need)) return false;
        // sub-tiles beyond the top of the truncation bucket of the lane's last key hold no row the list would take
        const float top = lk[K - 1] >= init ? A.search2 : __uint_as_float((lk[K - 1] | 63u) + 1u);
        const unsigned sub = sub_mask<D>(ti, pr, q.valid, top);
        stage_f32(db, ti, L);
        scan_tile<D>(L, ti.count, pr, [&](unsigned key, int) {
            if (__any(key < lk[K - 1])) {
#pragma unroll
                for (int m = K - 1; m > 0; --m) lk[m] = umed3(lk[m - 1], lk[m], key);
                lk[0] = min(lk[0], key);
            }
        }, sub);
        wave_sync();
        return true;
    };
    traverse<D>(db, qb, seed, visit1, [&]() { return wave_maxf(lane_bound()); });

    // ---- the exact phase's bound: from the k-th key ---------------------------
    unsigned kth = lk[0];
#pragma unroll
    for (int m = 1; m < K; ++m)
        if (m == k - 1) kth = lk[m];
    float thr = A.search2;            // screened d2 of every row that can be in the answer
    unsigned tau = limited ? init : 0xFFFFFFFFu;
    if (kth < init) {
        const float s = __uint_as_float((kth | 63u) + 1u);
        const float B = fmaf(8.f, marg(A.mg, s), s) * 1.000001f;
        const float t2 = fmaf(2.f, marg(A.mg, B), B) * 1.000001f;
        if (t2 < thr) {
            thr = t2;
            tau = __float_as_uint(t2) | 63u;
        }
    }
    const float b2 = q.valid ? thr : -1.f;

    // ---- phase 2: exact (d2, original index) lists -----------------------------
    int cnt = 0;
    double wd2 = 0.0;   // the list's last entry once it holds k (cnt == k)
    int widx = 0;
    auto offer = [&](double d2, int og) {
        if (!(d2 <= A.maxd2)) return;
        if (cnt == k && !(d2 < wd2 || (d2 == wd2 && og < widx))) return;
        if constexpr (K == 1) {
            wd2 = d2;
            widx = og;
            cnt = 1;
        } else {
            KnnList<K>& S = s_list[w];
            int m = cnt < k ? cnt : k - 1;   // the slot that opens: a new last one, or the dropped last entry's
            while (m > 0) {
                const double pd = S.d2[m - 1][l];
                const int pi = S.idx[m - 1][l];
                if (!(d2 < pd || (d2 == pd && og < pi))) break;
                S.d2[m][l] = pd;
                S.idx[m][l] = pi;
                --m;
            }
            S.d2[m][l] = d2;
            S.idx[m][l] = og;
            if (cnt < k) ++cnt;
            if (cnt == k) {
                wd2 = S.d2[k - 1][l];
                widx = S.idx[k - 1][l];
            }
        }
    };
    auto visit2 = [&](int Tt) -> bool {
        const TileInfo ti = tile_meta(db, Tt);
        float pr[D];
        const bool need = lane_gap2<D>(q, ti, pr) <= b2;
        if (!__any(need)) return false;
        const unsigned sub = sub_mask<D>(ti, pr, q.valid, b2);
        stage_f32(db, ti, L);
        stage_f64(db, ti, L);
        if (l < ti.count) L.t.perm[l] = db.perm[ti.start + l];
        wave_sync();
        unsigned long long cand = 0;   // the staged rows this lane screens within its bound
        scan_tile<D>(L, ti.count, pr, [&](unsigned key, int j) {
            if (key <= tau) cand |= 1ull << j;
        }, sub);
        cand &= ti.count >= kTile ? ~0ull : (1ull << ti.count) - 1ull;   // (padding rows of the last row group)
        if (!q.valid) cand = 0;
        while (wave_any(cand != 0)) {
            if (cand) {
                const int j = __ffsll(cand) - 1;
                cand &= cand - 1;
                const double qq[3] = {L.t.x64[j], L.t.y64[j], L.t.z64[j]};
                // (not dist2_exact: its products and sums are plain operators under the compiler's default
                // contraction, and a fused dx * dx + dy * dy moves d2 by an ulp, which is fine for an order but not
                // for the bits the contract returns)
                offer(filter_d2<D>(qq, q.p64), L.t.perm[j]);
            }
        }
        wave_sync();
        return true;
    };
    traverse<D>(db, qb, seed, visit2, [&]() { return wave_maxf(b2); });

    // ---- the caller's rows: original query order through the query set's perm ---
    if (q.valid) {
        const int64_t o = A.qc.perm[i];
        const double inf = __longlong_as_double(0x7FF0000000000000ll);
        for (int m = 0; m < k; ++m) {
            double d2 = inf;
            int64_t id = -1;
            if (m < cnt) {
                if constexpr (K == 1) {
                    d2 = wd2;
                    id = widx;
                } else {
                    d2 = s_list[w].d2[m][l];
                    id = s_list[w].idx[m][l];
                }
            }
            A.dist2[o * k + m] = d2;
            A.index[o * k + m] = id;
        }
        A.count[o] = cnt;
    }
}

// ---------------------------------------------------------------------------
// host-side launcher
// ---------------------------------------------------------------------------
// the instantiation that serves k: the smallest K >= k of 1, 8, 16, 32 (its first k entries are emitted)
hipError_t launch_knn_query(const KnnArgs& a, hipStream_t st) {
    clear_foreign_error();
    if (a.qc.ntiles <= 0) return hipSuccess;
    if (a.k < 1 || a.k > kKnnMaxK || a.qc.dim != a.db.dim) return hipErrorInvalidValue;
    const unsigned g = (unsigned)((a.qc.ntiles + kWavesPerWG - 1) / kWavesPerWG);
    const int dim = a.db.dim;
#define GICP_KNNQ(DD, KK)                                                                 \
    if (dim == DD && a.k <= KK) {                                                         \
        hipLaunchKernelGGL((k_knn_query<DD, KK>), dim3(g), dim3(256), 0, st, a);          \
        return hipGetLastError();                                                         \
    }
    GICP_KNNQ(2, 1)
    GICP_KNNQ(2, 8)
    GICP_KNNQ(2, 16)
    GICP_KNNQ(2, 32)
    GICP_KNNQ(3, 1)
    GICP_KNNQ(3, 8)
    GICP_KNNQ(3, 16)
    GICP_KNNQ(3, 32)
#undef GICP_KNNQ
    return hipErrorInvalidValue;
}

}  // namespace gicp
