// gicp_stats_dev.h — the layout of the sufficient statistics of loss() / grad_loss() (gicp.py:52-76, DESIGN.md
// §4), stated twice and checked against each other at compile time: stat_slot maps an entry (p, q) of the
// product u v^T to its statistic (k_corr's statistics GEMM, gicp_corr.hip), stat_terms maps a statistic to its
// (u, v) terms (k_batch_align's sums, gicp_batch.hip).  constexpr functions and data only.
#pragma once
#include <stdint.h>

#include "gicp_internal.h"

namespace gicp {

template <int D>
struct StatIdx {
    static constexpr int NS = D * (D + 1) / 2;
    static constexpr int pa(int p) { return D == 3 ? (p < 3 ? 0 : (p < 5 ? 1 : 2)) : (p < 2 ? 0 : 1); }
    static constexpr int pb(int p) {
        return D == 3 ? (p == 0 ? 0 : p == 1 ? 1 : p == 2 ? 2 : p == 3 ? 1 : 2) : (p == 0 ? 0 : 1);
    }
};

// Where entry (p, q) of the statistics GEMM's 16x16 product u v^T goes in the statistics vector (DESIGN.md
// §4), or kNoSlot: most of the product is not a statistic.  Each statistic has exactly one (p, q).
constexpr int kNoSlot = 0xFF;
template <int D>
constexpr int stat_slot(int p, int q) {
    constexpr int NS = D * (D + 1) / 2;
    constexpr int oB = NS * NS, oC = oB + NS * D, oR = oC + NS, oT = oR + D * D, o0 = oT + D;
    if (p < NS) {
        if (q < NS) return p * NS + q;                       // A[ab][ij]
        if (q < NS + D) return oB + p * D + (q - NS);        // B[ab][i]
        if (q == NS + D) return oC + p;                      // C[ab]
    } else if (p < NS + D) {
        if (q >= NS && q < NS + D) return oR + (p - NS) * D + (q - NS);   // gR[a][i]
        if (q == NS + D) return oT + (p - NS);                            // gt[a]
    } else if (q == NS + D) {
        if (p <= NS + D + 1) return o0 + (p - NS - D);       // c0, count
        if (p == NS + D + 2) return nstat(D) + 3;            // sum |r|^2 (extended slot)
    }
    return kNoSlot;
}
// Lane l of v_mfma_f64_16x16x4_f64 holds product entries (p = (l >> 4) + 4 j, q = l & 15), j = 0..3: their
// slots, one byte each (byte j), as one dword per lane
template <int D>
struct StatSlots {
    uint32_t lane[64];
    constexpr StatSlots() : lane{} {
        for (int l = 0; l < 64; ++l) {
            uint32_t w = 0;
            for (int j = 0; j < 4; ++j) w |= (uint32_t)stat_slot<D>((l >> 4) + 4 * j, l & 15) << (8 * j);
            lane[l] = w;
        }
    }
};
static_assert(nstat_ext(3) <= kNoSlot && nstat_ext(2) <= kNoSlot, "a statistic's slot fits a byte");
// every statistic, and the extended sum |r|^2, has one owner among the 256 entries; no other slot is written
template <int D>
constexpr bool stat_slots_one_owner() {
    int owners[kNoSlot] = {};
    for (int p = 0; p < 16; ++p)
        for (int q = 0; q < 16; ++q)
            if (stat_slot<D>(p, q) != kNoSlot) ++owners[stat_slot<D>(p, q)];
    for (int k = 0; k < kNoSlot; ++k)
        if (owners[k] != ((k < nstat(D) || k == nstat(D) + 3) ? 1 : 0)) return false;
    return true;
}
static_assert(stat_slots_one_owner<2>() && stat_slots_one_owner<3>(), "one owner lane per statistic");

// The same layout read the other way: which u term (row p) and v term (column q) statistic k is the product of
// (A[ab][ij], B[ab][i], C[ab], gR[a][i], gt[a], c0, count; k = nstat(D): the sum of |r|^2)
template <int D>
constexpr void stat_terms(int k, int& iu, int& iv) {
    constexpr int NS = D * (D + 1) / 2;
    iv = NS + D;   // the 1
    if (k < NS * NS) {
        iu = k / NS;
        iv = k % NS;
        return;
    }
    k -= NS * NS;
    if (k < NS * D) {
        iu = k / D;
        iv = NS + k % D;
        return;
    }
    k -= NS * D;
    if (k < NS) {
        iu = k;
        return;
    }
    k -= NS;
    if (k < D * D) {
        iu = NS + k / D;
        iv = NS + k % D;
        return;
    }
    k -= D * D;
    iu = NS + k;   // gt[a], then c0, the count, the sum of |r|^2
}
// the two statements of the layout agree: statistic k's terms own slot k (the sum of |r|^2: the extended slot)
template <int D>
constexpr bool stat_terms_match_slots() {
    for (int k = 0; k <= nstat(D); ++k) {
        int iu = 0, iv = 0;
        stat_terms<D>(k, iu, iv);
        if (stat_slot<D>(iu, iv) != (k < nstat(D) ? k : nstat(D) + 3)) return false;
    }
    return true;
}
static_assert(stat_terms_match_slots<2>() && stat_terms_match_slots<3>(), "stat_terms and stat_slot state one layout");

}  // namespace gicp
