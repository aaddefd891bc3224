// gicp_cov.hip — per-point surface covariances and the target's neighbour graph on the MI355X (gfx950).
//
// Reference behaviour (python-implementation/gicp.py):
//   k_knn_cov   <- compute_covariance_matrix / _single_point, gicp.py:5-35
//                  (k nearest incl. self, distance strictly < d_n, np.cov, eig ->
//                  surface-aligned covariance; identity for isolated points)
//   k_graph_pack   no counterpart: it packs the neighbour graph k_corr's descent reads
#include <hip/hip_runtime.h>

#include "gicp_cov_dev.h"
#include "gicp_internal.h"
#include "gicp_search_dev.h"
#include "gicp_wave_dev.h"

namespace gicp {

// G: the target's neighbour graph rows come out of the same two walks: phase 1 keeps the
// KL = max(K + 1, kGraphK + 2) smallest keys (the covariance uses the first K + 1, the graph all), phase 2
// visits every tile either needs and takes each row for the covariance sums (key <= tau) and / or the
// graph row (key <= tau_g).  Tiles are visited in the same order whatever the bound, so the sums and rows
// are those of separate walks, bit for bit.
template <int D, int K, bool G>
__global__ void __launch_bounds__(256) k_knn_cov(CovArgs A) {
    __shared__ WaveLds s_lds[kWavesPerWG];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    WaveLds& L = s_lds[w];
    const DevCloud& cl = A.cl;
    TileInfo qt;
    Query<D> q, qb;
    int i = 0;
    const int T = split_query<D>(cl, A.q_begin, A.q_end, A.split, A.sh_n, A.sh_r, qt, q, qb, i);
    if (T < 0) return;  // waves are independent (no workgroup barrier here)

    // ---- phase 1: fp32 screen for the K+1 smallest keys ------------------
    constexpr int K1 = K + 1, KG = kGraphK, KL = G ? (K1 > KG + 2 ? K1 : KG + 2) : K1;
    const unsigned init = __float_as_uint(A.search2) | 63u;
    unsigned lk[KL];
#pragma unroll
    for (int m = 0; m < KL; ++m) lk[m] = init;
    auto lane_bound = [&]() -> float {
        if (!q.valid) return -1.f;
        if (G) return key_d2(lk[KL - 1]);   // >= the covariance's own bound below
        const float kk = key_d2(lk[K1 - 1]), km = key_d2(lk[K1 - 2]);
        return fminf(kk, km + 2.f * marg(A.mg, km));
    };
    auto visit1 = [&](int Tt) -> bool {
        const TileInfo ti = tile_meta(cl, Tt);
        float pr[D];
        const bool need = lane_gap2<D>(q, ti, pr) <= lane_bound();
        if (!__any(need)) return false;
        // sub-tiles beyond the top of the truncation bucket of each lane's last list key hold no row the
        // list would take (a key below it screens at most at that bucket's top)
        const unsigned sub = sub_mask<D>(ti, pr, q.valid, __uint_as_float((lk[KL - 1] | 63u) + 1u));
        stage_f32(cl, ti, L);
        scan_tile<D>(L, ti.count, pr, [&](unsigned key, int) {
            if (__any(key < lk[KL - 1])) {
#pragma unroll
                for (int m = KL - 1; m > 0; --m) lk[m] = umed3(lk[m - 1], lk[m], key);
                lk[0] = min(lk[0], key);
            }
        }, sub);
        wave_sync();
        return true;
    };
    traverse<D>(cl, qb, T, visit1, [&]() { return wave_maxf(lane_bound()); });

    // graph: rows keyed <= tau_g (the (kGraphK + 1)-th key, self excluded from the row) and the radius the
    // row certifies (k_graph's rules: from the (kGraphK + 2)-th key, or the screen radius)
    unsigned tau_g = 0;
    float r2g = 0.f, tau_g_hi = -1.f;
    if constexpr (G) {
        tau_g = lk[KG];
        if (lk[KG + 1] >= init) {
            r2g = A.search2 - marg(A.mg, A.search2);
        } else {
            const float kd = key_d2(lk[KG + 1] > tau_g ? lk[KG + 1] : tau_g);
            r2g = kd - marg(A.mg, kd);
        }
        tau_g_hi = tau_g >= init ? A.search2 : __uint_as_float((tau_g | 63u) + 1u);
    }

    int c = 0;
#pragma unroll
    for (int m = 0; m < K1; ++m) c += lk[m] < init ? 1 : 0;
    const int nacc = min(c, K);
    unsigned tau = init;
#pragma unroll
    for (int m = 0; m < K; ++m)
        if (m == nacc - 1) tau = lk[m];
    const float tau_d2 = key_d2(tau);
    bool amb = false;
    if (c > K) {
        const float a1 = key_d2(lk[K - 1]), a2 = key_d2(lk[K]);
        amb = (a2 - a1) <= marg(A.mg, a1) + marg(A.mg, a2);
    }
    const float dn2_lo = (float)A.dn2 * (1.0f - 2.4e-7f);
    if (tau_d2 + marg(A.mg, tau_d2) >= dn2_lo) amb = true;
    amb = amb && q.valid;

    // ---- phase 2: fp64 shifted sums over the accepted keys ------------------
    CovSums<D> S;
    S.n = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) S.s[a] = 0.0;
#pragma unroll
    for (int k = 0; k < D * (D + 1) / 2; ++k) S.ss[k] = 0.0;
    const bool take_lane = q.valid && !amb;
    // cull by the top of tau's truncation bucket: a point keyed <= tau may screen above key_d2(tau)
    const float tau_hi = __uint_as_float((tau | 63u) + 1u);
    // the lane's phase-2 bound: the covariance's, and the graph row's
    const float b2 = fmaxf(take_lane ? tau_hi : -1.f, (G && q.valid) ? tau_g_hi : -1.f);
    int gcnt = 0;
    bool gover = false;
    float4* row_out = G ? A.g_nb + (int64_t)i * KG : nullptr;
    auto visit2 = [&](int Tt) -> bool {
        const TileInfo ti = tile_meta(cl, Tt);
        float pr[D];
        const bool need = lane_gap2<D>(q, ti, pr) <= b2;
        if (!__any(need)) return false;
        const unsigned sub = sub_mask<D>(ti, pr, b2 >= 0.f, b2);
        stage_f32(cl, ti, L);
        stage_f64(cl, ti, L);
        scan_tile<D>(L, ti.count, pr, [&](unsigned key, int j) {
            const bool take = take_lane && key <= tau;
            if (__any(take)) {
                const double qq[3] = {L.t.x64[j], L.t.y64[j], L.t.z64[j]};
                double d[D];
#pragma unroll
                for (int a = 0; a < D; ++a) d[a] = qq[a] - q.p64[a];
                if (take) cov_add<D>(S, d);
            }
            if constexpr (G) {
                const int t = ti.start + j;
                if (q.valid && key <= tau_g && t != i) {
                    if (gcnt < KG) {
                        const double qq[3] = {L.t.x64[j], L.t.y64[j], L.t.z64[j]};
                        float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
                        for (int a = 0; a < D; ++a) v[a] = (float)(qq[a] - q.p64[a]);
                        row_out[gcnt] = make_float4(v[0], v[1], v[2], __int_as_float(t));
                        ++gcnt;
                    } else {
                        gover = true;
                    }
                }
            }
        }, sub);
        wave_sync();
        return true;
    };
    traverse<D>(cl, qb, T, visit2, [&]() { return wave_maxf(b2); });
    if (G && q.valid) {
        // r rounded down; an overflowing row (ties at tau beyond kGraphK) certifies nothing
        const float r = gover ? 0.f : __builtin_amdgcn_sqrtf(fmaxf(r2g, 0.f)) * 0.99999f;
        A.g_nbh[i] = make_float2(r, __int_as_float(gcnt));
    }

    // ---- fp64 fallback for lanes the screen could not decide ----------------
    if (__any(amb)) {
        if (A.amb_counter && l == 0) atomicAdd(A.amb_counter, __popcll(__ballot(amb)));
        double lk64[K];
#pragma unroll
        for (int m = 0; m < K; ++m) lk64[m] = A.dn2;
        const float bound_f = A.search2;
        auto visit3 = [&](int Tt) -> bool {
            const TileInfo ti = tile_meta(cl, Tt);
            float pr[D];
            const float b64 = (float)lk64[K - 1];
            const bool need = amb && lane_gap2<D>(q, ti, pr) <= b64 + 2.f * marg(A.mg, b64);
            if (!__any(need)) return false;
            stage_f64(cl, ti, L);
            for (int j = 0; j < ti.count; ++j) {
                const double qq[3] = {L.t.x64[j], L.t.y64[j], L.t.z64[j]};
                const double d2 = dist2_exact<D>(qq, q.p64);
                if (__any(amb && d2 < lk64[K - 1])) {
                    if (amb) {
#pragma unroll
                        for (int m = K - 1; m > 0; --m) lk64[m] = fmin(lk64[m], fmax(lk64[m - 1], d2));
                        lk64[0] = fmin(lk64[0], d2);
                    }
                }
            }
            wave_sync();
            return true;
        };
        traverse<D>(cl, qb, T, visit3, [&]() { return wave_maxf(amb ? bound_f : -1.f); });
        int c64 = 0;
#pragma unroll
        for (int m = 0; m < K; ++m) c64 += lk64[m] < A.dn2 ? 1 : 0;
        double tau64 = A.dn2;
#pragma unroll
        for (int m = 0; m < K; ++m)
            if (m == c64 - 1) tau64 = lk64[m];
        int nless = 0;
#pragma unroll
        for (int m = 0; m < K; ++m) nless += lk64[m] < tau64 ? 1 : 0;
        int eq_left = c64 - nless;
        auto visit4 = [&](int Tt) -> bool {
            const TileInfo ti = tile_meta(cl, Tt);
            float pr[D];
            const float b64 = (float)tau64;
            const bool need = amb && lane_gap2<D>(q, ti, pr) <= b64 + 2.f * marg(A.mg, b64);
            if (!__any(need)) return false;
            stage_f64(cl, ti, L);
            for (int j = 0; j < ti.count; ++j) {
                const double qq[3] = {L.t.x64[j], L.t.y64[j], L.t.z64[j]};
                const double d2 = dist2_exact<D>(qq, q.p64);
                bool take = amb && c64 > 0 && (d2 < tau64 || (d2 == tau64 && eq_left > 0));
                if (take && d2 == tau64) --eq_left;
                if (__any(take)) {
                    double d[D];
#pragma unroll
                    for (int a = 0; a < D; ++a) d[a] = qq[a] - q.p64[a];
                    if (take) cov_add<D>(S, d);
                }
            }
            wave_sync();
            return true;
        };
        traverse<D>(cl, qb, T, visit4, [&]() {
            const float b64 = (float)tau64;
            return wave_maxf(amb ? b64 + 2.f * marg(A.mg, b64) : -1.f);
        });
    }

    if (q.valid) {
        // m into the point's record (PointRec: a is the cloud's epsilon and is not stored; an isolated point,
        // the descriptor's own test, is marked in m0)
        const double4 cd = cov_descriptor<D>(S, A.min_nb, A.eps_a, A.m_scale);
        const bool isolated = S.n < (double)A.min_nb;
        PointRec* const r = A.rec_out + i;
        r->m0 = isolated ? __longlong_as_double((long long)kRecIsolated) : cd.y;
        *reinterpret_cast<double2*>(&r->m1) = make_double2(cd.z, cd.w);
        A.count_out[i] = (int)S.n;
    }
}

// ---------------------------------------------------------------------------
// target neighbour graph: for every target point i its kGraphK nearest other target
// points (relative positions + sorted indices) and a radius r(i) such that EVERY target t != i with true
// |x_t - x_i| < r(i) is in the row.  Built once per target cloud by k_knn_cov<D, K, true> (the same walks
// as the covariances); k_corr's graph descent proves nearest neighbours with it.  Only conservativeness of
// r matters (no tie rules): phase 1 keeps the kGraphK + 2 smallest screened keys (self included); phase 2
// emits the rows keyed <= tau = the (kGraphK + 1)-th key, self excluded; a row not emitted has a screened
// key > tau, so its true d2 >= key_d2(lk[kGraphK + 1]) - margin when that key is above tau (else
// key_d2(tau) - margin); a lane that found fewer keys within the screen radius has every target within it:
// r2 = search2 - margin.
// Pack the graph rows (DevCloud::nbq / nbx): offsets quantised to int16 in units of s = max |offset| / 32767
// (error <= s / 2 per axis, which k_corr's bound adds), entries ordered nearest-first, each with its
// sorted-index delta (kGraphFar when it does not fit 16 bits), so a descent step finds the next node without
// reading nbi.
__global__ void __launch_bounds__(256) k_graph_pack(const float4* __restrict__ nb, const float2* __restrict__ nbh,
                                                    int64_t n, uint4* __restrict__ nbq, uint4* __restrict__ nbx,
                                                    int32_t* __restrict__ nbi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 h = nbh[i];
    const int cnt = __float_as_int(h.y);
    float m = 0.f;
    for (int k = 0; k < cnt; ++k) {
        const float4 v = nb[i * kGraphK + k];
        m = fmaxf(m, fmaxf(fabsf(v.x), fmaxf(fabsf(v.y), fabsf(v.z))));
    }
    const float s = m > 0.f ? m / 32767.f : 1e-30f;
    const float inv = 1.f / s;
    // entries nearest-first (squared offset length, ties by sorted index): k_corr's descent reads the first
    // half-line and needs the rest only when an entry there could still be the nearest
    float key[kGraphK];
    int ord[kGraphK];
    for (int k = 0; k < cnt; ++k) {
        const float4 v = nb[i * kGraphK + k];
        const float kk = fmaf(v.z, v.z, fmaf(v.y, v.y, v.x * v.x));
        const int t = __float_as_int(v.w);
        int pos = k;
        while (pos > 0 && (key[pos - 1] > kk || (key[pos - 1] == kk && __float_as_int(nb[i * kGraphK + ord[pos - 1]].w) > t))) {
            key[pos] = key[pos - 1];
            ord[pos] = ord[pos - 1];
            --pos;
        }
        key[pos] = kk;
        ord[pos] = k;
    }
    uint32_t w[2 + 2 * kGraphK];
    w[0] = __float_as_uint(h.x);
    w[1] = __float_as_uint(s);
    // unused entries (k >= cnt) repeat the last real entry (or the node itself, offset and delta 0, in an
    // empty row), so the descent needs no per-entry validity test: a repeated entry never becomes the
    // strictly nearer candidate and at most makes the runner-up equal the winner, which the descent
    // treats as a near tie resolved exactly over the real entries (nbi = -1 marks the repeats)
    int q[4] = {0, 0, 0, 0};
    for (int k = 0; k < kGraphK; ++k) {
        int idx = -1;
        if (k < cnt) {
            const float4 v = nb[i * kGraphK + ord[k]];
            const float c[3] = {v.x, v.y, v.z};
            for (int a = 0; a < 3; ++a) q[a] = max(-32767, min(32767, __float2int_rn(c[a] * inv)));
            idx = __float_as_int(v.w);
            const int64_t d = (int64_t)idx - i;
            q[3] = d >= -32767 && d <= 32767 ? (int)d : kGraphFar;
        }
        w[2 + 2 * k] = ((uint32_t)q[0] & 0xFFFFu) | ((uint32_t)q[1] << 16);
        w[3 + 2 * k] = ((uint32_t)q[2] & 0xFFFFu) | ((uint32_t)q[3] << 16);
        nbi[i * kGraphK + k] = idx;
    }
    for (int c = 0; c < 8; ++c) nbq[i * 8 + c] = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
    uint32_t x[12] = {};
    for (int k = 0; k < 2 * (kGraphK - kGraphLineA); ++k) x[k] = w[2 + 2 * kGraphLineA + k];
    for (int c = 0; c < 3; ++c) nbx[i * 3 + c] = make_uint4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
}

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------
hipError_t launch_knn_cov(const CovArgs& a, int dim, int k, bool graph, hipStream_t st) {
    clear_foreign_error();
    const int nq = a.q_end - a.q_begin;
    if (nq <= 0) return hipSuccess;
    if (a.split != 1 && a.split != kSub) return hipErrorInvalidValue;
    const unsigned g = (unsigned)(((int64_t)nq * a.split + kWavesPerWG - 1) / kWavesPerWG);
#define GICP_KNN(DD, KK)                                                                              \
    if (dim == DD && k == KK) {                                                                        \
        if (graph) hipLaunchKernelGGL((k_knn_cov<DD, KK, true>), dim3(g), dim3(256), 0, st, a);        \
        else hipLaunchKernelGGL((k_knn_cov<DD, KK, false>), dim3(g), dim3(256), 0, st, a);             \
        return hipGetLastError();                                                                      \
    }
    GICP_KNN(2, 6)
    GICP_KNN(3, 20)
    GICP_KNN(3, 10)
    GICP_KNN(2, 10)
#undef GICP_KNN
    return hipErrorInvalidValue;
}

hipError_t launch_graph_pack(const GraphArgs& a, hipStream_t st) {
    clear_foreign_error();
    if (a.cl.n <= 0) return hipSuccess;
    const unsigned gp = grid256(a.cl.n);
    hipLaunchKernelGGL(k_graph_pack, dim3(gp), dim3(256), 0, st, a.nb, a.nbh, a.cl.n, a.nbq, a.nbx, a.nbi);
    return hipGetLastError();
}

}  // namespace gicp
