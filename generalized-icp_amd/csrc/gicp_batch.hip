// gicp_batch.hip — batched registration on the MI355X (gfx950): many small cloud pairs in one launch
// (DESIGN.md §3p).  A pair of a few hundred points keeps a few wavefronts busy and a gicp_align call is launch
// and synchronisation latency; here every problem gets ONE workgroup that stays for the problem's whole outer
// loop, so the GPU's idle CUs become throughput.  No index is built: the clouds are small enough for exact fp64
// brute force over points held in LDS.
//
//   k_batch_cov<D, K>    per-point surface covariances with k_knn_cov's semantics: the K nearest (self included)
//                        among those strictly nearer than d_n, ties at the K-th distance to the lower rows, the
//                        shifted sums in row order, cov_descriptor's C = a I - m m^T.  One lane per point, its
//                        cloud in LDS; the K smallest distances live in K registers (an unrolled compare-exchange
//                        chain, no indexed private array).
//   k_batch_align<D, R>  one workgroup per problem.  Per iteration: every source row p' = t + R s and its exact
//                        nearest target (the lower row on equal distance), W and the robust weight as k_corr's
//                        epilogue forms them, the statistics summed in source-row order by one thread per
//                        statistic, then wave 0 runs solve_update<D> (gicp_solve_dev.h) on the problem's own
//                        IterState in LDS.  No atomics, no host round trip, nothing shared between workgroups:
//                        a problem's bits depend on its clouds, its T0 and the parameters alone.
#include <hip/hip_runtime.h>

#include "gicp_cov_dev.h"
#include "gicp_internal.h"
#include "gicp_solver.h"
#include "gicp_solve_dev.h"
#include "gicp_stats_dev.h"
#include "gicp_wave_dev.h"

namespace gicp {
namespace {

constexpr int kBatchUnroll = 4;   // target rows a lane has in flight in k_batch_align's search

extern __shared__ double s_mem[];

template <int D, int K>
__global__ void __launch_bounds__(kBatchThreads) k_batch_cov(BatchCovArgs A) {
    const int2 wk = A.work[blockIdx.x];
    const int64_t o = A.offsets[wk.x];
    const int n = (int)(A.offsets[wk.x + 1] - o);
    const int cap = A.cap;
    for (int j = threadIdx.x; j < n; j += kBatchThreads)
#pragma unroll
        for (int a = 0; a < D; ++a) s_mem[a * cap + j] = A.xyz[(o + j) * D + a];
    __syncthreads();
    const int i = wk.y + (int)threadIdx.x;
    if (i >= n) return;
    double p[D];
#pragma unroll
    for (int a = 0; a < D; ++a) p[a] = s_mem[a * cap + i];
    // the K smallest d2 below d_n^2, ascending (every lane reads row j: an LDS broadcast)
    double lk[K];
#pragma unroll
    for (int m = 0; m < K; ++m) lk[m] = A.dn2;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        double q[D];
#pragma unroll
        for (int a = 0; a < D; ++a) q[a] = s_mem[a * cap + j];
        const double d2 = dist2_exact<D>(q, p);
        if (d2 < lk[K - 1]) {
#pragma unroll
            for (int m = K - 1; m > 0; --m) lk[m] = fmin(lk[m], fmax(lk[m - 1], d2));
            lk[0] = fmin(lk[0], d2);
        }
    }
    int c = 0;
#pragma unroll
    for (int m = 0; m < K; ++m) c += lk[m] < A.dn2 ? 1 : 0;
    double tau = A.dn2;   // the c-th smallest: rows below it are in, rows at it while places are left
#pragma unroll
    for (int m = 0; m < K; ++m)
        if (m == c - 1) tau = lk[m];
    int nless = 0;
#pragma unroll
    for (int m = 0; m < K; ++m) nless += lk[m] < tau ? 1 : 0;
    int eq_left = c - nless;
    CovSums<D> S;
    S.n = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) S.s[a] = 0.0;
#pragma unroll
    for (int k = 0; k < D * (D + 1) / 2; ++k) S.ss[k] = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        double q[D];
#pragma unroll
        for (int a = 0; a < D; ++a) q[a] = s_mem[a * cap + j];
        const double d2 = dist2_exact<D>(q, p);
        const bool take = c > 0 && (d2 < tau || (d2 == tau && eq_left > 0));
        if (take) {
            if (d2 == tau) --eq_left;
            double d[D];
#pragma unroll
            for (int a = 0; a < D; ++a) d[a] = q[a] - p[a];
            cov_add<D>(S, d);
        }
    }
    const double4 cv = cov_descriptor<D, true>(S, A.min_nb, A.eps_a, A.m_scale);
    A.cov[o + i] = cv;
    A.count[o + i] = (int)S.n;
    if (A.dbg_cov) {   // C = a I - m m^T, the products rounded on their own (k_rotate_cov's formula at R = I)
        const double m[3] = {cv.y, cv.z, cv.w};
        double* out = A.dbg_cov + (o + i) * D * D;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) out[a * D + b] = (a == b ? cv.x : 0.0) - __dmul_rn(m[a], m[b]);
    }
}

// LDS of a k_batch_align workgroup, in doubles: the reduction's row chunk (the solve's exchange area lies over
// it: the solve runs when the chunk is spent), the pass's statistics, the problem's IterState, the header copy
// solve_update reads, then the target's points [D][cap]
template <int D>
struct BatchLds {
    static constexpr int NS = D * (D + 1) / 2;
    static constexpr int NU = NS + D + 3;   // u = (W sym, W r, r^T W r, accepted, |r|^2)
    static constexpr int NV = NS + D + 1;   // v = (s s sym, s, 1)
    static constexpr int NUV = NU + NV;
    static constexpr int kRow = kBatchRows * NUV;
    static constexpr int kSolve = (int)((sizeof(SolveLds<D>) + 7) / 8);
    static constexpr int oStats = kRow > kSolve ? kRow : kSolve;
    static constexpr int oState = oStats + 80;
    static constexpr int oHdr = oState + (int)(sizeof(IterState) / 8);
    static constexpr int oTgt = oHdr + kStateHeader;
    static constexpr size_t bytes(int cap) { return sizeof(double) * ((size_t)oTgt + (size_t)D * cap); }
};
static_assert(sizeof(IterState) % 8 == 0 && nstat_ext(3) <= 80, "the state and the statistics are whole doubles");
static_assert(BatchLds<3>::bytes(kBatchMaxPoints) <= 65536 && BatchLds<2>::bytes(kBatchMaxPoints) <= 65536,
              "the largest target fits a workgroup's 64 KB");

template <int D, bool Robust>
__global__ void __launch_bounds__(kBatchThreads) k_batch_align(BatchArgs A) {
    using L = BatchLds<D>;
    constexpr int NS = L::NS, NU = L::NU, NV = L::NV, NUV = L::NUV, N1 = D + 1;
    constexpr int NSS = nstat(D), NSX = nstat_ext(D);
    double* const s_row = s_mem;
    SolveLds<D>* const s_sl = reinterpret_cast<SolveLds<D>*>(s_mem);
    double* const s_stats = s_mem + L::oStats;
    IterState* const s_state = reinterpret_cast<IterState*>(s_mem + L::oState);
    IterState* const s_hdr = reinterpret_cast<IterState*>(s_mem + L::oHdr);   // (its header only)
    double* const s_tgt = s_mem + L::oTgt;
    const int tid = threadIdx.x, b = blockIdx.x;
    const gicp_batch_problem* const pr = A.prob + b;
    const int64_t so = A.offsets[pr->source], to = A.offsets[pr->target];
    const int ns = (int)(A.offsets[pr->source + 1] - so), nt = (int)(A.offsets[pr->target + 1] - to);
    const int cap = A.cap;
    for (int j = tid; j < nt; j += kBatchThreads)
#pragma unroll
        for (int a = 0; a < D; ++a) s_tgt[a * cap + j] = A.xyz[(to + j) * D + a];
    // the problem's state: what gicp_align uploads before its loop
    for (int k = tid; k < (int)(sizeof(IterState) / 8); k += kBatchThreads) reinterpret_cast<double*>(s_state)[k] = 0.0;
    if (tid >= NSS && tid < NSX) s_stats[tid] = tid == NSS + 1 ? (double)ns * (double)nt : 0.0;   // pairs evaluated
    __syncthreads();
    if (tid < N1 * N1) s_state->T[tid] = pr->T0[tid];
    if (tid == 0) {
        s_state->last_loss = INFINITY;
        s_state->tol = A.tol;
        s_state->fixed = A.fixed;
        s_state->trans_eps = A.trans_eps;
        s_state->rot_cos = A.rot_cos;
        s_state->fit_eps = A.fit_eps;
        s_state->rel_eps = A.rel_eps;
        s_state->prev_mse = INFINITY;
        s_state->converged_at = -1;
    }
    // P lanes share a source row (each takes every P-th target row) while the rows leave threads idle; a power
    // of two up to the wave, a function of the problem's own size alone
    int P = 1;
    while (P < kWave && kBatchThreads / (2 * P) >= ns) P *= 2;
    const int slots = kBatchThreads / P, r = tid / P, pl = tid & (P - 1);
    const int nsweeps = (ns + slots - 1) / slots;
    int iu = 0, iv = 0;
    if (tid <= NSS) stat_terms<D>(tid, iu, iv);
    const int64_t row0 = (A.dbg_index || A.dbg_dist) ? A.row0[b] : 0;

    for (int it = 0; it < A.max_iter; ++it) {
        __syncthreads();   // the state as the last solve (or the set-up) left it
        if (tid < kStateHeader) reinterpret_cast<double*>(s_hdr)[tid] = reinterpret_cast<const double*>(s_state)[tid];
        __syncthreads();
        if (s_hdr->converged) break;   // (uniform)
        double R[D * D], t[D];
#pragma unroll
        for (int a = 0; a < D; ++a) {
#pragma unroll
            for (int c = 0; c < D; ++c) R[a * D + c] = s_hdr->T[a * N1 + c];
            t[a] = s_hdr->T[a * N1 + D];
        }
        double acc = 0.0;   // statistic tid, summed in source-row order
        for (int sw = 0; sw < nsweeps; ++sw) {
            const int i = sw * slots + r;
            const bool valid = i < ns;
            double sv[D] = {}, pp[D] = {};
            double best = INFINITY;
            int bj = 0x7FFFFFFF;
            if (valid) {
#pragma unroll
                for (int a = 0; a < D; ++a) sv[a] = A.xyz[(so + i) * D + a];
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    double p = t[a];
#pragma unroll
                    for (int c = 0; c < D; ++c) p += R[a * D + c] * sv[c];
                    pp[a] = p;
                }
                // ascending rows, strict <: the lower row on equal distance.  kBatchUnroll rows at a time, with a
                // trip count the whole workgroup shares: their LDS reads and distances overlap (one row at a time
                // the loop waits out an LDS round trip and a chain of fp64 operations per row), the comparisons
                // keep their order; a row past the end reads the last row and compares as +inf
                for (int jb = 0; jb < nt; jb += kBatchUnroll * P) {
                    double d2u[kBatchUnroll];
#pragma unroll
                    for (int k = 0; k < kBatchUnroll; ++k) {
                        const int j = jb + k * P + pl, jc = min(j, nt - 1);
                        double q[D];
#pragma unroll
                        for (int a = 0; a < D; ++a) q[a] = s_tgt[a * cap + jc];
                        const double d2 = dist2_exact<D>(q, pp);
                        d2u[k] = j < nt ? d2 : INFINITY;
                    }
#pragma unroll
                    for (int k = 0; k < kBatchUnroll; ++k)
                        if (d2u[k] < best) {
                            best = d2u[k];
                            bj = jb + k * P + pl;
                        }
                }
            }
            for (int o = 1; o < P; o <<= 1) {   // (a row's lanes are P consecutive lanes of one wave)
                const double od = __shfl_xor(best, o);
                const int oj = __shfl_xor(bj, o);
                if (od < best || (od == best && oj < bj)) {
                    best = od;
                    bj = oj;
                }
            }
            // ---- W = inv(R C_s R^T + C_t) or its model, the robust weight, r: k_corr's epilogue restated (no shared
            // form left both kernels' code as it is) ----
            double u[NU] = {}, v[NV] = {};
            const bool writer = valid && pl == 0;
            if (writer) {
                // sqrt(d2) <= d_c (accept_d2_max); a row whose every d2 overflowed found no target at all
                const bool on = best <= A.dc2_max && bj < nt;
                if (A.dbg_dist) A.dbg_dist[row0 + i] = sqrt(best);
                if (A.dbg_index) A.dbg_index[row0 + i] = on ? (int64_t)bj : -1;
                if (on) {
                    double W[D][D], qv[D];
#pragma unroll
                    for (int a = 0; a < D; ++a) qv[a] = s_tgt[a * cap + bj];
                    const double4 ct = A.cov[to + bj];
                    const double mt[3] = {ct.y, ct.z, ct.w};
                    if (A.cov_model == GICP_COV_POINT_TO_POINT) {
#pragma unroll
                        for (int a = 0; a < D; ++a)
#pragma unroll
                            for (int c = 0; c < D; ++c) W[a][c] = a == c ? 1.0 : 0.0;
                    } else if (A.cov_model == GICP_COV_POINT_TO_PLANE) {
#pragma unroll
                        for (int a = 0; a < D; ++a)
#pragma unroll
                            for (int c = 0; c < D; ++c) W[a][c] = mt[a] * mt[c] * A.pl_inv;
                    } else {
                        const double4 cs = A.cov[so + i];
                        const double ms[3] = {cs.y, cs.z, cs.w};
                        double mr[D];
#pragma unroll
                        for (int a = 0; a < D; ++a) {
                            mr[a] = 0.0;
#pragma unroll
                            for (int c = 0; c < D; ++c) mr[a] += R[a * D + c] * ms[c];
                        }
                        double S[D][D];
#pragma unroll
                        for (int a = 0; a < D; ++a)
#pragma unroll
                            for (int c = 0; c < D; ++c)
                                S[a][c] = (a == c ? cs.x + ct.x : 0.0) - mr[a] * mr[c] - mt[a] * mt[c];
                        if constexpr (D == 2) {
                            const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
                            const double id = solver_detail::recip(det);
                            W[0][0] = S[1][1] * id;
                            W[1][1] = S[0][0] * id;
                            W[0][1] = W[1][0] = -S[0][1] * id;
                        } else {
                            const double c00 = S[1][1] * S[2][2] - S[1][2] * S[2][1];
                            const double c01 = S[0][2] * S[2][1] - S[0][1] * S[2][2];
                            const double c02 = S[0][1] * S[1][2] - S[0][2] * S[1][1];
                            const double c11 = S[0][0] * S[2][2] - S[0][2] * S[2][0];
                            const double c12 = S[0][2] * S[1][0] - S[0][0] * S[1][2];
                            const double c22 = S[0][0] * S[1][1] - S[0][1] * S[1][0];
                            const double det = S[0][0] * c00 + S[0][1] * c01 + S[0][2] * c02;
                            const double id = solver_detail::recip(det);
                            W[0][0] = c00 * id;
                            W[0][1] = W[1][0] = c01 * id;
                            W[0][2] = W[2][0] = c02 * id;
                            W[1][1] = c11 * id;
                            W[1][2] = W[2][1] = c12 * id;
                            W[2][2] = c22 * id;
                        }
                    }
                    double rr[D], wr[D], r2 = 0.0, rwr = 0.0;
#pragma unroll
                    for (int a = 0; a < D; ++a) rr[a] = qv[a] - pp[a];
#pragma unroll
                    for (int a = 0; a < D; ++a) r2 += rr[a] * rr[a];
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        wr[a] = 0.0;
#pragma unroll
                        for (int c = 0; c < D; ++c) wr[a] += W[a][c] * rr[c];
                        rwr += rr[a] * wr[a];
                    }
                    if constexpr (Robust) {   // w from e = r^T W r (include/gicp_hip.h GICP_ROBUST_*); W~ = w W
                        const double e = fmax(rwr, 0.0), c2 = A.robust_c2;
                        double w;
                        if (A.robust_kernel == GICP_ROBUST_HUBER) {
                            const double s = sqrt(e);
                            w = s <= A.robust_c ? 1.0 : A.robust_c / s;
                        } else if (A.robust_kernel == GICP_ROBUST_CAUCHY) {
                            w = 1.0 / (1.0 + e / c2);
                        } else if (A.robust_kernel == GICP_ROBUST_GEMAN_MCCLURE) {
                            const double g = c2 / (c2 + e);
                            w = g * g;
                        } else {   // GICP_ROBUST_TUKEY
                            const double g = 1.0 - e / c2;
                            w = e < c2 ? g * g : 0.0;
                        }
#pragma unroll
                        for (int a = 0; a < D; ++a) {
#pragma unroll
                            for (int c = 0; c < D; ++c) W[a][c] *= w;
                            wr[a] *= w;
                        }
                        rwr *= w;
                    }
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < D; ++a)
#pragma unroll
                        for (int c = a; c < D; ++c) u[k++] = W[a][c];
#pragma unroll
                    for (int a = 0; a < D; ++a) u[NS + a] = wr[a];
                    u[NS + D] = rwr;
                    u[NS + D + 1] = 1.0;
                    u[NS + D + 2] = r2;
                }
                int k = 0;
#pragma unroll
                for (int a = 0; a < D; ++a)
#pragma unroll
                    for (int c = a; c < D; ++c) v[k++] = sv[a] * sv[c];
#pragma unroll
                for (int a = 0; a < D; ++a) v[NS + a] = sv[a];
                v[NS + D] = 1.0;
            }
            // ---- the sweep's rows into the statistics, kBatchRows at a time, in row order ----
            const int rows = min(slots, ns - sw * slots);
            for (int c0 = 0; c0 < rows; c0 += kBatchRows) {
                if (writer && r >= c0 && r < c0 + kBatchRows) {
                    double* const o = s_row + (r - c0) * NUV;
#pragma unroll
                    for (int k = 0; k < NU; ++k) o[k] = u[k];
#pragma unroll
                    for (int k = 0; k < NV; ++k) o[NU + k] = v[k];
                }
                __syncthreads();
                if (tid <= NSS) {
                    const int nr = min(kBatchRows, rows - c0);
                    for (int q = 0; q < nr; ++q) acc += s_row[q * NUV + iu] * s_row[q * NUV + NU + iv];
                }
                __syncthreads();
            }
        }
        if (tid < NSS) s_stats[tid] = acc;
        if (tid == NSS) s_stats[NSS + 3] = acc;   // sum |r|^2 (extended slot)
        __syncthreads();
        if (tid < kWave) solve_update<D>(s_state, s_hdr, s_stats, *s_sl, nullptr);
    }
    __syncthreads();
    BatchOut* const out = A.out + b;
    if (tid < 16) out->T[tid] = s_state->T[tid];
    if (tid < 80) out->stats[tid] = s_state->stats_solved[tid];
    if (tid == 0) {
        out->loss = s_state->loss;
        out->mse = s_state->mse;
        out->iterations = s_state->iter;
        out->converged = s_state->converged;
        out->converged_at = s_state->converged_at;
        out->stop_reason = s_state->stop_reason;
        out->solve_fail = s_state->solve_fail;
        out->pad = 0;
    }
}

}  // namespace

int batch_max_points(int dim) { return (dim == 2 || dim == 3) ? kBatchMaxPoints : GICP_E_INVALID; }

// The covariances of every cloud on `st`: `grid` workgroups, one per A.work entry.  hipErrorInvalidValue for a
// k that has no instantiation.
hipError_t launch_batch_cov(const BatchCovArgs& A, int dim, int k, int grid, hipStream_t st) {
    (void)hipGetLastError();
    if (grid <= 0 || A.cap < 1 || A.cap > kBatchMaxPoints) return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (size_t)dim * A.cap;
#define GICP_BCOV(DD, KK)                                                                                  \
    if (dim == DD && k == KK) {                                                                             \
        hipLaunchKernelGGL((k_batch_cov<DD, KK>), dim3(grid), dim3(kBatchThreads), lds, st, A);            \
        return hipGetLastError();                                                                           \
    }
    GICP_BCOV(2, 6)
    GICP_BCOV(2, 10)
    GICP_BCOV(3, 10)
    GICP_BCOV(3, 20)
#undef GICP_BCOV
    return hipErrorInvalidValue;
}

// The registrations on `st`: one workgroup per problem.
hipError_t launch_batch_align(const BatchArgs& A, int dim, int grid, hipStream_t st) {
    (void)hipGetLastError();
    if (grid <= 0 || A.cap < 1 || A.cap > kBatchMaxPoints || (dim != 2 && dim != 3)) return hipErrorInvalidValue;
    const bool rb = A.robust_kernel != GICP_ROBUST_NONE;
    const dim3 g(grid), blk(kBatchThreads);
    if (dim == 2) {
        const size_t lds = BatchLds<2>::bytes(A.cap);
        if (rb) hipLaunchKernelGGL((k_batch_align<2, true>), g, blk, lds, st, A);
        else hipLaunchKernelGGL((k_batch_align<2, false>), g, blk, lds, st, A);
    } else {
        const size_t lds = BatchLds<3>::bytes(A.cap);
        if (rb) hipLaunchKernelGGL((k_batch_align<3, true>), g, blk, lds, st, A);
        else hipLaunchKernelGGL((k_batch_align<3, false>), g, blk, lds, st, A);
    }
    return hipGetLastError();
}

}  // namespace gicp
