// gicp_eval.hip — the registration report on the MI355X (gfx950, wave64): what gicp_evaluate reduces on the
// device from the per-point outputs a pass left there.
//
//   k_eval_init      the result words, the select's state and its histograms
//   k_eval_values<D> one lane per source row, original order: the two 64-bit keys of the row (bit patterns of
//                    dist_i and of the whitened residual s_i = sqrt(max(r^T W~ r, 0)); all ones if rejected) and
//                    the overlap table: per threshold the inlier count (ballot, one integer atomic per workgroup)
//                    and the workgroup's sum of dist^2 (wave butterfly, waves added in order) as a partial
//   k_eval_sums      one workgroup adds the partials in an order fixed by their number
//   k_sel_hist       one round of the radix select: per distinct prefix a histogram of the round's digit over the
//                    keys that carry the prefix, integer counts in LDS, flushed with integer atomics
//   k_sel_narrow     one wave per rank: the bin that holds the rank (a wave prefix sum over the 256 counts), the
//                    rank inside it, the longer prefix; ranks whose prefixes coincide share one histogram
//
// Pose, thresholds and counts are kernel arguments: wave-uniform, in scalar registers.  No floating-point
// atomics: the counts are integers and the fp64 sums are added in a fixed order, so a report is the same bits on
// every call and every context.  Both key values are non-negative doubles, whose bit patterns order as the
// values do; the all-ones key of a rejected row is above every one of them, and the ranks asked for lie below
// the number of accepted rows, so the select never lands on it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gicp_internal.h"

namespace gicp {

namespace {

constexpr int kSelBlock = 256;
constexpr int kSelGridMax = 1024;   // workgroups per key array: the rest of the keys by a grid stride

__global__ void __launch_bounds__(256) k_eval_init(EvalArgs A) {
    const int tid = threadIdx.x;
    for (int i = tid; i < kSelQueries * kSelBins; i += 256) A.hist[i] = 0u;
    if (tid < kEvalOutWords) A.out[tid] = 0ull;
    if (tid < kSelQueries) {
        A.sel->prefix[tid] = 0ull;
        A.sel->rank[tid] = A.rank[tid];
        A.sel->slot[tid] = (tid / kEvalMax) * kEvalMax;   // no digit known yet: one histogram per array
    }
}

template <int D>
__global__ void __launch_bounds__(kEvalBlock) k_eval_values(EvalArgs A) {
    constexpr int DD = D * D, NW = kEvalBlock / kWave;
    // a row of W~ takes LD doubles in LDS: 9 (3-D) and 5 (2-D) are odd, so the lanes' 8-byte reads of one entry
    // fall into distinct banks
    constexpr int LD = DD | 1;
    __shared__ double s_w[kEvalBlock * LD];
    __shared__ double s_sum[NW][kEvalMax];
    __shared__ unsigned s_cnt[NW][kEvalMax];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int64_t row0 = (int64_t)blockIdx.x * kEvalBlock;
    const int64_t i = row0 + tid;
    const bool in = i < A.n;
    // the workgroup's weights, read at unit stride across the wave
    const int64_t wend = A.n * DD;
#pragma unroll
    for (int k = 0; k < DD; ++k) {
        const int e = k * kEvalBlock + tid;
        const int64_t g = row0 * DD + e;
        s_w[(e / DD) * LD + e % DD] = g < wend ? A.w[g] : 0.0;
    }
    int64_t j = -1;
    double dist = 0.0;
    if (in) {
        j = A.idx[i];
        dist = A.dist[i];
    }
    const bool acc = in && j >= 0 && j < A.m;
    RecPos s4 = {0.0, 0.0, 0.0}, q4 = {0.0, 0.0, 0.0};
    if (acc) {
        s4 = rec_pos(A.src_xyz + A.src_inv[i]);
        q4 = rec_pos(A.tgt_xyz + A.tgt_inv[j]);
    }
    __syncthreads();
    unsigned long long kd = ~0ull, ks = ~0ull;
    if (acc) {
        const double s[3] = {s4.x, s4.y, s4.z}, q[3] = {q4.x, q4.y, q4.z};
        double r[D];
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double p = A.t[a];
#pragma unroll
            for (int b = 0; b < D; ++b) p += A.R[a * 3 + b] * s[b];
            r[a] = q[a] - p;
        }
        double e = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double wr = 0.0;
#pragma unroll
            for (int b = 0; b < D; ++b) wr += s_w[tid * LD + a * D + b] * r[b];
            e += r[a] * wr;
        }
        const double sres = e > 0.0 ? sqrt(e) : 0.0;   // (never -0.0: its bit pattern would sort last)
        kd = (unsigned long long)__double_as_longlong(dist);
        ks = (unsigned long long)__double_as_longlong(sres);
    }
    if (A.nq > 0 && in) {
        A.keys[i] = kd;
        A.keys[A.n + i] = ks;
    }
    if (A.nthr <= 0) return;
#pragma unroll
    for (int t = 0; t < kEvalMax; ++t) {
        if (t < A.nthr) {
            const bool hit = acc && dist <= A.thr[t];
            const unsigned long long m = __ballot(hit);
            double v = hit ? dist * dist : 0.0;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) v += __shfl_xor(v, o);   // (a + b on both partners: one value per wave)
            if (lane == 0) {
                s_sum[wv][t] = v;
                s_cnt[wv][t] = (unsigned)__popcll(m);
            }
        }
    }
    __syncthreads();
    if (tid < A.nthr) {
        double v = s_sum[0][tid];
        unsigned c = s_cnt[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            v += s_sum[w][tid];
            c += s_cnt[w][tid];
        }
        A.part[(int64_t)blockIdx.x * kEvalMax + tid] = v;
        if (c) atomicAdd(&A.out[kEvalOutCnt + tid], (unsigned long long)c);
    }
}

// The partials of threshold t, [nblocks][kEvalMax], added by one workgroup: thread k adds its run of
// ceil(nblocks / 256) consecutive partials in order, then the 256 run sums are added pairwise in a fixed tree.
__global__ void __launch_bounds__(256) k_eval_sums(const double* __restrict__ part, int nblocks, int nthr,
                                                   unsigned long long* out) {
    __shared__ double s[256];
    const int tid = threadIdx.x;
    const int per = (nblocks + 255) / 256;
    const int b0 = min(nblocks, tid * per), b1 = min(nblocks, b0 + per);
    for (int t = 0; t < nthr; ++t) {
        double v = 0.0;
        for (int b = b0; b < b1; ++b) v += part[(int64_t)b * kEvalMax + t];
        s[tid] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) s[tid] += s[tid + o];
            __syncthreads();
        }
        if (tid == 0) out[kEvalOutSum + t] = (unsigned long long)__double_as_longlong(s[0]);
        __syncthreads();
    }
}

// blockIdx.y: the key array.  Round `round` takes bits [64 - 8 (round + 1), 64 - 8 round) of the keys whose
// higher bits equal a query's prefix.
__global__ void __launch_bounds__(kSelBlock) k_sel_hist(const unsigned long long* __restrict__ keys, int64_t n, int nq,
                                                         const SelState* __restrict__ sel, uint32_t* hist, int round) {
    __shared__ uint32_t h[kEvalMax][kSelBins];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int q0 = (int)blockIdx.y * kEvalMax;
    for (int i = tid; i < kEvalMax * kSelBins; i += kSelBlock) (&h[0][0])[i] = 0u;
    unsigned long long pre[kEvalMax];
    bool own[kEvalMax];   // this query's histogram is taken (it is the first of its prefix)
#pragma unroll
    for (int q = 0; q < kEvalMax; ++q) {
        pre[q] = sel->prefix[q0 + q];
        own[q] = q < nq && sel->slot[q0 + q] == q0 + q;
    }
    __syncthreads();
    const int shift = 64 - kSelBits * (round + 1);
    const unsigned long long* k = keys + (int64_t)blockIdx.y * n;
    for (int64_t base = (int64_t)blockIdx.x * kSelBlock; base < n; base += (int64_t)gridDim.x * kSelBlock) {
        const int64_t i = base + tid;
        const bool valid = i < n;
        const unsigned long long key = valid ? k[i] : 0ull;
        const unsigned long long hi = round == 0 ? 0ull : key >> (shift + kSelBits);
        const unsigned digit = (unsigned)(key >> shift) & (kSelBins - 1);
#pragma unroll
        for (int q = 0; q < kEvalMax; ++q) {
            if (!own[q]) continue;
            const bool match = valid && hi == pre[q];
            const unsigned long long m = __ballot(match);
            if (m == 0ull) continue;
            // the high digits of doubles of one scale coincide: one add per wave where every lane agrees
            const int first = __ffsll((long long)m) - 1;
            const unsigned d0 = __shfl(digit, first);
            const unsigned long long same = __ballot(match && digit == d0);
            if (same == m) {
                if (lane == first) atomicAdd(&h[q][d0], (unsigned)__popcll(m));
            } else if (match) {
                atomicAdd(&h[q][digit], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < kEvalMax * kSelBins; i += kSelBlock) {
        const uint32_t v = (&h[0][0])[i];
        if (v) atomicAdd(&hist[q0 * kSelBins + i], v);
    }
}

// One wave per query (16 waves).  The histogram's 256 counts sit 4 to a lane; the lane whose running total first
// passes the rank holds the bin.  Then the state of the next round and clean histograms for it.
__global__ void __launch_bounds__(kSelQueries * kWave) k_sel_narrow(SelState* sel, uint32_t* hist, int nq, int round,
                                                                    unsigned long long* out) {
    __shared__ unsigned long long npre[kSelQueries], nrank[kSelQueries];
    const int q = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const bool live = (q % kEvalMax) < nq;
    if (live) {
        const unsigned long long pre = sel->prefix[q], rk = sel->rank[q];
        const uint4 c = reinterpret_cast<const uint4*>(hist + sel->slot[q] * kSelBins)[lane];
        const unsigned long long loc = (unsigned long long)c.x + c.y + c.z + c.w;
        unsigned long long inc = loc;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        const unsigned long long exc = inc - loc;
        if (lane == 0) {   // (overwritten below by the lane that holds the rank)
            npre[q] = round == 0 ? 0ull : pre << kSelBits;
            nrank[q] = 0ull;
        }
        if (exc <= rk && rk < inc) {
            unsigned long long r = rk - exc;
            unsigned bin = 4u * lane;
            if (r >= c.x) {
                r -= c.x;
                ++bin;
                if (r >= c.y) {
                    r -= c.y;
                    ++bin;
                    if (r >= c.z) {
                        r -= c.z;
                        ++bin;
                    }
                }
            }
            npre[q] = (round == 0 ? 0ull : pre << kSelBits) | bin;
            nrank[q] = r;
        }
    }
    __syncthreads();   // every histogram is read; every new prefix is in LDS
    if (live && lane == 0) {
        int s = q;
        for (int p = q - 1; p >= (q / kEvalMax) * kEvalMax; --p)
            if (npre[p] == npre[q]) s = p;
        sel->prefix[q] = npre[q];
        sel->rank[q] = nrank[q];
        sel->slot[q] = s;
        if (round == kSelRounds - 1) out[kEvalOutKey + q] = npre[q];
    }
    for (int i = threadIdx.x; i < kSelQueries * kSelBins; i += kSelQueries * kWave) hist[i] = 0u;
}

}  // namespace

// The report's device work on `st`, after a pass that left index, distance and weight of every source row in
// A.idx / A.dist / A.w: A.out receives the counts, the sums and, with A.nq > 0, the selected keys.
hipError_t launch_eval(const EvalArgs& A, hipStream_t st) {
    (void)hipGetLastError();
    if (A.n <= 0 || A.m <= 0 || (A.dim != 2 && A.dim != 3) || A.nthr < 0 || A.nthr > kEvalMax || A.nq < 0 ||
        A.nq > kEvalMax || !A.idx || !A.dist || !A.w || !A.src_xyz || !A.src_inv || !A.tgt_xyz || !A.tgt_inv || !A.part ||
        !A.sel || !A.hist || !A.out || (A.nq > 0 && !A.keys))
        return hipErrorInvalidValue;
    const int64_t nb = (A.n + kEvalBlock - 1) / kEvalBlock;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eval_init, dim3(1), dim3(256), 0, st, A);
    if (A.dim == 3) hipLaunchKernelGGL(k_eval_values<3>, dim3((unsigned)nb), dim3(kEvalBlock), 0, st, A);
    else hipLaunchKernelGGL(k_eval_values<2>, dim3((unsigned)nb), dim3(kEvalBlock), 0, st, A);
    if (A.nthr > 0) hipLaunchKernelGGL(k_eval_sums, dim3(1), dim3(256), 0, st, A.part, (int)nb, A.nthr, A.out);
    if (A.nq > 0) {
        const unsigned gx = (unsigned)std::min<int64_t>((A.n + kSelBlock - 1) / kSelBlock, kSelGridMax);
        for (int r = 0; r < kSelRounds; ++r) {
            hipLaunchKernelGGL(k_sel_hist, dim3(gx, 2), dim3(kSelBlock), 0, st, A.keys, A.n, A.nq, A.sel, A.hist, r);
            hipLaunchKernelGGL(k_sel_narrow, dim3(1), dim3(kSelQueries * kWave), 0, st, A.sel, A.hist, A.nq, r, A.out);
        }
    }
    return hipGetLastError();
}

}  // namespace gicp
