// gicp_extras.hip — the drop-in's visualisation extras on the MI355X (gfx950): the top-k of det(W)
// (gicp.py:169-172) and the rotated source covariances (gicp.py:120-121 all_source_cov_matrices).
#include <hip/hip_runtime.h>

#include "gicp_internal.h"

namespace gicp {

// ---------------------------------------------------------------------------
// top-k of det(W) for the drop-in's visualisation extras (gicp.py:169-172)
// ---------------------------------------------------------------------------
// Order: larger det first, equal dets -> larger original index first, i.e. the last k positions of a
// stable ascending argsort.  NaN (rows of other ranks' shards, memset 0xFF) never enters a list.
constexpr int kTopMax = 16;

__device__ __forceinline__ bool top_gt(double va, int64_t ia, double vb, int64_t ib) {
    return va > vb || (va == vb && ia > ib);
}

// Each thread keeps its k best in registers (descending, unrolled so nothing spills), then the block
// pops its k best with k rounds of a block-wide argmax over the threads' heads.
struct TopList {
    double v[kTopMax];
    int64_t i[kTopMax];   // (original index << 32) | sorted position: ties order by the original index
    __device__ void init() {
#pragma unroll
        for (int p = 0; p < kTopMax; ++p) {
            v[p] = -INFINITY;
            i[p] = -1;
        }
    }
    __device__ void insert(double cv, int64_t ci, int k) {
        if (!top_gt(cv, ci, -INFINITY, -1)) return;   // NaN / sentinel
#pragma unroll
        for (int p = 0; p < kTopMax; ++p) {
            if (p < k && top_gt(cv, ci, v[p], i[p])) {
                const double tv = v[p];
                const int64_t ti = i[p];
                v[p] = cv;
                i[p] = ci;
                cv = tv;
                ci = ti;
            }
        }
    }
};

__device__ void top_block_emit(TopList& L, int k, double* out_v, int64_t* out_i) {
    __shared__ double s_v[4];
    __shared__ int64_t s_i[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = 0; r < k; ++r) {
        double bv = L.v[0];
        int64_t bi = L.i[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off);
            const int64_t oi = __shfl_xor(bi, off);
            if (top_gt(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_v[w] = bv;
            s_i[w] = bi;
        }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
        for (int u = 1; u < (int)(blockDim.x >> 6); ++u)
            if (top_gt(s_v[u], s_i[u], bv, bi)) {
                bv = s_v[u];
                bi = s_i[u];
            }
        __syncthreads();
        if (threadIdx.x == 0) {
            out_v[r] = bv;
            out_i[r] = bi;
        }
        if (bi >= 0 && L.i[0] == bi && L.v[0] == bv) {   // indices are unique: exactly one owner pops
#pragma unroll
            for (int p = 0; p + 1 < kTopMax; ++p) {
                L.v[p] = L.v[p + 1];
                L.i[p] = L.i[p + 1];
            }
            L.v[kTopMax - 1] = -INFINITY;
            L.i[kTopMax - 1] = -1;
        }
    }
}

// stage 1: block b reduces its contiguous chunk of det[0, n) to k candidates
__global__ void __launch_bounds__(256) k_top1(const double* __restrict__ det, const int32_t* __restrict__ perm,
                                              int64_t n, int k, double* pv, int64_t* pi) {
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(n, b0 + chunk);
    TopList L;
    L.init();
    for (int64_t x = b0 + threadIdx.x; x < b1; x += blockDim.x)
        L.insert(det[x], ((int64_t)perm[x] << 32) | (int64_t)x, k);
    top_block_emit(L, k, pv + (int64_t)blockIdx.x * k, pi + (int64_t)blockIdx.x * k);
}

// stage 2: one block merges the m = blocks x k candidates; ascending output (np.argsort(...)[-k:]),
// plus the matched target index of each winner
// stage 2: one block reduces the stage-1 candidates; outputs ascending (np.argsort(det)[-k:] order), the
// source as its original index, the target from the pass's sorted-order record (tgt_sorted)
__global__ void __launch_bounds__(256) k_top2(const double* pv, const int64_t* pi, int m, int k,
                                              const int64_t* __restrict__ tgt_sorted, double* ov, int64_t* osrc,
                                              int64_t* otgt) {
    __shared__ double s_ov[kTopMax];
    __shared__ int64_t s_oi[kTopMax];
    TopList L;
    L.init();
    for (int x = threadIdx.x; x < m; x += blockDim.x) L.insert(pv[x], pi[x], k);
    top_block_emit(L, k, s_ov, s_oi);
    __syncthreads();
    if ((int)threadIdx.x < k) {
        const int r = k - 1 - (int)threadIdx.x;   // descending -> ascending
        const int64_t si = s_oi[r];
        ov[threadIdx.x] = si >= 0 ? s_ov[r] : 0.0;
        osrc[threadIdx.x] = si >= 0 ? (si >> 32) : -1;
        otgt[threadIdx.x] = si >= 0 ? tgt_sorted[si & 0xFFFFFFFFll] : -1;
    }
}

hipError_t launch_top_weights(const double* det, const int64_t* tgt_sorted, const int32_t* perm, int64_t n, int k,
                              double* scratch_v, int64_t* scratch_i, int blocks, double* ov, int64_t* osrc,
                              int64_t* otgt, hipStream_t st) {
    clear_foreign_error();
    if (k < 1 || k > kTopMax || blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_top1, dim3(blocks), dim3(256), 0, st, det, perm, n, k, scratch_v, scratch_i);
    hipLaunchKernelGGL(k_top2, dim3(1), dim3(256), 0, st, scratch_v, scratch_i, blocks * k, k, tgt_sorted, ov, osrc,
                       otgt);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// rotated covariances (gicp.py:120-121 all_source_cov_matrices): R C Rᵀ = a I − (R m)(R m)ᵀ per
// point, written in original order, a and m decoded from the point records (decode_cov; a row that was not
// computed comes out NaN).  HBM-bound: 52 B read, D² × 8 B written per point.
// ---------------------------------------------------------------------------
struct Rot {
    double r[9];
};

template <int D>
__global__ void __launch_bounds__(256) k_rotate_cov(const PointRec* __restrict__ rec, double eps_a,
                                                    const int32_t* __restrict__ perm, int64_t n, Rot R,
                                                    double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s0 = rec[i].m0, s1 = rec[i].m1, s2 = rec[i].m2;
    double ca, m0;
    decode_cov(eps_a, s0, s1, ca, m0);
    const double m[3] = {m0, s1, s2};
    double rm[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double v = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) v = fma(R.r[a * D + b], m[b], v);
        rm[a] = v;
    }
    double* o = out + (int64_t)perm[i] * D * D;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) o[a * D + b] = (a == b ? ca : 0.0) - __dmul_rn(rm[a], rm[b]);   // no fma: the
}                                                                                                 // host formula's rounding

hipError_t launch_rotate_cov(const PointRec* rec, double eps_a, const int32_t* perm, int64_t n, int dim, const double* R,
                             double* out, hipStream_t st) {
    clear_foreign_error();
    if (n <= 0) return hipSuccess;
    Rot r{};
    for (int k = 0; k < dim * dim; ++k) r.r[k] = R[k];
    const unsigned g = grid256(n);
    if (dim == 2) hipLaunchKernelGGL(k_rotate_cov<2>, dim3(g), dim3(256), 0, st, rec, eps_a, perm, n, r, out);
    else hipLaunchKernelGGL(k_rotate_cov<3>, dim3(g), dim3(256), 0, st, rec, eps_a, perm, n, r, out);
    return hipGetLastError();
}

}  // namespace gicp
