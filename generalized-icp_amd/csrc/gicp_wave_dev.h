// gicp_wave_dev.h — wave-level device helpers shared by the kernel files: uniform wave reductions, lane reads,
// the wave sort, the screen's key and margin helpers, the exact fp64 square distance (the order a KD-tree sums it
// in: the reference's neighbour queries, gicp.py:19-20 and gicp.py:126-127), and the diagnostic phase timers.
// Device code only: __device__ __forceinline__ functions and templates, no __shared__ or __device__ variables.
#pragma once
#include <hip/hip_runtime.h>

#include "gicp_internal.h"

namespace gicp {

__device__ __forceinline__ int lane_id() { return __lane_id(); }
__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
    return max(min(a, b), min(max(a, b), c));
}
__device__ __forceinline__ float key_d2(unsigned k) { return __uint_as_float(k & ~63u); }
// margin of the fp32 screen at d2 (raw v_sqrt_f32, inflated past its 1-ulp error: the bound stays conservative)
__device__ __forceinline__ float marg(const Margin& m, float d2) {
    return fmaf(m.a * 1.0001f, __builtin_amdgcn_sqrtf(d2), fmaf(m.c, d2, m.b));
}

// Wave-wide min / max of floats that are >= 0 or a negative "none" marker, result uniform
// (SGPR): signed-integer compares on the bit patterns (monotonic for such values, no NaN
// canonicalisation), each step one v_{min,max}_i32 with a DPP source: row_shr 1/2/4/8,
// row_bcast 15/31, then readlane 63.
#define GICP_WAVE_REDUCE(OP, ID, x)                                                      \
    x = OP(x, __builtin_amdgcn_update_dpp(ID, x, 0x111, 0xf, 0xf, false));               \
    x = OP(x, __builtin_amdgcn_update_dpp(ID, x, 0x112, 0xf, 0xf, false));               \
    x = OP(x, __builtin_amdgcn_update_dpp(ID, x, 0x114, 0xf, 0xf, false));               \
    x = OP(x, __builtin_amdgcn_update_dpp(ID, x, 0x118, 0xf, 0xf, false));               \
    x = OP(x, __builtin_amdgcn_update_dpp(ID, x, 0x142, 0xa, 0xf, false));               \
    x = OP(x, __builtin_amdgcn_update_dpp(ID, x, 0x143, 0xc, 0xf, false));
__device__ __forceinline__ float wave_maxf(float v) {
    int x = __float_as_int(v);
    GICP_WAVE_REDUCE(max, (int)0x80000000, x)
    return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}
__device__ __forceinline__ float readlane_f(float v, int k) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ double readlane_d(double v, int k) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), k);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// wave minimum of keys < 2^31 (screen keys: non-negative fp32 bits), uniform
__device__ __forceinline__ unsigned wave_min_key(unsigned v) {
    int x = (int)v;
    GICP_WAVE_REDUCE(min, 0x7fffffff, x)
    return (unsigned)__builtin_amdgcn_readlane(x, 63);
}
__device__ __forceinline__ double wave_mind(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_maxd(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }
// ascending bitonic sort of one (key, val) pair per lane across the wave; ties by val (deterministic)
__device__ __forceinline__ void wave_sort64(float& key, int& val) {
    const int l = __lane_id();
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const float pk = __shfl_xor(key, j);
            const int pv = __shfl_xor(val, j);
            const bool take_min = ((l & k) == 0) == ((l & j) == 0);
            const bool less = pk < key || (pk == key && pv < val);
            const bool greater = pk > key || (pk == key && pv > val);
            if (take_min ? less : greater) {
                key = pk;
                val = pv;
            }
        }
}
// any lane: the ballot's scalar result tested directly (no bool -> int -> compare round trip)
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// Diagnostic-only phase timer (build with `make STAMPS=1`): s_memtime cycles per phase per wave.
// 0 setup, 1 traversal tests, 2 tile need-test + staging, 3 row scan, 4 fp64 fallback,
// 5 epilogue (W, statistics), 6 statistics reduction.  Compiles to nothing otherwise.
struct Stamps {
#ifdef GICP_STAMPS
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last = 0, rt0 = 0;
    __device__ __forceinline__ void start() {
        last = __builtin_amdgcn_s_memtime();
        rt0 = __builtin_amdgcn_s_memrealtime();
    }
    __device__ __forceinline__ void mark(int c) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        acc[c] += t - last;
        last = t;
    }
    // event counters: 0 tile visits, 1 tiles scanned, 2 chunks scanned, 3 list used, 4 list length,
    // 5 traversal block tests, 6 traversal candidate blocks, 7 fp64 fallback tiles
    unsigned cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void count(int k, unsigned v = 1) { cnt[k] += v; }
#elif defined(GICP_TIMELINE)   // `make VARIANT=tl VDEFS=-DGICP_TIMELINE`: wave start/end, phase ends, counters
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // realtime (100 MHz) at the end of the certificate + descent phase and at the end of the walk; the walk's
    // kind (0 none, 1 candidate list, 2 list then full walk, 3 full walk, 4 sparse search); lanes that descended / walked
    unsigned long long tdesc = 0, twalk = 0, ta = 0, tb = 0, te = 0, tf = 0;
    unsigned kind = 0, ndesc = 0, nwalk = 0, nwalk_jp = 0;
    float wb0 = 0.f;
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void count(int k, unsigned v = 1) { cnt[k] += v; }
#else
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void count(int, unsigned = 1) {}
#endif
};

#ifdef GICP_TIMELINE
// realtime stamp taken once `a` and `b` are available (their loads complete): the asm's inputs make the
// compiler wait for them first, and volatile asms keep their order
template <class A, class B>
__device__ __forceinline__ unsigned long long tl_after(A a, B b) {
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(a), "v"(b) : "memory");
    return t;
}
#endif

// exact-rounding fp64 square distance, summed in axis order without FMA contraction
// (the order a KD-tree accumulates it in)
template <int D>
__device__ __forceinline__ double dist2_exact(const double* a, const double* b) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double d = __dsub_rn(a[k], b[k]);
        s = __dadd_rn(s, __dmul_rn(d, d));
    }
    return s;
}

}  // namespace gicp
