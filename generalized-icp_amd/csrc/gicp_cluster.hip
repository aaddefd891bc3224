// gicp_cluster.hip — Euclidean cluster extraction on the MI355X (gfx950), DESIGN.md §3t: the connected components of
// the graph "rows within `radius` of each other", numbered by their smallest row, and the rows of the clusters whose
// size lies in [min_size, max_size].  The predicate is gicp_filter.h's, the decision gicp_cluster.h's: the functions
// the host yardstick calls.
//
//   launch_grid_sort   (gicp_filter.hip) radius outlier removal's grid: k_voxel_key, rocPRIM radix sort of (key, row),
//                      k_ror_gather -- the points packed in key order
//   k_cluster_init     parent[i] = i, size[i] = 0
//   k_cluster_edges<D> the hot kernel: one lane per point IN KEY ORDER walks the neighbour runs that do not lie before
//                      its own (gicp_runs_dev.h: 5 of 9, 2-D 2 of 3) and, in them, the rows after its own, so every
//                      pair is tested once; a pair within the radius whose ends do not already share a root is
//                      united.  ONE lock-free pass: no rounds, no "changed" word, no host round trip
//   k_cluster_roots    one lane per row: the root of its tree (written over its parent), the root flag, the size of
//                      the root by integer atomic adds, one per wave and distinct root
//   rocPRIM            inclusive scan of the root flags -> cluster number + 1: roots ascend with their smallest row
//   k_cluster_labels   label of every row, size of every cluster, the keep flag of the decision, C
//   rocPRIM, k_filter_compact   (gicp_filter.hip) as for the crop: survivors in their order, exact bounds, M
//
// The forest.  parent[x] <= x always; a root is a row with parent[x] == x.  A hook is one compare-and-swap on a ROOT,
// hi -> lo with lo < hi, so a tree's root is the smallest row of the tree and, once the kernel has ended, of the
// component.  A row that has stopped being a root never becomes one again and its parent is only ever replaced by an
// ancestor of it (path halving), so whatever value a lane reads from parent[x] -- fresh or stale, the loads are
// relaxed and may be served by another XCD's L2 -- is x itself or an ancestor of x.  No lane waits for another lane's
// store: a failed compare-and-swap returns the parent that made it fail, and the lane goes on from there.  Every loop
// is bounded by the data: a parent chain strictly decreases, and the larger root of a retried hook strictly decreases.
// The partition, the roots, the sizes and so every output are integers that do not depend on the schedule: the output
// is bit-identical from call to call, from context to context, and to the host's.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include "gicp_cluster.h"
#include "gicp_internal.h"
#include "gicp_runs_dev.h"

namespace gicp {

// gicp_filter.hip
hipError_t launch_grid_sort(const VoxelArgs&, double*, hipStream_t);
hipError_t launch_flag_scan(const int32_t*, int32_t*, int64_t, void*, size_t, hipStream_t);
hipError_t launch_filter_compact(const double*, int64_t, int, int32_t*, int32_t*, void*, size_t, const int32_t*, double*,
                                 int32_t*, unsigned long long*, hipStream_t);

namespace {

__device__ __forceinline__ int32_t par_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void par_store(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as this lane sees it, halving the path on the way: every row passed is given its
// grandparent, an ancestor.  The chain strictly decreases.
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    int32_t p = par_load(parent + x);
    while (p != x) {
        const int32_t g = par_load(parent + p);
        if (g != p) par_store(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// Unite the trees of rows a and b; returns the root they share afterwards (as far as this lane can tell).  The
// larger root is hooked below the smaller by a compare-and-swap that succeeds only while it still is a root;
// otherwise the swap returns its parent, and the larger of the two roots found from there is smaller than before.
__device__ __forceinline__ int32_t unite(int32_t* parent, int32_t a, int32_t b) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = find_root(parent, old);
        b = find_root(parent, lo);
    }
    return a;
}

__global__ void __launch_bounds__(256) k_cluster_init(int32_t* __restrict__ parent, int32_t* __restrict__ size, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = (int32_t)i;
    size[i] = 0;
}

// One lane per point in key order; the pairs (j, t) with t after j in key order.
template <int D>
__global__ void __launch_bounds__(256) k_cluster_edges(VoxelArgs V, ClusterArgs C) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= V.n) return;
    const uint64_t* __restrict__ ks = V.keys_s;
    const double* __restrict__ pk = C.packed;
    const int32_t* __restrict__ rows = V.idx_s;
    int32_t* parent = C.parent;
    const uint64_t key = ks[j];
    double p[D];
    for (int a = 0; a < D; ++a) p[a] = pk[j * D + a];
    int32_t root = rows[j];   // the root this lane last saw above its row
    neighbour_runs<D, true>(ks, V.n, key, V.bits, C.cmax, [&](int64_t b, int64_t e) {
        for (int64_t t = b > j ? b : j + 1; t < e; ++t) {
            double q[D];
            for (int a = 0; a < D; ++a) q[a] = pk[t * D + a];
            if (!ror_near(filter_d2<D>(p, q), C.r2)) continue;
            const int32_t o = rows[t];
            if (par_load(parent + o) == root) continue;   // both ends already hang below one root
            root = unite(parent, root, o);
        }
        return false;
    });
}

// One lane per row: its root, the root flag, the sizes.
__global__ void __launch_bounds__(256) k_cluster_roots(ClusterArgs C, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    int32_t r = 0;
    if (live) {
        r = (int32_t)i;
        for (int32_t p = par_load(C.parent + r); p != r; p = par_load(C.parent + r)) r = p;   // (strictly decreasing)
        par_store(C.parent + i, r);   // (an ancestor, as every value another lane may read here)
        C.root[i] = r == (int32_t)i ? 1 : 0;
    }
    // One add per wave and distinct root: the lanes that share the root of the first lane still to be counted are
    // counted by that lane, until none is left (at most 64 turns; a cloud that is mostly one cluster would
    // otherwise queue an add per row on one word)
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t r0 = __shfl(r, lead);
        const unsigned long long same = __ballot(live && r == r0) & todo;
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(C.size + r0, (int32_t)__popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(256) k_cluster_labels(ClusterArgs C, int64_t n, unsigned long long* res) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t r = C.parent[i];
    const int32_t c = C.cid1[r] - 1, s = C.size[r];
    C.labels[i] = c;
    if (r == (int32_t)i) C.sizes[c] = s;
    C.keep[i] = cluster_keeps(s, C.min_size, C.max_size) ? 1 : 0;
    if (i == n - 1) res[7] = (unsigned long long)C.cid1[i];   // C (k_filter_compact leaves this word alone)
}

}  // namespace

// Euclidean cluster extraction on `st`: V.raw [n][dim] -> C.labels, C.sizes, C.out [M][dim], C.idx_out, V.res (bounds
// of the kept rows, M in res[6], the number of clusters in res[7]).
hipError_t launch_cluster(const VoxelArgs& V, const ClusterArgs& C, hipStream_t st) {
    clear_foreign_error();
    if (V.n <= 0 || V.n > 0x7FFFFFFFll || (V.dim != 2 && V.dim != 3) || !V.raw || !V.keys_s || !V.idx_s || !V.res || !C.packed ||
        !C.parent || !C.size || !C.root || !C.cid1 || !C.labels || !C.sizes || !C.keep || !C.pos1 || !C.out || C.min_size < 1)
        return hipErrorInvalidValue;
    const int64_t n = V.n;
    const unsigned g = grid256(n);
    hipError_t e = launch_grid_sort(V, C.packed, st);   // (also resets the result words)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cluster_init, dim3(g), dim3(256), 0, st, C.parent, C.size, n);
    if (V.dim == 3) hipLaunchKernelGGL(k_cluster_edges<3>, dim3(g), dim3(256), 0, st, V, C);
    else hipLaunchKernelGGL(k_cluster_edges<2>, dim3(g), dim3(256), 0, st, V, C);
    hipLaunchKernelGGL(k_cluster_roots, dim3(g), dim3(256), 0, st, C, n);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_flag_scan(C.root, C.cid1, n, V.tmp, V.tmp_bytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cluster_labels, dim3(g), dim3(256), 0, st, C, n, V.res);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_filter_compact(V.raw, n, V.dim, C.keep, C.pos1, V.tmp, V.tmp_bytes, nullptr, C.out, C.idx_out, V.res, st);
}

}  // namespace gicp
