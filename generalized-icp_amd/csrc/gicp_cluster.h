// gicp_cluster.h — Euclidean cluster extraction: the decision, shared by the device kernels
// (gicp_cluster.hip) and the host yardstick (gicp_hostmath.cpp cluster_points_host), and the kernels' arguments.
//
//   edges      i ~ j (i != j) iff ror_near(filter_d2<D>(p_i, p_j), radius^2): gicp_filter.h's functions, called as
//              they are -- fp64, every product and sum rounded on its own, the bound inclusive
//   clusters   the connected components; numbered 0 .. C - 1 in ascending order of their smallest row
//   decision   a cluster is kept iff min_size <= size and (max_size == 0 or size <= max_size)
#pragma once
#include <stdint.h>

#include "gicp_filter.h"

namespace gicp {

__host__ __device__ inline bool cluster_keeps(int32_t size, int32_t min_size, int32_t max_size) {
    return min_size <= size && (max_size == 0 || size <= max_size);
}

// Cluster stage (launch_cluster): V.raw [n][dim] -> out [M][dim], rows in their order.  The cells are those of radius
// outlier removal's grid (leaf = radius kRorEdge); V carries the key layout and the sort's scratch as for launch_ror.
// parent, size, root, cid1 and labels are indexed by the row of V.raw, and a parent is a row: after k_cluster_edges
// every tree's root is its component's smallest row.
struct ClusterArgs {
    int64_t cmax[3];          // highest cell per axis relative to cmin
    double r2;
    int32_t min_size, max_size;
    double* packed;           // [n][dim] scratch: the points in key order
    int32_t* parent;          // [n] scratch: the forest; after k_cluster_roots the root of every row
    int32_t* size;            // [n] scratch: rows per root (0 elsewhere)
    int32_t* root;            // [n] scratch: 1 where the row is a root
    int32_t* cid1;            // [n] scratch: inclusive scan of `root`: cluster number + 1 at a root
    int32_t* labels;          // [n] cluster of every row
    int32_t* sizes;           // [n] rows per cluster, the first C entries
    int32_t* keep;            // [n] scratch: keep flags
    int32_t* pos1;            // [n] scratch: their inclusive scan
    double* out;              // [n][dim]
    int32_t* idx_out;         // [n] row of each kept row (nullable)
};

}  // namespace gicp
