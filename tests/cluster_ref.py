"""NumPy / SciPy restatement of Euclidean cluster extraction (include/gicp_hip.h) and the inputs the
cluster tests share (test_cluster_cpu.py, test_gpu_cluster.py).

The definition: rows i != j are adjacent iff d2(p_i, p_j) <= radius * radius, d2 = ((dx*dx + dy*dy) + dz*dz) in fp64 with
every product and sum rounded on its own (filter_ref.d2, elementwise NumPy operations) and the squared radius one rounded
product; the clusters are the connected components, numbered in ascending order of their smallest row; a cluster is kept
iff min_size <= size and (max_size == 0 or size <= max_size).  scipy's cKDTree only PROPOSES candidate pairs, within
radius (1 + 1e-6); the expression decides, so the partition is exact.  tests/test_cluster_cpu.py checks it against a
brute force over all pairs on the small cases."""
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import filter_ref as F
import knn_ref as K


def edges(points, radius):
    """[E, 2] the adjacent pairs (i < j) of the definition."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    if len(p) < 2:
        return np.zeros((0, 2), dtype=np.int64)
    pairs = cKDTree(p).query_pairs(radius * (1.0 + 1e-6), output_type="ndarray")
    near = F.d2(p[pairs[:, 0]], p[pairs[:, 1]]) <= np.float64(radius) * np.float64(radius)
    return pairs[near].astype(np.int64)


def number(comp):
    """Component ids of any kind -> (labels int32 numbered by smallest row, sizes int32)."""
    _, first, inv = np.unique(comp, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    labels = rank[inv].astype(np.int32)
    return labels, np.bincount(labels).astype(np.int32)


def keeps(sizes, min_size, max_size):
    return (sizes >= min_size) & ((max_size == 0) | (sizes <= max_size))


def cluster(points, radius, min_size=1, max_size=0):
    """(labels [N] int32, sizes [C] int32, keep mask [N]) of the definition."""
    n = len(points)
    e = edges(points, radius)
    g = coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    labels, sizes = number(comp)
    return labels, sizes, keeps(sizes, min_size, max_size)[labels]


def brute(points, radius):
    """(labels, sizes) by a union-find over ALL pairs: quadratic, for the small cases."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    n = len(p)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    r2 = np.float64(radius) * np.float64(radius)
    for i in range(n - 1):
        for j in np.flatnonzero(F.d2(p[i + 1:], p[i][None, :]) <= r2) + i + 1:
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return number(np.array([find(i) for i in range(n)]))


# ---- inputs ----

SIZES = (1, 2, 63, 64, 65, 255, 256, 257)          # the wave and workgroup edges of one-lane-per-row kernels
# near the percolation threshold of the clouds below (their density does not depend on n): singletons, small clusters
# and clusters of hundreds of rows side by side
MIX_RADIUS = {3: 1.7, 2: 1.15}
STEP = 2.0 ** -3                                   # the chains' spacing: d2 == radius^2 exactly at radius 2^-3
EDGE = 1.0 + 2.0 ** -16                            # the device's cell edge at radius 1 (gicp_filter.h kRorEdge)


def mix_cloud(n, dim):
    return F._cloud(n, dim, n) * (n / 64.0) ** (1.0 / dim)


def chain(n, dim, order="line"):
    """n rows on a line along x from -100, spacing 2^-3 (every coordinate exact), in the given row order."""
    pos = np.arange(n)
    if order == "random":       # the smallest row sits far from most of its component
        pos = np.random.default_rng([41, n]).permutation(n)
    elif order == "snake":      # even positions ascending, then odd positions descending
        pos = np.concatenate([pos[0::2], pos[1::2][::-1]])
    p = np.zeros((n, dim))
    p[:, 0] = -100.0 + pos * STEP
    p[:, 1] = 3.0
    return p


def two_chains(n, dim):
    """Two chains interleaved row by row, 1.0 (more than the radius) apart on y."""
    p = chain(n, dim)
    p[:, 0] = -100.0 + (np.arange(n) // 2) * STEP
    p[1::2, 1] += 1.0
    return p


def _directions(dim):
    return [np.array(d) for d in np.ndindex(*([3] * dim)) if any(v != 1 for v in d)]


def diagonal_pairs(dim):
    """For each of the 26 (8) directions d: a pair 0.4 |d| cell edges apart in the cells c and c + d, and a pair
    1.1 |d| apart in the cells c and c + 2 d, which must never be linked; the groups far from one another, about the
    origin (negative cells included).  Radius 1."""
    out = []
    for k, d3 in enumerate(_directions(dim)):
        d = d3 - 1.0
        base = np.full(dim, -40.0) + 10.0 * np.array(np.unravel_index(k, [3] * dim))
        out += [(base + 0.5 + 0.3 * d) * EDGE, (base + d + 0.5 - 0.3 * d) * EDGE]
        far = base + 4.0
        out += [(far + 0.5 + 0.45 * d) * EDGE, (far + 2.0 * d + 0.5 - 0.45 * d) * EDGE]
    pts = np.array(out)
    return pts[np.random.default_rng(23).permutation(len(pts))]


def coincident(dim):
    """70 coincident rows among 40 others: one cluster of 70 at any radius."""
    return K.coincident(dim)


@functools.lru_cache(maxsize=None)
def cases(dim):
    """{name: (points, radius, min_size, max_size)}: the cases the host function and the device are both held to."""
    out = {}
    for n in SIZES + F.BLOCK_EDGES:
        out[f"n{n}"] = (mix_cloud(n, dim), MIX_RADIUS[dim], 1 if n < 3 else 2, 0)
    below = float(np.nextafter(STEP, 0.0))
    out["chain_4097"] = (chain(4097, dim), STEP, 1, 0)                       # one component: the bound is inclusive
    out["chain_4097_below"] = (chain(4097, dim), below, 1, 0)                # 4 097 singletons
    out["chain_4097_random"] = (chain(4097, dim, "random"), STEP, 1, 0)
    out["chain_4097_snake"] = (chain(4097, dim, "snake"), STEP, 1, 0)
    out["chain_two"] = (two_chains(4097, dim), STEP, 1, 0)                   # two components
    out["chain_16385"] = (chain(16385, dim, "random"), STEP, 1, 0)
    out["diagonal_pairs"] = (diagonal_pairs(dim), 1.0, 2, 2)
    out["key_runs"] = (F._key_runs(dim), 1.0, 3, 0)                          # cells at both ends of every axis
    out["coincident"] = (coincident(dim), 1e-3, 70, 70)
    out["duplicates"] = (F._duplicates(dim), 1e-3, 2, 3)
    out["lattice"] = (F._lattice(dim), 0.25, 1, 0)                           # every edge exactly on the bound
    out["lattice_below"] = (F._lattice(dim), float(np.nextafter(0.25, 0.0)), 1, 1)
    out["widest"] = (F.widest(dim), 1.0, 1, 0)                               # the widest grid taken, corners occupied
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(dim, name):
    """The reference's answer of a case, computed once and shared (read only)."""
    pts, radius, lo, hi = cases(dim)[name]
    labels, sizes, keep = cluster(pts, radius, lo, hi)
    for a in (labels, sizes, keep):
        a.setflags(write=False)
    return labels, sizes, keep


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check(call, points, radius, min_size=1, max_size=0, want=None, what=""):
    """One call of gicp.cluster_points / gicp.cluster_points_host held to the reference, exactly: labels, sizes (and so
    C), the kept index and rows; the call with no optional output returns the same rows."""
    labels, sizes, keep = want if want is not None else cluster(points, radius, min_size, max_size)
    rows, idx, got_labels, got_sizes = call(points, radius, min_size, max_size, return_index=True, return_labels=True,
                                            return_sizes=True)
    assert same_bits(got_sizes, sizes), (what, "sizes", len(got_sizes), len(sizes))
    assert same_bits(got_labels, labels), (what, "labels", np.flatnonzero(got_labels != labels)[:5])
    assert same_bits(idx, np.flatnonzero(keep).astype(np.int64)), (what, "kept rows")
    assert same_bits(rows, np.ascontiguousarray(points[keep])), (what, "rows")
    assert same_bits(call(points, radius, min_size, max_size), rows), (what, "rows alone")


# the setting that leaves exactly the core on both clouds of these fixtures of tests/density_ref.py
# (test_cluster_cpu.py asserts it): the 12 far returns are singletons (stretched_3d) or one clump of 12 (offset_origin_3d)
CORE_CLUSTER = {"stretched_3d": (3.0, 13, 0), "offset_origin_3d": (3.0, 13, 0)}
