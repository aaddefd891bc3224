"""NumPy brute force of the k-nearest-neighbour contract (include/gicp_hip.h) and the inputs the kNN
tests share (test_knn_cpu.py, test_gpu_knn.py).

The contract, restated operation for operation: d2(q, p) = ((dx*dx + dy*dy) + dz*dz) in fp64 with dx = p_x - q_x,
each product and sum rounded on its own (NumPy's elementwise arithmetic does exactly that), the z term dropped in
2-D; the rows of the database are ordered by (d2, original index) -- np.lexsort((index, d2)) -- and the first k of
them within max_distance (d2 <= max_distance * max_distance, inclusive; None: no limit) are the answer, padded with
index -1 and d2 +inf."""
import functools

import numpy as np

CHUNK_PAIRS = 1 << 24      # pairs per block of the distance matrix (128 MB of fp64)


def d2_rows(points, queries):
    """[Q, M] squared distances, the contract's expression."""
    dx = points[None, :, 0] - queries[:, None, 0]
    dy = points[None, :, 1] - queries[:, None, 1]
    d2 = dx * dx + dy * dy
    if points.shape[1] == 3:
        dz = points[None, :, 2] - queries[:, None, 2]
        d2 = d2 + dz * dz
    return d2


def knn(points, queries=None, k=1, max_distance=None):
    """(index [Q, k] int64, d2 [Q, k] float64, count [Q] int32) of the contract.  Per query the rows are ordered by
    np.lexsort((index, d2)); only the rows up to the k-th smallest d2 enter the sort (every row of the answer is
    among them, ties included), which keeps a 262 209-row database affordable."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    queries = points if queries is None else np.ascontiguousarray(queries, dtype=np.float64)
    M, Q = len(points), len(queries)
    lim = np.inf if max_distance is None or max_distance == 0 else np.float64(max_distance) * np.float64(max_distance)
    idx = np.full((Q, k), -1, dtype=np.int64)
    out = np.full((Q, k), np.inf)
    cnt = np.zeros(Q, dtype=np.int32)
    step = max(1, CHUNK_PAIRS // M)
    kk = min(k, M)
    for lo in range(0, Q, step):
        d2 = d2_rows(points, queries[lo:lo + step])
        kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        for r in range(len(d2)):
            cand = np.nonzero((d2[r] <= kth[r]) & (d2[r] <= lim))[0]
            order = cand[np.lexsort((cand, d2[r, cand]))][:k]
            n = len(order)
            idx[lo + r, :n] = order
            out[lo + r, :n] = d2[r, order]
            cnt[lo + r] = n
    return idx, out, cnt


def has_exact_tie(points, queries, k):
    """True if, for some query, two of its k + 1 nearest rows are at exactly the same d2 (the order among the first
    k, or the choice of the k-th, then rests on the index rule)."""
    _, d2, _ = knn(points, queries, min(k + 1, len(points)))
    return bool(np.any(np.diff(d2, axis=1) == 0))


# ---- inputs ----

def random_cloud(n, dim, seed, scale=10.0):
    return np.random.default_rng([seed, dim, n]).uniform(-scale, scale, (n, dim))


def lattice(dim, side=6, seed=11):
    """The integer lattice {0 .. side-1}^dim in shuffled row order: index order differs from Morton order."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), -1).reshape(-1, dim).astype(np.float64)
    return g[np.random.default_rng([seed, dim]).permutation(len(g))]


def lattice_queries(dim, side=6):
    """Lattice points, edge midpoints (2 equidistant rows) and cell centres (2^dim equidistant rows), inside and
    on the rim of the lattice."""
    pts = np.array([[0] * dim, [2] * dim, [side - 1] * dim, [1, 3, 2][:dim]], dtype=np.float64)
    mids = np.array([[0.5] + [0] * (dim - 1), [2] * (dim - 1) + [2.5], [side - 1.5] + [side - 1] * (dim - 1)])
    cent = np.array([[0.5] * dim, [2.5] * dim, [side - 1.5] * dim, [1.5, 3.5, 0.5][:dim]])
    return np.concatenate([pts, mids, cent])


def coincident(dim, copies=70, seed=12):
    """70 coincident rows (more than a tile) scattered by a shuffle among 90 others, some of them coincident pairs."""
    rng = np.random.default_rng([seed, dim])
    other = rng.integers(-8, 9, (90, dim)).astype(np.float64) * 0.25
    pts = np.concatenate([np.tile(np.full((1, dim), 0.375), (copies, 1)), other])
    return pts[rng.permutation(len(pts))]


@functools.lru_cache(maxsize=None)
def big_cloud(dim):
    """262 209 rows: more than 4 096 tiles, so a second super-block of the box hierarchy."""
    return random_cloud(262209, dim, 21, scale=50.0)


def cases(dim, max_k=32, big=False):
    """[(name, points, queries or None, k, max_distance or None)]: the cases the host yardstick and the device are
    both held to.  big: also the 262 209-row database (200 queries)."""
    out = []
    base = random_cloud(4097, dim, 1)
    # query counts at the wave and workgroup edges; databases of more than one block of 64 tiles
    for q in (1, 63, 64, 65, 257):
        out.append((f"queries_{q}", base, random_cloud(q, dim, 100 + q, scale=12.0), 8, None))
    # k: 1, 2, 8, 20, max_k and the instantiation boundaries 1 | 8 | 16 | 32 with their neighbours
    for k in (1, 2, 7, 8, 9, 15, 16, 17, 20, max_k - 1, max_k):
        out.append((f"k_{k}", base, random_cloud(65, dim, 7), k, None))
    # database sizes: 1 row, k - 1 / k / k + 1 rows (pads and count), one tile and two
    for k in (2, 8, max_k):
        for m in sorted({1, k - 1, k, k + 1, 64, 65}):
            out.append((f"rows_{m}_k{k}", random_cloud(m, dim, 3), random_cloud(9, dim, 4), k, None))
            out.append((f"self_rows_{m}_k{k}", random_cloud(m, dim, 3), None, k, None))
    out.append(("self_4097", base, None, 8, None))
    # exact ties: the shuffled lattice, k below / at / above the shell sizes 2, 2^dim, and 1 + 2 dim at a point
    lat, lq = lattice(dim), lattice_queries(dim)
    shell = 2 ** dim
    for k in sorted({1, 2, 3, shell - 1, shell, shell + 1, 2 * dim, 2 * dim + 1, 2 * dim + 2, 20}):
        out.append((f"lattice_k{k}", lat, lq, k, None))
    out.append(("lattice_self", lat, None, 2 * dim + 2, None))
    co = coincident(dim)
    out.append(("coincident_k32", co, np.concatenate([co[:5], random_cloud(6, dim, 5, scale=2.0)]), max_k, None))
    out.append(("coincident_self", co, None, max_k, None))
    out.append(("coincident_k1", co, None, 1, None))
    # max_distance: exactly on the bound (kept), one ulp below (dropped), a radius that leaves queries empty
    out.append(("lattice_r1", lat, lq, 2 * dim + 2, 1.0))
    out.append(("lattice_r1_below", lat, lq, 2 * dim + 2, float(np.nextafter(1.0, 0.0))))
    out.append(("lattice_r_half", lat, lq, 4, 0.5))
    out.append(("radius_some_empty", base, random_cloud(257, dim, 8, scale=14.0), 8, 0.9))
    out.append(("radius_k1", base, random_cloud(257, dim, 8, scale=14.0), 1, 0.9))
    # bad geometry: a query 1e6 away with no limit; queries outside the database's Morton frame
    far = random_cloud(70, dim, 9)
    far[3] += 1e6
    out.append(("far_query", base, far, 8, None))
    out.append(("outside_frame", base, random_cloud(130, dim, 10) + 35.0, 16, None))
    out.append(("outside_frame_r", base, random_cloud(130, dim, 10) * 3.0, 2, 6.0))
    if big:
        out.append(("big_262209", big_cloud(dim), random_cloud(200, dim, 22, scale=55.0), 8, None))
        out.append(("big_262209_k1", big_cloud(dim), random_cloud(200, dim, 23, scale=55.0), 1, None))
    return out


@functools.lru_cache(maxsize=None)
def case_table(dim, big=False):
    return {c[0]: c for c in cases(dim, big=big)}


@functools.lru_cache(maxsize=None)
def expected(dim, name, big=False):
    """The reference's answer of a case, computed once and shared (read only)."""
    _, p, q, k, r = case_table(dim, big)[name]
    res = knn(p, q, k, r)
    for a in res:
        a.setflags(write=False)
    return res


def same_bits(got, want):
    """The comparison of every kNN test: bit for bit."""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
