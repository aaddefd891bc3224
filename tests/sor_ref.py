"""NumPy restatement of statistical outlier removal (include/gicp_hip.h) and the inputs the SOR tests
share (test_sor_cpu.py, test_gpu_sor.py).

The definition, operation for operation, every one an elementwise fp64 NumPy operation and so rounded on its own:
  mean_i = (sum of sqrt(d2) over the n = min(k, M - 1) smallest d2(p_i, p_j), j != i, ascending, sequential) / n
  T(v)   = pad v with +0.0 to a power of two, replace v by v[0::2] + v[1::2] until one value is left
  mu     = T(mean) / M,  sigma = sqrt(T((mean - mu)^2) / (M - 1)),  thr = mu + std_ratio * sigma (product first)
  keep i iff mean_i <= thr
scipy's cKDTree only proposes k + 8 candidates besides the row itself; d2 is the contract's expression
(knn_ref.d2_rows' arithmetic) and the candidates are sorted by it.  Only the multiset of the n smallest d2 enters, so
the tree's choice among exact ties does not matter; tests/test_sor_cpu.py checks the proposal against the brute force
of knn_ref on the small cases."""
import functools

import numpy as np
from scipy.spatial import cKDTree

import knn_ref as K

EXTRA = 8      # candidates proposed beyond k (and the row itself)


def candidate_d2(points, k):
    """[M, min(k + 1 + EXTRA, M) - 1 or more] ascending d2 of each row's candidate neighbours, the row itself left out
    (+inf in its place, sorted to the end)."""
    M, dim = points.shape
    kq = min(k + 1 + EXTRA, M)
    _, idx = cKDTree(points).query(points, k=kq)
    idx = np.asarray(idx).reshape(M, kq)
    q = points[idx]                                   # [M, kq, dim]
    dx = q[:, :, 0] - points[:, None, 0]
    dy = q[:, :, 1] - points[:, None, 1]
    d2 = dx * dx + dy * dy
    if dim == 3:
        dz = q[:, :, 2] - points[:, None, 2]
        d2 = d2 + dz * dz
    me = idx == np.arange(M)[:, None]
    # a row that is not among its own candidates has kq coincident rows before it: every candidate is at 0, and
    # dropping the last one drops nothing the mean needs
    me[~me.any(axis=1), -1] = True
    d2 = np.where(me, np.inf, d2)
    return np.sort(d2, axis=1)


def mean_distance(points, k):
    """mean_i of every row."""
    M = len(points)
    n = min(k, M - 1)
    d2 = candidate_d2(points, k)
    s = np.zeros(M)
    for m in range(n):
        s = s + np.sqrt(d2[:, m])
    return s / np.float64(n)


def tree_sum(v):
    """T(v)."""
    v = np.asarray(v, dtype=np.float64)
    size = 1
    while size < len(v):
        size *= 2
    v = np.concatenate([v, np.zeros(size - len(v))])
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return np.float64(v[0])


def statistics(mean, std_ratio):
    """(mu, sigma, thr) of the means."""
    M = np.float64(len(mean))
    mu = tree_sum(mean) / M
    dev = mean - mu
    sigma = np.sqrt(tree_sum(dev * dev) / (M - np.float64(1.0)))
    prod = np.float64(std_ratio) * sigma
    return mu, sigma, mu + prod


def sor(points, k, std_ratio):
    """(keep mask [M], mean [M], (mu, sigma, thr)) of the definition."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    mean = mean_distance(points, k)
    mu, sigma, thr = statistics(mean, std_ratio)
    return mean <= thr, mean, (mu, sigma, thr)


# ---- inputs ----

K_LIST = (1, 7, 8, 15, 16, 31)      # both sides of the K = 8 / 16 / 32 instantiations: the query asks for k + 1


def cloud_with_outliers(n, dim, seed):
    """A uniform cloud with every 40th row pushed out by 2 .. 6 cloud widths: some rows go at std_ratio 1."""
    rng = np.random.default_rng([seed, dim, n])
    p = rng.uniform(-10.0, 10.0, (n, dim))
    far = np.arange(0, n, 40)
    p[far] += rng.uniform(40.0, 120.0, (len(far), dim)) * rng.choice([-1.0, 1.0], (len(far), dim))
    return p


def cases(dim):
    """[(name, points, k, std_ratio)]: the cases the host yardstick and the device are both held to."""
    out = []
    for k in K_LIST:      # M = 2, 3, k, k + 1, k + 2: lists shorter than k + 1, exactly k + 1, one more
        for m in sorted({2, 3, k, k + 1, k + 2} - {0, 1}):
            out.append((f"rows_{m}_k{k}", cloud_with_outliers(m, dim, 3), k, 1.0))
    for m in (63, 64, 65, 255, 256, 257):      # the wave and the workgroup of the tree, and one more
        out.append((f"rows_{m}_k8", cloud_with_outliers(m, dim, 4), 8, 1.0))
    base = cloud_with_outliers(4097, dim, 1)      # two tree levels
    for k in K_LIST:
        out.append((f"rows_4097_k{k}", base, k, 1.0))
    for r in (0.0, 0.5, 2.5):
        out.append((f"rows_4097_ratio_{r}", base, 8, r))
    co = K.coincident(dim)      # 70 coincident rows: their means are 0, and a row need not be among its own first k + 1
    for k in (1, 8, 31):
        out.append((f"coincident_k{k}", co, k, 1.0))
    lat = K.lattice(dim)      # ties everywhere
    for k in (2 * dim, 2 * dim + 1, 8, 31):
        out.append((f"lattice_k{k}", lat, k, 1.0))
    return out


def big_cases(dim):
    """Device only (the host yardstick is quadratic): 65 537 rows, three tree levels."""
    return [("rows_65537_k8", cloud_with_outliers(65537, dim, 2), 8, 1.0)]


@functools.lru_cache(maxsize=None)
def case_table(dim, big=False):
    return {c[0]: c for c in cases(dim) + (big_cases(dim) if big else [])}


@functools.lru_cache(maxsize=None)
def expected(dim, name, big=False):
    """The reference's answer of a case, computed once and shared (read only)."""
    _, p, k, r = case_table(dim, big)[name]
    keep, mean, stats = sor(p, k, r)
    keep.setflags(write=False)
    mean.setflags(write=False)
    return keep, mean, stats


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check(call, points, k, std_ratio, want=None, what=""):
    """One call of gicp.sor_points / gicp.sor_points_host held to the reference, bit for bit: rows, index, mean, mu,
    sigma, thr."""
    keep, mean, (mu, sigma, thr) = want if want is not None else sor(points, k, std_ratio)
    rows, idx, got_mean, st = call(points, k, std_ratio, return_index=True, return_mean=True, return_stats=True)
    assert same_bits(got_mean, mean), (what, "mean", np.argwhere(got_mean != mean)[:5])
    got = np.array([st["mu"], st["sigma"], st["threshold"]])
    assert same_bits(got, np.array([mu, sigma, thr])), (what, "mu, sigma, thr", got, (mu, sigma, thr))
    assert same_bits(idx, np.nonzero(keep)[0].astype(np.int64)), (what, "kept rows")
    assert same_bits(rows, np.ascontiguousarray(points[keep])), (what, "rows")


ULP_SEARCH = 64      # rows above mu looked at for a threshold that hits the row's mean exactly


@functools.lru_cache(maxsize=None)
def ulp_trio(dim, name, big=False):
    """(row j, the three std_ratio values, hit) of a case, or None where the case has no such row: std_ratio =
    (mean_j - mu) / sigma and its two floating-point neighbours, for a row j above mu.  Among the first ULP_SEARCH such
    rows the first whose own mean one of the three thresholds equals is taken (hit = True: the run in which the
    inclusive bound decides row j); without one, the first row above mu.  None only where sigma is 0 or no mean lies
    above mu (two rows, all rows coincident)."""
    _, mean, (mu, sigma, _) = expected(dim, name, big)
    if not sigma > 0:
        return None
    first = None
    for j in np.nonzero(mean > mu)[0][:ULP_SEARCH]:
        r0 = (mean[j] - mu) / sigma
        trio = (np.nextafter(r0, 0.0), r0, np.nextafter(r0, np.inf))
        if not np.all(np.isfinite(trio)):
            continue
        trio = tuple(float(r) for r in trio)
        if any(statistics(mean, r)[2] == mean[j] for r in trio):
            return int(j), trio, True
        if first is None:
            first = (int(j), trio, False)
    return first


def ulp_cases(dim, big=False):
    """The cases the threshold-to-the-ulp tests run: every case of the table that has a row above mu and sigma > 0."""
    return [name for name in case_table(dim, big) if ulp_trio(dim, name, big) is not None]


def check_ulp(dim, name, calls, big=False):
    """The three runs of a case: every call of `calls` (gicp.sor_points, gicp.sor_points_host) keeps the reference's set,
    and where the threshold is mean_j itself row j is kept.  Returns how many runs hit mean_j."""
    _, pts, k, _ = case_table(dim, big)[name]
    _, mean, _ = expected(dim, name, big)
    j, trio, hit = ulp_trio(dim, name, big)
    hits = 0
    for r in trio:
        thr = statistics(mean, r)[2]
        want = np.nonzero(mean <= thr)[0]
        for call in calls:
            _, idx, st = call(pts, k, r, return_index=True, return_stats=True)
            assert st["threshold"] == thr, (name, r, call.__name__)
            assert np.array_equal(idx, want), (name, r, call.__name__)
        if thr == mean[j]:
            hits += 1
            assert j in want
    assert (hits > 0) == hit, name
    return hits


@functools.lru_cache(maxsize=None)
def empty_stage_cloud():
    """Three collinear rows whose means (k = 1) are equal and whose mu = T(mean) / 3 rounds below them: at std_ratio 0
    nothing is kept.  Found by search over the spacing; read only."""
    rng = np.random.default_rng(77)
    for _ in range(2000):
        a = rng.uniform(0.1, 1.0)
        pts = np.array([[0.0, 0.0], [a, 0.0], [2 * a, 0.0]])
        keep, mean, (mu, _, _) = sor(pts, 1, 0.0)
        if not keep.any():
            assert mean[0] == mean[1] == mean[2] and mu < mean[0]
            pts.setflags(write=False)
            return pts
    raise AssertionError("no cloud with equal means and a mu below them among 2000 candidates")


# the fixtures of tests/density_ref.py whose survivors are exactly the core (test_sor_cpu.py asserts it)
CORE_SOR = {"stretched_3d": (8, 1.0), "stretched_2d": (8, 1.0), "offset_origin_3d": (15, 1.0)}
