"""Euclidean cluster extraction without a GPU: the NumPy / SciPy restatement (tests/cluster_ref.py)
against a brute force over all pairs, the host yardstick gicp.cluster_points_host (gicp_cluster_points_host,
csrc/gicp_hostmath.cpp) against the restatement exactly on every case the device is held to, the refusals with the
library's text, the identity with radius outlier removal's counts, and the preconditions of the fixtures the GPU tests
build on."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import cKDTree

import cluster_ref as R
import density_ref as D
import filter_ref as F

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402


def test_bound_entry_points():
    for name in ("gicp_cluster_points", "gicp_cluster_points_host", "gicp_set_cluster"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().gicp_version() >= 108
    for name in ("csrc/gicp_cluster.hip", "csrc/gicp_cluster.h", "csrc/gicp_runs_dev.h"):
        assert name in _lib.HASH_SRCS
    for name in ("cluster_points", "cluster_points_host"):
        assert name in gicp.__all__
    assert C.sizeof(_lib.Cluster) == 16


SMALL = ("n1", "n2", "n65", "n257", "n1025", "diagonal_pairs", "key_runs", "coincident", "duplicates")


@pytest.mark.parametrize("dim", [2, 3])
def test_the_reference_equals_a_brute_force_over_all_pairs(dim):
    for name in SMALL:
        pts, radius, _, _ = R.cases(dim)[name]
        labels, sizes, _ = R.expected(dim, name)
        bl, bs = R.brute(pts, radius)
        assert R.same_bits(labels, bl) and R.same_bits(sizes, bs), name


def _cases():
    return [(dim, name) for dim in (2, 3) for name in R.cases(dim)]


@pytest.mark.parametrize("dim,name", _cases())
def test_host_yardstick_equals_the_reference(dim, name):
    pts, radius, lo, hi = R.cases(dim)[name]
    R.check(gicp.cluster_points_host, pts, radius, lo, hi, R.expected(dim, name), name)


def test_the_cases_say_what_they_are_meant_to():
    """The table is not vacuous."""
    for dim in (2, 3):
        for name in ("chain_4097", "chain_4097_random", "chain_4097_snake"):
            assert list(R.expected(dim, name)[1]) == [4097], name
        assert list(R.expected(dim, "chain_16385")[1]) == [16385]
        assert np.all(R.expected(dim, "chain_4097_below")[1] == 1) and len(R.expected(dim, "chain_4097_below")[1]) == 4097
        assert sorted(R.expected(dim, "chain_two")[1]) == [2048, 2049]
        nd = 3 ** dim - 1
        sizes = R.expected(dim, "diagonal_pairs")[1]
        assert np.sum(sizes == 2) == nd and np.sum(sizes == 1) == 2 * nd and len(sizes) == 3 * nd
        assert 70 in R.expected(dim, "coincident")[1]
        assert list(R.expected(dim, "lattice")[1]) == [25 ** dim] and np.all(R.expected(dim, "lattice_below")[1] == 1)
        for n in (257, 4097, 65537):      # singletons, small clusters and large ones side by side
            sizes = R.expected(dim, f"n{n}")[1]
            assert np.sum(sizes == 1) > n // 100 and np.sum((sizes > 1) & (sizes < 10)) > n // 100 and sizes.max() >= 50, (n, dim)
        # the chains' smallest row sits far from most of its component
        for order in ("random", "snake"):
            p = R.chain(4097, dim, order)
            assert np.abs(p[:, 0] - p[0, 0]).mean() > 1000 * R.STEP, order


@pytest.mark.parametrize("dim", [2, 3])
def test_a_permutation_permutes_the_partition(dim):
    pts, radius, _, _ = R.cases(dim)["n4097"]
    labels, sizes, _ = R.expected(dim, "n4097")
    perm = np.random.default_rng([7, dim]).permutation(len(pts))
    p2 = np.ascontiguousarray(pts[perm])
    _, l2, s2 = gicp.cluster_points_host(p2, radius, return_labels=True, return_sizes=True)
    # the same partition: rows share a label after iff they did before; the numbering follows the new smallest rows
    back = np.empty_like(l2)
    back[perm] = l2
    pairs = np.unique(np.stack([labels, back], 1), axis=0)
    assert len(pairs) == len(sizes) == len(s2)
    assert R.same_bits(s2[pairs[:, 1]], sizes[pairs[:, 0]])
    first = np.full(len(s2), len(l2))
    np.minimum.at(first, l2, np.arange(len(l2)))
    assert np.all(np.diff(first) > 0)
    R.check(gicp.cluster_points_host, p2, radius, 2, 0, None, "permuted")


@pytest.mark.parametrize("dim", [2, 3])
def test_decision_on_either_side_of_a_size(dim):
    pts, radius, _, _ = R.cases(dim)["n4097"]
    labels, sizes, _ = R.expected(dim, "n4097")
    s = int(np.sort(np.unique(sizes))[len(np.unique(sizes)) // 2])      # an existing size, neither the smallest nor the largest
    for lo, hi in ((s, 0), (s + 1, 0), (1, s), (1, s - 1), (s, s), (2, s), (int(sizes.max()), 0), (1, 1)):
        rows, idx = gicp.cluster_points_host(pts, radius, lo, hi, return_index=True)
        want = np.flatnonzero(R.keeps(sizes, lo, hi)[labels])
        assert np.array_equal(idx, want) and len(want) > 0, (lo, hi)
        assert R.same_bits(rows, np.ascontiguousarray(pts[want]))
    with pytest.raises(ValueError, match=r"cluster: none of the \d+ clusters of the 4097 points has a size in"):
        gicp.cluster_points_host(pts, radius, int(sizes.max()) + 1, 0)


@pytest.mark.parametrize("dim", [2, 3])
def test_singletons_are_the_rows_radius_outlier_removal_counts_zero(dim):
    for name in ("n4097", "key_runs", "duplicates", "diagonal_pairs"):
        pts, radius, _, _ = R.cases(dim)[name]
        _, labels, sizes = gicp.cluster_points_host(pts, radius, return_labels=True, return_sizes=True)
        _, counts = gicp.filter_points_host(pts, radius=radius, min_neighbors=1, return_counts=True)
        assert np.array_equal(counts == 0, sizes[labels] == 1), name


def test_null_outputs():
    lib = _lib.load()
    pts, radius, lo, hi = R.cases(3)["n257"]
    labels, sizes, keep = R.expected(3, "n257")
    c = _lib.Cluster(radius, lo, hi)
    assert lib.gicp_cluster_points_host(_lib.dptr(pts), 257, 3, C.byref(c), None, None, None, None, None, None) == 0
    m, nc = C.c_int64(-1), C.c_int64(-1)
    assert lib.gicp_cluster_points_host(_lib.dptr(pts), 257, 3, C.byref(c), None, None, C.byref(nc), None, None, C.byref(m)) == 0
    assert m.value == keep.sum() and nc.value == len(sizes)


REFUSED = [
    (dict(radius=0.0), "cluster: radius must be finite and > 0"),
    (dict(radius=-1.0), "cluster: radius must be finite and > 0"),
    (dict(radius=np.inf), "cluster: radius must be finite and > 0"),
    (dict(radius=np.nan), "cluster: radius must be finite and > 0"),
    (dict(min_size=0), "cluster: min_size must be >= 1"),
    (dict(min_size=5, max_size=4), "cluster: max_size 4 must be 0 (no upper limit) or at least min_size 5"),
    (dict(max_size=-1), "cluster: max_size -1 must be 0"),
    (dict(points=np.array([[0.0, 1.0, np.nan], [0.0, 0.0, 0.0]])), "cluster: cloud contains non-finite coordinates"),
    (dict(points=np.array([[0.0, 0.0, 0.0], [0.0, 3e6, 0.0]])), "cluster: radius grid too wide: axis y spans"),
    (dict(points=np.array([[1e12, 0.0, 0.0], [1e12, 1.0, 0.0]])), "cluster: axis x lies beyond 2^35 cells of edge radius = 1"),
    (dict(min_size=60), "cluster: none of the"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
def test_host_refusals_carry_the_library_text(kw, text):
    args = dict(points=R.mix_cloud(50, 3), radius=1.0, min_size=1, max_size=0)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        gicp.cluster_points_host(args["points"], args["radius"], args["min_size"], args["max_size"])
    assert str(e.value).startswith("gicp_cluster_points_host: " + text), str(e.value)


def test_row_counts_and_null_arguments_are_refused():
    lib = _lib.load()
    pts = R.mix_cloud(20, 3)
    c = _lib.Cluster(1.0, 1, 0)
    m = C.c_int64(5)
    for n, dim, cp, text in ((0, 3, C.byref(c), b"cluster: the cloud must hold 1 .."), (-3, 3, C.byref(c), b"cluster: the cloud must hold 1 .."),
                             (2 ** 31, 3, C.byref(c), b"cluster: the cloud must hold 1 .."), (20, 4, C.byref(c), b"cluster: the cloud must be an N x 2 or N x 3"),
                             (20, 3, None, b"cluster: the setting must not be NULL")):
        rc = lib.gicp_cluster_points_host(_lib.dptr(pts), n, dim, cp, None, None, None, None, None, C.byref(m))
        assert rc == _lib.GICP_E_INVALID and lib.gicp_last_host_error().startswith(b"gicp_cluster_points_host: " + text)
        assert m.value == 5


@pytest.mark.parametrize("dim", [2, 3])
def test_widest_span_is_taken_and_the_next_refused(dim):
    with pytest.raises(ValueError, match=r"cluster: radius grid too wide: axis x spans .* cells of edge radius = 1 "):
        gicp.cluster_points_host(F.widest(dim, extra=1), 1.0)


def test_a_refused_host_call_writes_nothing():
    lib = _lib.load()
    pts = R.mix_cloud(20, 3).copy()
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    for bad, c in ((True, _lib.Cluster(1.0, 1, 0)), (False, _lib.Cluster(1.0, 21, 0))):     # non-finite input; nothing kept
        p = pts.copy()
        if bad:
            p[7, 1] = np.inf
        out = np.full((20, 3), 7.5)
        idx = np.full(20, 77, dtype=np.int64)
        labels = np.full(20, 77, dtype=np.int32)
        sizes = np.full(20, 77, dtype=np.int32)
        m, nc = C.c_int64(5), C.c_int64(5)
        rc = lib.gicp_cluster_points_host(_lib.dptr(p), 20, 3, C.byref(c), labels.ctypes.data_as(i32), sizes.ctypes.data_as(i32),
                                          C.byref(nc), _lib.dptr(out), idx.ctypes.data_as(i64), C.byref(m))
        assert rc == _lib.GICP_E_INVALID and b"cluster: " in lib.gicp_last_host_error()
        assert np.all(out == 7.5) and np.all(idx == 77) and np.all(labels == 77) and np.all(sizes == 77)
        assert m.value == 5 and nc.value == 5


@pytest.mark.parametrize("name", sorted(R.CORE_CLUSTER))
def test_fixture_survivors_are_the_core(name):
    """What the fused-build tests of test_gpu_cluster.py rest on: at radius 3.0 both clouds of the fixture are one
    component of 8 000 rows, the core, plus 12 singletons (stretched_3d) or one component of 12 (offset_origin_3d), so
    min_size 13 leaves exactly the core rows test_gpu_filter.py builds from; no decision is near its bound."""
    f = D.fixture(name)
    radius, lo, hi = R.CORE_CLUSTER[name]
    for which in ("source", "target"):
        labels, sizes, keep = R.cluster(f[which], radius, lo, hi)
        assert np.array_equal(keep, f["core_" + which]), (name, which, int(keep.sum()))
        assert sorted(sizes) == ([1] * 12 + [8000] if name == "stretched_3d" else [12, 8000]), (name, which)
        tree = cKDTree(f[which])      # no pair within 1e-7 of the bound
        assert tree.count_neighbors(tree, radius * (1 + 1e-7)) == tree.count_neighbors(tree, radius * (1 - 1e-7))
        rows, idx = gicp.cluster_points_host(f[which], radius, lo, hi, return_index=True)
        assert np.array_equal(idx, np.flatnonzero(f["core_" + which]))
        assert R.same_bits(rows, np.ascontiguousarray(f[which][f["core_" + which]]))
