"""Statistical outlier removal without a GPU: the NumPy restatement (tests/sor_ref.py) against a
brute force of its own candidates, the host yardstick gicp.sor_points_host (gicp_sor_points_host, csrc/gicp_hostmath.cpp
over csrc/gicp_sor.h) against the restatement bit for bit on every case the device is held to, the refusals with the
library's text, and the preconditions of the fixtures the GPU tests build on."""
import ctypes as C

import numpy as np
import pytest

import density_ref as D
import knn_ref as K
import sor_ref as R

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402


def test_bound_entry_points():
    for name in ("gicp_sor_max_k", "gicp_sor_points", "gicp_sor_points_host", "gicp_set_sor"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().gicp_version() >= 107
    assert gicp.sor_max_k() == gicp.knn_max_k() - 1 == 31
    assert "csrc/gicp_sor.hip" in _lib.HASH_SRCS and "csrc/gicp_sor.h" in _lib.HASH_SRCS
    for name in ("sor_points", "sor_points_host", "sor_max_k"):
        assert name in gicp.__all__
    assert C.sizeof(_lib.Sor) == 16


@pytest.mark.parametrize("dim", [2, 3])
def test_the_proposed_candidates_hold_the_nearest_rows(dim):
    """cKDTree's k + 8 candidates against all pairs (knn_ref's brute force, a self-query for k + 1 with entry 0
    dropped): the same d2 lists, ties and coincident rows included."""
    for name in ("rows_257_k8", "rows_9_k8", "rows_3_k31", "coincident_k8", "coincident_k31", "lattice_k31", f"lattice_k{2 * dim}"):
        _, pts, k, _ = R.case_table(dim)[name]
        n = min(k, len(pts) - 1)
        _, d2, cnt = K.knn(pts, None, n + 1)
        assert np.all(cnt == n + 1) and np.all(d2[:, 0] == 0)
        assert R.same_bits(np.ascontiguousarray(R.candidate_d2(pts, k)[:, :n]), np.ascontiguousarray(d2[:, 1:])), name


def test_tree_sum_is_the_pairwise_tree():
    v = np.random.default_rng(5).uniform(0.0, 1.0, 1000)
    assert R.tree_sum(v[:4]) == (v[0] + v[1]) + (v[2] + v[3])
    assert R.tree_sum(v[:3]) == (v[0] + v[1]) + v[2]
    assert R.tree_sum(v[:1]) == v[0]
    # 256 aligned rows first, then the partials: the device's two levels
    part = np.array([R.tree_sum(v[b:b + 256]) for b in range(0, 1000, 256)])
    assert R.tree_sum(v) == R.tree_sum(part)
    assert R.tree_sum(v) != np.cumsum(v)[-1]       # (the sequential sum differs: the order is pinned, not incidental)


def _cases():
    return [(dim, name) for dim in (2, 3) for name in R.case_table(dim)]


@pytest.mark.parametrize("dim,name", _cases())
def test_host_yardstick_equals_the_reference(dim, name):
    _, pts, k, ratio = R.case_table(dim)[name]
    R.check(gicp.sor_points_host, pts, k, ratio, R.expected(dim, name), name)


def test_the_cases_remove_and_keep():
    """The tables are not vacuous: the 4 097-row cloud loses its outliers and only them at std_ratio 1, the coincident
    rows have mean 0, the lattice ties."""
    keep, mean, _ = R.expected(3, "rows_4097_k8")
    far = np.zeros(4097, dtype=bool)
    far[::40] = True
    assert np.array_equal(~keep, far)
    co = K.coincident(3)
    keep, mean, _ = R.expected(3, "coincident_k31")
    assert np.all(mean[np.all(co == 0.375, axis=1)] == 0) and 0 < keep.sum() < len(co)
    _, mean, _ = R.expected(3, "lattice_k6")
    assert np.all(mean[np.all((K.lattice(3) > 0) & (K.lattice(3) < 5), axis=1)] == 1.0)


def _ulp_cases():
    return [(dim, name) for dim in (2, 3) for name in R.ulp_cases(dim)]


@pytest.mark.parametrize("dim,name", _ulp_cases())
def test_threshold_to_the_ulp_on_the_host(dim, name):
    """Per case: std_ratio = (mean_j - mu) / sigma for a row j above mu, and its two floating-point neighbours.  Host
    and reference agree on the kept set in all three, and where a threshold is mean_j itself row j is kept (the bound
    is inclusive)."""
    R.check_ulp(dim, name, [gicp.sor_points_host])


def test_the_ulp_cases_leave_out_only_what_has_no_such_row():
    """Every case of the table runs, but those with sigma = 0 or no mean above mu: two rows, or k = 1 on three; and
    most cases have a run whose threshold is the row's own mean."""
    for dim in (2, 3):
        out = sorted(set(R.case_table(dim, True)) - set(R.ulp_cases(dim, True)))
        for name in out:
            _, mean, (mu, sigma, _) = R.expected(dim, name, True)
            assert sigma == 0 or not np.any(mean > mu), name
        assert all(name.startswith("rows_2_") for name in out), out
        hit = [name for name in R.ulp_cases(dim, True) if R.ulp_trio(dim, name, True)[2]]
        assert len(hit) >= 30 and "rows_65537_k8" in hit and any(n.startswith("coincident") for n in hit), (dim, len(hit))


def test_null_outputs_and_exact_sizes():
    lib = _lib.load()
    pts = R.cloud_with_outliers(300, 3, 9)
    keep, mean, (mu, sigma, thr) = R.sor(pts, 8, 1.0)
    s = _lib.Sor(8, 0, 1.0)
    m = C.c_int64(-1)
    assert lib.gicp_sor_points_host(_lib.dptr(pts), 300, 3, C.byref(s), None, None, None, None, C.byref(m)) == 0
    assert m.value == keep.sum()
    st = np.zeros(3)
    assert lib.gicp_sor_points_host(_lib.dptr(pts), 300, 3, C.byref(s), None, None, None, _lib.dptr(st), C.byref(m)) == 0
    assert R.same_bits(st, np.array([mu, sigma, thr]))


REFUSED = [
    (dict(k=0), "sor: k must be 1..gicp_sor_max_k()"),
    (dict(k=32), "sor: k must be 1..gicp_sor_max_k()"),
    (dict(k=-1), "sor: k must be 1..gicp_sor_max_k()"),
    (dict(std_ratio=-0.5), "sor: std_ratio must be finite and >= 0"),
    (dict(std_ratio=np.inf), "sor: std_ratio must be finite and >= 0"),
    (dict(std_ratio=np.nan), "sor: std_ratio must be finite and >= 0"),
    (dict(points=np.zeros((1, 3))), "sor: statistical outlier removal needs at least 2 rows"),
    (dict(points=np.array([[0.0, 1.0, np.nan], [0.0, 0.0, 0.0]])), "non-finite"),
    # d2 overflows: every mean is +inf
    (dict(points=np.array([[1e200, 0.0, 0.0], [-1e200, 0.0, 0.0], [0.0, 1e200, 0.0]])), "sor: the squared extent of the rows is not finite"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
def test_host_refusals_carry_the_library_text(kw, text):
    args = dict(points=R.cloud_with_outliers(50, 3, 1), k=4, std_ratio=1.0)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        gicp.sor_points_host(args["points"], args["k"], args["std_ratio"])
    assert text in str(e.value) and str(e.value).startswith("gicp_sor_points_host: ")


def test_a_stage_that_leaves_no_row_is_refused():
    """Equal means whose tree sum, divided by M, rounds below them (sor_ref.empty_stage_cloud finds one by search)."""
    with pytest.raises(ValueError, match="sor: statistical outlier removal removed all 3 points"):
        gicp.sor_points_host(R.empty_stage_cloud(), 1, 0.0)


def test_a_refused_host_call_writes_nothing():
    lib = _lib.load()
    pts = R.cloud_with_outliers(20, 3, 1).copy()
    pts[7, 1] = np.inf
    out = np.full((20, 3), 7.5)
    idx = np.full(20, 77, dtype=np.int64)
    mean = np.full(20, 7.5)
    st = np.full(3, 7.5)
    m = C.c_int64(5)
    s = _lib.Sor(4, 0, 1.0)
    rc = lib.gicp_sor_points_host(_lib.dptr(pts), 20, 3, C.byref(s), _lib.dptr(out), idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                  _lib.dptr(mean), _lib.dptr(st), C.byref(m))
    assert rc == _lib.GICP_E_INVALID and b"non-finite" in lib.gicp_last_host_error()
    assert np.all(out == 7.5) and np.all(idx == 77) and np.all(mean == 7.5) and np.all(st == 7.5)


@pytest.mark.parametrize("name", sorted(R.CORE_SOR))
def test_fixture_survivors_are_the_core(name):
    """What the fused-build tests of test_gpu_sor.py rest on: both clouds of the fixture come out as the core alone,
    and every row's mean lies at least 0.9 thr away from thr, so no decision is near its bound."""
    f = D.fixture(name)
    k, ratio = R.CORE_SOR[name]
    for which in ("source", "target"):
        keep, mean, (mu, sigma, thr) = R.sor(f[which], k, ratio)
        assert np.array_equal(keep, f["core_" + which]), (name, which, keep.sum())
        assert np.all(np.abs(mean - thr) >= 0.9 * thr), (name, which)


def test_a_clump_larger_than_k_survives():
    """offset_origin_3d at k = 8: the 12 returns about the origin are each other's neighbours, so k must exceed the
    size of the clump (the one-shot parity case of the GPU tests)."""
    f = D.fixture("offset_origin_3d")
    keep, mean, (mu, _, _) = R.sor(f["source"], 8, 1.0)
    assert len(f["source"]) == 8012 and keep.sum() == 6752 and abs(mu - 0.858) < 5e-4
    assert keep[~f["core_source"]].all()
    R.check(gicp.sor_points_host, f["source"], 8, 1.0, (keep, mean, R.statistics(mean, 1.0)), "offset_origin_3d_k8")
