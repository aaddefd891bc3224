"""Exact k-nearest-neighbour queries without a GPU: the NumPy reference of the contract
(tests/knn_ref.py) against scipy's cKDTree where no exact tie is involved, the host yardstick gicp.knn_host
(gicp_knn_host, a brute force in csrc/gicp_hostmath.cpp) against the reference bit for bit on every case the device
is held to, and the refusals with the library's text."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import cKDTree

import knn_ref as K

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402


def test_bound_entry_points():
    for name in ("gicp_knn_max_k", "gicp_knn", "gicp_knn_points", "gicp_knn_host"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().gicp_version() >= 106
    assert gicp.knn_max_k() == 32
    assert "csrc/gicp_knn.hip" in _lib.HASH_SRCS
    for name in ("knn", "knn_host", "knn_max_k"):
        assert name in gicp.__all__


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_reference_agrees_with_ckdtree_where_nothing_ties(dim, k):
    pts = K.random_cloud(3000, dim, 31)
    qs = K.random_cloud(400, dim, 32, scale=11.0)
    assert not K.has_exact_tie(pts, qs, k)          # so scipy's traversal-dependent choice at ties is not involved
    idx, d2, cnt = K.knn(pts, qs, k)
    _, want = cKDTree(pts).query(qs, k=k)
    assert np.array_equal(idx, np.asarray(want).reshape(len(qs), k))
    assert np.all(cnt == k) and np.all(np.diff(d2, axis=1) > 0)


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_radius_agrees_with_ckdtree(dim):
    pts = K.random_cloud(3000, dim, 33)
    qs = K.random_cloud(400, dim, 34, scale=13.0)
    r = {2: 0.8, 3: 2.5}[dim]      # most queries find 8 rows, those beyond the cloud's rim none
    idx, d2, cnt = K.knn(pts, qs, 8, r)
    assert not K.has_exact_tie(pts, qs, 8)
    _, want = cKDTree(pts).query(qs, k=8, distance_upper_bound=r)
    want = np.where(want == len(pts), -1, want)
    assert np.array_equal(idx, want)
    assert np.array_equal(cnt, (want >= 0).sum(axis=1)) and 0 in cnt and 8 in cnt
    assert np.all(np.isinf(d2[idx < 0])) and np.all(d2[idx >= 0] <= r * r)


def _cases():
    return [(dim, name) for dim in (2, 3) for name in K.case_table(dim)]


@pytest.mark.parametrize("dim,name", _cases())
def test_host_yardstick_equals_the_reference(dim, name):
    _, pts, qs, k, r = K.case_table(dim)[name]
    want_i, want_d, want_c = K.expected(dim, name)
    idx, d2 = gicp.knn_host(pts, qs, k=k, max_distance=r)
    assert K.same_bits(idx, want_i), (name, np.argwhere(idx != want_i)[:5])
    assert K.same_bits(d2, want_d), name
    assert np.array_equal((idx >= 0).sum(axis=1), want_c)


def test_host_count_output_and_null_outputs():
    lib = _lib.load()
    pts, qs = K.lattice(3), K.lattice_queries(3)
    want_i, want_d, want_c = K.knn(pts, qs, 7, 1.0)
    cnt = np.full(len(qs), -7, dtype=np.int32)
    rc = lib.gicp_knn_host(_lib.dptr(pts), len(pts), _lib.dptr(qs), len(qs), 3, 7, 1.0, None, None,
                           cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0 and K.same_bits(cnt, want_c)
    idx = np.empty((len(qs), 7), dtype=np.int64)
    assert lib.gicp_knn_host(_lib.dptr(pts), len(pts), _lib.dptr(qs), len(qs), 3, 7, 1.0,
                             idx.ctypes.data_as(C.POINTER(C.c_int64)), None, None) == 0
    assert K.same_bits(idx, want_i)


def test_the_lattice_cases_do_tie():
    """The cases meant to rest on the index rule do: a cell centre has 2^dim rows at one distance."""
    for dim in (2, 3):
        assert K.has_exact_tie(K.lattice(dim), K.lattice_queries(dim), 2 ** dim)
        _, d2, _ = K.knn(K.coincident(dim), None, 32)
        assert np.all(d2[np.all(K.coincident(dim) == 0.375, axis=1)] == 0)


REFUSED = [
    (dict(k=0), "k must be 1..gicp_knn_max_k()"),
    (dict(k=33), "k must be 1..gicp_knn_max_k()"),
    (dict(max_distance=-1.0), "max_distance must be finite and >= 0"),
    (dict(max_distance=np.inf), "max_distance must be finite and >= 0"),
    (dict(max_distance=np.nan), "max_distance must be finite and >= 0"),
    (dict(points=np.zeros((4, 4)), queries=None), "cloud must be a non-empty N x 2 or N x 3 array"),
    (dict(points=np.zeros((0, 3))), "cloud must be a non-empty N x 2 or N x 3 array"),
    (dict(queries=np.zeros((0, 3))), "queries must be a non-empty Q x dim array"),
    (dict(points=np.array([[0.0, 1.0, np.nan], [0.0, 0.0, 0.0]])), "non-finite"),
    (dict(queries=np.array([[0.0, np.inf, 0.0]])), "non-finite"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
def test_host_refusals_carry_the_library_text(kw, text):
    args = dict(points=K.random_cloud(20, 3, 1), queries=K.random_cloud(5, 3, 2), k=2, max_distance=None)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        gicp.knn_host(args["points"], args["queries"], k=args["k"], max_distance=args["max_distance"])
    assert text in str(e.value) and str(e.value).startswith("gicp_knn_host: ")


def test_a_refused_host_call_writes_nothing():
    lib = _lib.load()
    pts, qs = K.random_cloud(20, 3, 1), K.random_cloud(5, 3, 2)
    qs[4, 1] = np.nan
    idx = np.full((5, 2), 77, dtype=np.int64)
    d2 = np.full((5, 2), 7.5)
    cnt = np.full(5, 77, dtype=np.int32)
    rc = lib.gicp_knn_host(_lib.dptr(pts), 20, _lib.dptr(qs), 5, 3, 2, 0.0, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                           _lib.dptr(d2), cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == _lib.GICP_E_INVALID and b"non-finite" in lib.gicp_last_host_error()
    assert np.all(idx == 77) and np.all(d2 == 7.5) and np.all(cnt == 77)
    assert lib.gicp_knn_host(_lib.dptr(pts), 20, _lib.dptr(pts), 5, 3, 2, 0.0, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                             _lib.dptr(d2), cnt.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert np.all(cnt == 2) and np.all(idx[:, 0] == np.arange(5))
