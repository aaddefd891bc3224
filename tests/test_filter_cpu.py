"""Input filters, the parts that need no GPU: the host yardstick gicp_filter_points_host against the
NumPy reference (tests/filter_ref.py) bit for bit, the refusals with their messages, the new entry points' argument
checks, which must not touch HIP, and the preconditions the GPU tests of test_gpu_filter.py lean on, measured here."""
import ctypes as C
import inspect

import numpy as np
import pytest

import density_ref as D
import filter_ref as F

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", sorted(F.cases(3)))
def test_host_filter_matches_reference(dim, name):
    keep, counts = F.check_against_reference(gicp.filter_points_host, dim, name)
    if name == "widest":      # the 70 coincident rows, and each corner with the cells beside it, a distance of exactly 1
        assert keep.sum() == 70 + 2 * (1 + dim) and counts.max() == 69
    if name.startswith("lattice_3"):
        pts, kw, _, _ = F.reference(dim, name)
        r = np.sqrt(F.d2(pts, np.zeros((1, dim))))
        assert np.any(r == 1.25) and np.any(r == 2.5)          # rows exactly on both bounds, kept
        assert np.all(keep[(r == 1.25) | (r == 2.5)] | (kw.get("radius", 0) > 0))
    if name == "dense_cell":
        assert counts.max() >= 4999


def test_cases_decide_something():
    """Every case keeps some rows and, but for the smallest, removes some: a filter that kept or dropped everything
    would pass no information."""
    for dim in (2, 3):
        for name in F.cases(dim):
            _, _, keep, _ = F.reference(dim, name)
            assert keep.any(), (dim, name)
            if name not in ("one_row", "two_coincident"):
                assert not keep.all(), (dim, name)


def test_rounded_difference_two_cells_apart():
    """radius 1, x_i = 1 - 2^-53, x_j = 2: the exact difference exceeds the radius, the rounded one is 1.0, so
    d2 <= r^2 holds -- and floor(x / radius) puts the two 2 cells apart.  The grid's edge radius (1 + 2^-16) keeps
    them in adjacent cells (gicp_filter.h kRorEdge)."""
    for dim in (2, 3):
        pts = np.zeros((3, dim))
        pts[0, 0], pts[1, 0], pts[2, 0] = 1.0 - 2.0 ** -53, 2.0, 50.0
        assert pts[1, 0] - pts[0, 0] == 1.0 and np.floor(pts[1, 0]) - np.floor(pts[0, 0]) == 2
        keep, counts = F.filter_ref(pts, radius=1.0, min_neighbors=1)
        assert list(counts) == [1, 1, 0]
        rows, idx, cnt = gicp.filter_points_host(pts, radius=1.0, min_neighbors=1, return_index=True, return_counts=True)
        assert list(idx) == [0, 1] and list(cnt) == [1, 1, 0]


def test_identity_and_order():
    pts = np.random.default_rng(2).normal(size=(100, 3))
    rows, idx, cnt = gicp.filter_points_host(pts, return_index=True, return_counts=True)
    assert rows.tobytes() == pts.tobytes() and np.array_equal(idx, np.arange(100)) and np.all(cnt == 0)
    rows, idx = gicp.filter_points_host(pts, max_range=1.5, return_index=True)
    assert np.all(np.diff(idx) > 0) and rows.tobytes() == pts[idx].tobytes()


def _host(pts, f, out=None):
    """(rc, message) of one raw gicp_filter_points_host call."""
    lib = _lib.load()
    a = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.full_like(a, -7.0) if out is None else out
    m = C.c_int64(-5)
    rc = lib.gicp_filter_points_host(_lib.dptr(a), a.shape[0], a.shape[1], C.byref(f) if f is not None else None,
                                     _lib.dptr(out), None, None, C.byref(m))
    return rc, lib.gicp_last_host_error().decode(), out, m.value


def _filter(**kw):
    f = _lib.Filter()
    for k, v in kw.items():
        if k == "center":
            for i, c in enumerate(v):
                f.center[i] = c
        else:
            setattr(f, k, v)
    return f


REFUSED = [
    (dict(min_range=np.nan), "must be finite"),
    (dict(max_range=np.inf), "must be finite"),
    (dict(radius=np.nan, min_neighbors=1), "must be finite"),
    (dict(center=(0.0, np.inf, 0.0), max_range=1.0), "center is not finite"),
    (dict(min_range=-1.0), "must be >= 0"),
    (dict(max_range=-0.5), "must be >= 0"),
    (dict(radius=-2.0, min_neighbors=1), "must be >= 0"),
    (dict(min_range=3.0, max_range=2.0), "min_range 3 exceeds max_range 2"),
    (dict(radius=1.0, min_neighbors=0), "min_neighbors must be >= 1"),
]


def test_refusals_and_their_messages():
    pts = np.random.default_rng(4).uniform(-2.0, 2.0, (50, 3))
    for kw, text in REFUSED:
        rc, msg, out, m = _host(pts, _filter(**kw))
        assert rc == _lib.GICP_E_INVALID and text in msg and msg.startswith("gicp_filter_points_host: "), (kw, msg)
        assert np.all(out == -7.0)
        with pytest.raises(ValueError, match=text.replace("(", r"\(")):
            gicp.filter_points_host(pts, **kw)
    # min_range > max_range is no error without an upper limit
    assert _host(pts, _filter(min_range=1.0))[0] == _lib.GICP_OK
    rc, msg, _, _ = _host(pts, None)
    assert rc == _lib.GICP_E_INVALID and "filter must not be NULL" in msg
    bad = np.array(pts)
    bad[7, 2] = np.nan
    rc, msg, out, _ = _host(bad, _filter(max_range=1.0))
    assert rc == _lib.GICP_E_INVALID and "non-finite coordinates" in msg and np.all(out == -7.0)
    # a stage that leaves no row names itself
    rc, msg, _, m = _host(pts, _filter(min_range=100.0))
    assert rc == _lib.GICP_E_INVALID and "the range crop removed all 50 points" in msg and m == 0
    rc, msg, _, m = _host(pts, _filter(max_range=2.0, radius=0.01, min_neighbors=1))
    n_crop = int(np.sum(F.filter_ref(pts, max_range=2.0)[0]))
    assert 0 < n_crop < 50 and F.filter_ref(pts, radius=0.01)[1].max() == 0
    assert rc == _lib.GICP_E_INVALID and f"radius outlier removal removed all {n_crop} points the crop left" in msg and m == 0
    lib = _lib.load()
    out = np.empty_like(pts)
    f = _filter(max_range=1.0)
    m = C.c_int64()
    assert lib.gicp_filter_points_host(None, 50, 3, C.byref(f), _lib.dptr(out), None, None, C.byref(m)) == _lib.GICP_E_INVALID
    assert lib.gicp_filter_points_host(_lib.dptr(pts), 50, 3, C.byref(f), None, None, None, C.byref(m)) == _lib.GICP_E_INVALID
    assert lib.gicp_filter_points_host(_lib.dptr(pts), 50, 3, C.byref(f), _lib.dptr(out), None, None, None) == _lib.GICP_E_INVALID
    assert lib.gicp_filter_points_host(_lib.dptr(pts), 0, 3, C.byref(f), _lib.dptr(out), None, None, C.byref(m)) == _lib.GICP_E_INVALID
    assert lib.gicp_filter_points_host(_lib.dptr(pts), 50, 4, C.byref(f), _lib.dptr(out), None, None, C.byref(m)) == _lib.GICP_E_INVALID
    with pytest.raises(ValueError, match="center must hold 3 values"):
        gicp.filter_points_host(pts, center=(0.0, 0.0), max_range=1.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_widest_span_is_taken_and_the_next_refused(dim):
    """2^21 (3-D) / 2^31 (2-D) cells of edge radius pass (test_host_filter_matches_reference runs that cloud); one
    cell more is refused, and the message names the axis and the way out."""
    pts = F.widest(dim, extra=1)
    rc, msg, _, _ = _host(pts, _filter(radius=1.0, min_neighbors=1))
    span = 2 ** 21 if dim == 3 else 2 ** 31
    assert rc == _lib.GICP_E_INVALID, msg
    assert f"axis x spans {float(span + 1):.6g} cells of edge radius = 1" in msg and "max_range" in msg
    assert f"2^{21 if dim == 3 else 31}" in msg
    # the same cloud with that one point cropped away passes: the limit is on the CROPPED cloud
    far = pts[np.argmax(pts[:, 0])]
    keep, _ = F.filter_ref(pts, center=far, min_range=0.5, radius=1.0, min_neighbors=1)
    assert keep.sum() == 70 + 2 * (1 + dim) and not keep[np.argmax(pts[:, 0])]
    rows = gicp.filter_points_host(pts, center=far, min_range=0.5, radius=1.0, min_neighbors=1)
    assert rows.tobytes() == pts[keep].tobytes()


def test_null_context_is_invalid_without_hip():
    lib = _lib.load()
    pts = np.zeros((4, 3))
    out = np.full((4, 3), -7.0)
    f = _filter(max_range=1.0)
    m = C.c_int64()
    assert lib.gicp_filter_points(None, _lib.dptr(pts), 4, 3, C.byref(f), _lib.dptr(out), None, None, C.byref(m)) == _lib.GICP_E_INVALID
    assert lib.gicp_set_filter(None, C.byref(f)) == _lib.GICP_E_INVALID
    assert np.all(out == -7.0)


def test_new_entry_points_are_bound_and_hashed():
    for name in ("gicp_filter_points", "gicp_filter_points_host", "gicp_set_filter", "gicp_last_host_error"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().gicp_version() >= 104
    i = _lib.HASH_SRCS.index("csrc/gicp_filter.hip")
    assert _lib.HASH_SRCS[i - 1] == "csrc/gicp_eval.hip"
    j = _lib.HASH_SRCS.index("csrc/gicp_filter.h")
    assert _lib.HASH_SRCS[j - 1] == "csrc/gicp_sweep.h"
    assert _lib.build_info()["src"] == _lib.source_hash()
    assert C.sizeof(_lib.Filter) == 6 * 8 + 2 * 4
    assert callable(gicp.filter_points) and callable(gicp.filter_points_host)
    for m in ("set_filter", "filter_points"):
        assert {"center", "min_range", "max_range", "radius", "min_neighbors"} <= set(
            inspect.signature(getattr(gicp.Engine, m)).parameters)
    sig = inspect.signature(gicp.gicp).parameters
    for k in ("min_range", "max_range", "outlier_radius", "filter_center"):
        assert sig[k].default is None
    assert sig["outlier_min_neighbors"].default == 1
    from gicp.odometry import Odometry
    sig = inspect.signature(Odometry.__init__).parameters
    assert sig["min_range"].default is None and sig["max_range"].default is None
    assert sig["outlier_radius"].default is None and sig["outlier_min_neighbors"].default == 1


# ---- the preconditions of the fused GPU tests, asserted exactly ----

ROR = {"stretched_3d": (2.0, 3, 3), "halo_3d": (2.0, 3, 3), "stretched_2d": (20.0, 2, 2)}   # radius, core's least count, min_neighbors


@pytest.mark.parametrize("name", sorted(ROR))
def test_radius_filter_keeps_exactly_the_core(name):
    """Every far or halo point has 0 neighbours within the radius, every core point at least 3 (2-D: 2), in source
    and target, so radius outlier removal with that min_neighbors keeps exactly core_only(name).  No decision
    hangs on an ulp: the nearest d2 to r^2, over all pairs, is >= 1e-7 r^2 away, nine orders above rounding."""
    f = D.fixture(name)
    radius, least, min_nb = ROR[name]
    core = dict(source=D.core_only(name)[0], target=D.core_only(name)[1])
    for which in ("source", "target"):
        pts, is_core = f[which], f["core_" + which]
        keep, counts = F.filter_ref(pts, radius=radius, min_neighbors=min_nb)
        assert np.all(counts[~is_core] == 0), (which, counts[~is_core])
        assert counts[is_core].min() >= least, (which, int(counts[is_core].min()))
        assert np.array_equal(keep, is_core)
        assert F.min_margin(pts, radius) >= 1e-7
        rows, cnt = gicp.filter_points_host(pts, radius=radius, min_neighbors=min_nb, return_counts=True)
        assert rows.tobytes() == core[which].tobytes() and np.array_equal(cnt, counts)


def test_crop_keeps_exactly_the_core_of_offset_origin():
    """The 12 invalid returns about the origin have neighbours among themselves (up to 11), so radius outlier
    removal does not remove them; the crop center = 0, min_range = 10 does, and keeps exactly the core."""
    f = D.fixture("offset_origin_3d")
    core = dict(source=D.core_only("offset_origin_3d")[0], target=D.core_only("offset_origin_3d")[1])
    for which in ("source", "target"):
        pts, is_core = f[which], f["core_" + which]
        _, counts = F.filter_ref(pts, radius=2.0, min_neighbors=3)
        assert counts[~is_core].max() >= 3 and counts[~is_core].max() <= D.N_FAR - 1
        keep, _ = F.filter_ref(pts, min_range=10.0)
        assert np.array_equal(keep, is_core)
        r2 = F.d2(pts, np.zeros((1, 3)))
        assert np.min(np.abs(r2 - 100.0)) / 100.0 >= 1e-7
        rows = gicp.filter_points_host(pts, min_range=10.0)
        assert rows.tobytes() == core[which].tobytes()
