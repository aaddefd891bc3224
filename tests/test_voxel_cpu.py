"""Voxel-grid filter, the parts that need no GPU: the NumPy yardstick (tests/voxel_ref.py) against a plain
loop, and the new entry points' argument checks, which must not touch HIP."""
import ctypes as C

import numpy as np
import pytest

from voxel_ref import voxel_loop, voxel_ref

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("leaf,min_points", [(0.1, 1), (0.25, 1), (0.5, 2), (1.0, 5)])
def test_reference_equals_dict_loop(dim, leaf, min_points):
    """500 points, some exactly on cell faces and some negative: cells, order, counts and centroids (both
    sum a voxel's points in input order, so bit for bit) of voxel_ref equal the dict-of-lists loop's."""
    rng = np.random.default_rng(11)
    pts = rng.uniform(-2.0, 2.0, (500, dim))
    pts[:60] = rng.integers(-8, 8, (60, dim)) * 0.25
    c1, n1, k1 = voxel_ref(pts, leaf, min_points)
    c2, n2, k2 = voxel_loop(pts, leaf, min_points)
    assert len(c1) > 0
    assert np.array_equal(k1, k2) and np.array_equal(n1, n2)
    assert np.array_equal(c1, c2)
    assert n1.min() >= min_points
    if min_points == 1:
        assert n1.sum() == len(pts)


def test_null_context_is_invalid_without_hip():
    lib = _lib.load()
    pts = np.zeros((4, 3))
    out = np.zeros((4, 3))
    cnt = np.zeros(4, dtype=np.int32)
    m = C.c_int64(-7)
    rc = lib.gicp_voxel_downsample(None, _lib.dptr(pts), 4, 3, 0.1, 1, _lib.dptr(out),
                                   cnt.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m))
    assert rc == _lib.GICP_E_INVALID and m.value == -7
    assert lib.gicp_set_voxel(None, 0.1, 1) == _lib.GICP_E_INVALID
    n = C.c_int64(-7)
    assert lib.gicp_cloud_size(None, 0, C.byref(n)) == _lib.GICP_E_INVALID and n.value == -7
    assert lib.gicp_get_points(None, 0, _lib.dptr(out)) == _lib.GICP_E_INVALID


def test_new_entry_points_are_bound_and_hashed():
    for name in ("gicp_voxel_downsample", "gicp_set_voxel", "gicp_cloud_size", "gicp_get_points"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "csrc/gicp_voxel.hip" in _lib.HASH_SRCS
    assert callable(gicp.voxel_downsample)
    for m in ("set_voxel", "cloud_size", "points", "voxel_downsample"):
        assert hasattr(gicp.Engine, m)
