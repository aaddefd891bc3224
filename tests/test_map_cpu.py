"""The local voxel map without a GPU: the NumPy restatement (tests/map_ref.py) against the voxel filter's
(tests/voxel_ref.py) and against a plain loop, and Odometry's scan-to-map mode on the NumPy fake of the device
entry points (tests/fake_device.py) with the six gicp_map_* calls added on top of map_ref."""
import ctypes as C

import numpy as np
import pytest

from map_ref import MapLoop, MapRef, transform
from voxel_ref import voxel_ref

gicp = pytest.importorskip("gicp")
from fake_device import E_INVALID, E_STATE, OK, FakeLib, _arr  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from oracle import gicp_oracle as O  # noqa: E402

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)


def _pose3(axis, angle, t):
    T = np.eye(4)
    T[:3, :3] = O.so3_exp(np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis) * angle)
    T[:3, 3] = t
    return T


def _pose2(yaw, t):
    T = np.eye(3)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 2] = t
    return T


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("leaf", [0.1, 0.25])
def test_identity_pose_and_huge_window_is_the_voxel_filter(dim, leaf):
    rng = np.random.default_rng(1)
    pts = rng.uniform(-4.0, 4.0, (3000, dim))
    cells, cent, cnt, _ = MapRef(dim, leaf, 1e4).insert(pts, np.eye(dim + 1)).get()
    r_cent, r_cnt, r_cells = voxel_ref(pts, leaf)
    assert np.array_equal(cells, r_cells) and np.array_equal(cnt, r_cnt) and np.array_equal(cent, r_cent)
    for mp in (2, 3):
        k_cells, k_cent, k_cnt, _ = MapRef(dim, leaf, 1e4).insert(pts, np.eye(dim + 1)).get(mp)
        f_cent, f_cnt, f_cells = voxel_ref(pts, leaf, mp)
        assert np.array_equal(k_cells, f_cells) and np.array_equal(k_cnt, f_cnt) and np.array_equal(k_cent, f_cent)


def test_transform_is_the_stated_expression():
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(50, 3))
    T = _pose3([1, 2, 3], 0.7, [0.3, -5.0, 2.0])
    w = transform(pts, T)
    R, t = T[:3, :3], T[:3, 3]
    for a in range(3):
        assert np.array_equal(w[:, a], R[a, 0] * pts[:, 0] + R[a, 1] * pts[:, 1] + R[a, 2] * pts[:, 2] + t[a])
    np.testing.assert_allclose(w, O.apply_transformation(pts, T), atol=1e-12)


@pytest.mark.parametrize("dim", [3, 2])
def test_loop_agrees_with_vectorised(dim):
    rng = np.random.default_rng(3)
    poses = ([_pose3([1, 2, 3], 0.3, [0.2, 0.1, 0.0]), _pose3([3, -1, 2], -0.5, [1.4, -0.3, 0.2]),
              _pose3([0, 1, 1], 1.1, [-0.9, 0.8, 0.1])] if dim == 3 else
             [_pose2(0.3, [0.2, 0.1]), _pose2(-0.5, [1.4, -0.3]), _pose2(1.1, [-0.9, 0.8])])
    a, b = MapRef(dim, 0.25, 1.5), MapLoop(dim, 0.25, 1.5)
    for T in poses:
        pts = rng.uniform(-2.5, 2.5, (400, dim))
        a.insert(pts, T)
        b.insert(pts, T)
        ca, xa, na, _ = a.get()
        cb, xb, nb = b.get()
        assert len(ca) > 20
        assert np.array_equal(ca, cb) and np.array_equal(na, nb) and np.array_equal(xa, xb)
    assert np.array_equal(a.get(2)[0], b.get(2)[0])


def test_reentering_a_forgotten_region_starts_from_zero():
    rng = np.random.default_rng(4)
    A = rng.uniform(-1.0, 1.0, (500, 3))
    far = np.eye(4)
    far[0, 3] = 10.0
    m = MapRef(3, 0.25, 1.0)
    once = MapRef(3, 0.25, 1.0).insert(A, np.eye(4)).get()
    m.insert(A, np.eye(4))
    m.insert(A, far)                      # A's points land around x = 10: the voxels around 0 are forgotten
    assert np.all(m.get()[0][:, 0] >= 36)
    m.insert(A, np.eye(4))                # back: the voxels around x = 10 go, those around 0 start again
    cells, cent, cnt, _ = m.get()
    assert np.array_equal(cells, once[0]) and np.array_equal(cnt, once[2]) and np.array_equal(cent, once[1])
    twice = MapRef(3, 0.25, 1.0).insert(A, np.eye(4)).insert(A, np.eye(4)).get()
    assert np.array_equal(twice[2], 2 * once[2])


def test_window_is_a_cube_of_cells_around_the_pose_cell():
    pts = np.array([[0.05, 0.05], [0.30, 0.05], [-0.20, 0.05], [0.55, 0.05], [0.05, -0.30]])
    m = MapRef(2, 0.25, 0.25).insert(pts, np.eye(3))          # R = 1: cells -1 .. 1
    assert np.array_equal(m.get()[0], [[-1, 0], [0, 0], [1, 0]])
    m0 = MapRef(2, 4.0, 5e-324)                                # max_range / leaf rounds to 0: R = 0,
    assert m0.R == 0                                           # the pose's own cell only
    assert np.array_equal(m0.insert(pts * 16.0, np.eye(3)).get()[0], [[0, 0]])
    assert m0.get()[2][0] == 1


# ---- Odometry's scan-to-map mode on the fake device ------------------------------------------------------

class FakeMapLib(FakeLib):
    """tests/fake_device.FakeLib plus the gicp_map_* entry points on map_ref, and what Engine.map_to_target and
    Odometry need besides (gicp_cloud_size).  Records the start pose of every gicp_align."""

    def __init__(self, real, ndev=2):
        super().__init__(real, ndev)
        self.starts = []

    def gicp_cloud_size(self, ctx, which, out):
        c = self._c(ctx)
        cl = c.tgt if which == 0 else c.src
        out._obj.value = 0 if cl is None else len(cl["pts"])
        return OK

    def gicp_align(self, ctx, T0, p, T_out, res):
        d = self._c(ctx).src["pts"].shape[1]
        self.starts.append(_arr(T0, (d + 1, d + 1)).copy())
        return super().gicp_align(ctx, T0, p, T_out, res)

    def gicp_map_reset(self, ctx, dim, leaf, max_range):
        c = self._c(ctx)
        if dim not in (2, 3) or not (np.isfinite(leaf) and leaf > 0 and np.isfinite(max_range) and max_range > 0):
            return self._fail(c, E_INVALID, "bad map parameters")
        c.map = MapRef(dim, leaf, max_range)
        return OK

    def _map(self, c):
        return getattr(c, "map", None)

    def gicp_map_insert(self, ctx, which, T):
        c = self._c(ctx)
        m = self._map(c)
        cl = c.tgt if which == 0 else c.src
        if m is None or cl is None:
            return self._fail(c, E_STATE, "no map: call gicp_map_reset first" if m is None else "cloud not set")
        m.insert(cl["pts"], _arr(T, (m.dim + 1, m.dim + 1)).copy())
        return OK

    def gicp_map_insert_points(self, ctx, ptr, n, dim, T):
        c = self._c(ctx)
        m = self._map(c)
        if m is None:
            return self._fail(c, E_STATE, "no map: call gicp_map_reset first")
        m.insert(_arr(ptr, (int(n), int(dim))).copy(), _arr(T, (dim + 1, dim + 1)).copy())
        return OK

    def gicp_map_size(self, ctx, out):
        m = self._map(self._c(ctx))
        out._obj.value = 0 if m is None else len(m)
        return OK

    def gicp_map_get(self, ctx, cells, cent, cnt):
        c = self._c(ctx)
        m = self._map(c)
        if m is None:
            return self._fail(c, E_STATE, "no map: call gicp_map_reset first")
        k, x, n, _ = m.get()
        if len(k):
            _arr(cells, k.shape, np.int32)[:] = k
            _arr(cent, x.shape)[:] = x
            _arr(cnt, n.shape, np.int32)[:] = n
        return OK

    def gicp_map_to_target(self, ctx, p, min_points):
        c = self._c(ctx)
        m = self._map(c)
        if m is None:
            return self._fail(c, E_STATE, "no map: call gicp_map_reset first")
        x = m.get(min_points)[1]
        if not len(x):
            return self._fail(c, E_INVALID, "the map is empty")
        par = p._obj if hasattr(p, "_obj") else p
        cov, cnt = O.covariances(x, par.max_distance_nearest_neighbors, par.k_neighbors or None)
        c.tgt = dict(pts=x.copy(), cov=cov, cnt=cnt, p=par)
        return OK


@pytest.fixture
def fake(monkeypatch):
    from gicp import _lib
    lib = FakeMapLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", lib)
    monkeypatch.setattr(gicp, "_ENGINES", {})
    return lib


@pytest.fixture(scope="module")
def stream():
    return list(S.lidar_stream(4, beams=8, azimuths=240, step=0.15, along_path=True))


def _odo(init, **kw):
    from gicp.odometry import Odometry
    return Odometry(3, params=gicp.default_params(3, max_iterations=6, tolerance=1e-9, **P3), init=init,
                    map_voxel_size=0.25, map_range=30.0, **kw)


def test_map_mode_bookkeeping_on_the_fake_device(fake, stream):
    odo = _odo("identity")
    P0 = _pose3([0, 0, 1], 0.2, [1.0, -2.0, 0.5])
    odo.pose = P0
    out = [odo.step(scan) for scan, _ in stream]
    assert out[0] == (None, None) and len(odo.poses) == len(stream) == odo.frames
    assert np.array_equal(odo.poses[0], P0)
    for k in range(1, len(stream)):
        T, res = out[k]
        assert res["iterations"] >= 1
        np.testing.assert_allclose(T, np.linalg.inv(odo.poses[k]) @ odo.poses[k - 1], atol=1e-12)
        assert np.array_equal(fake.starts[k - 1], odo.poses[k - 1])     # init='identity': start at the last pose
    assert np.array_equal(odo.pose, odo.poses[-1])
    assert odo.eng.map_size() > 100 and odo.eng.n_tgt == odo.eng.map_size()
    cells, cent, cnt = odo.eng.map_get()
    assert cells.dtype == np.int32 and cnt.dtype == np.int32 and cent.shape == cells.shape
    assert int(cnt.sum()) <= sum(len(s) for s, _ in stream) and np.array_equal(np.floor(cent / 0.25), cells)
    assert odo.timing["map_s"] > 0 and odo.timing["iterations"] > 0
    odo.reset()
    assert odo.eng.map_size() == 0 and odo.frames == 0 and len(odo.poses) == 1
    assert odo.step(stream[0][0]) == (None, None) and odo.eng.map_size() > 0


def test_map_mode_constant_velocity_prediction_and_run(fake, stream):
    odo = _odo("constant_velocity")
    out = list(odo.run([s for s, _ in stream]))       # coming scans are accepted and ignored
    assert len(out) == len(stream) and out[0] == (None, None)
    P = odo.poses
    assert np.array_equal(fake.starts[0], P[0])       # second frame: no velocity yet
    for k in (2, 3):
        want = P[k - 1] @ (np.linalg.inv(P[k - 2]) @ P[k - 1])
        np.testing.assert_allclose(fake.starts[k - 1], want, atol=1e-12)


def test_map_mode_argument_errors(fake):
    from gicp.odometry import Odometry
    with pytest.raises(ValueError, match="map_range"):
        Odometry(3, map_voxel_size=0.25)
    with pytest.raises(ValueError, match="reference"):
        Odometry(3, map_voxel_size=0.25, map_range=10.0, composition="reference")
    with pytest.raises(ValueError, match="map_min_points"):
        Odometry(3, map_voxel_size=0.25, map_range=10.0, map_min_points=0)
    with pytest.raises(ValueError):
        Odometry(3, map_voxel_size=-1.0, map_range=10.0)       # from the library
    eng = gicp.Engine(0)
    with pytest.raises(gicp._lib.GicpError) as ei:
        eng.map_insert(np.eye(4), points=np.zeros((3, 3)))
    assert ei.value.code == gicp._lib.GICP_E_STATE


def test_scan_to_scan_mode_is_untouched(fake, stream):
    """map_voxel_size=None never calls a map entry point: today's mode."""
    from gicp.odometry import Odometry
    odo = Odometry(3, params=gicp.default_params(3, max_iterations=3, **P3), init="identity")
    for scan, _ in stream[:3]:
        odo.step(scan)
    assert odo.eng.map_size() == 0 and "map_s" not in odo.timing and len(odo.poses) == 3


def test_map_signatures_cover_the_six_calls():
    from gicp import _lib
    names = {"gicp_map_reset", "gicp_map_insert", "gicp_map_insert_points", "gicp_map_size", "gicp_map_get",
             "gicp_map_to_target"}
    assert names <= set(_lib.SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n
    assert _lib.SIGNATURES["gicp_map_get"][1][1] == C.POINTER(C.c_int32)
