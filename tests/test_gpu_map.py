"""The local voxel map on the device (gicp_map_*) against the NumPy restatement
(tests/map_ref.py), the voxel filter and the cloud builds it must equal bit for bit, and scan-to-map odometry
against the oracle frame by frame."""
import numpy as np
import pytest

from map_ref import MapRef
from test_gpu_voxel import _points
from voxel_ref import voxel_ref

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from oracle import gicp_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
P2 = dict(max_distance_correspondence=20.0, max_distance_nearest_neighbors=25.0)


def _pose(dim, k, t):
    """Non-trivial poses: 3-D rotations about skew axes, 2-D yaws."""
    T = np.eye(dim + 1)
    if dim == 3:
        axis = np.array([[1.0, 2.0, 3.0], [3.0, -1.0, 2.0], [-2.0, 1.0, 1.5]][k % 3])
        T[:3, :3] = O.so3_exp(axis / np.linalg.norm(axis) * [0.31, -0.77, 1.9][k % 3])
    else:
        a = [0.31, -0.77, 1.9][k % 3]
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:dim, dim] = np.asarray(t, dtype=np.float64)[:dim]
    return T


@pytest.fixture
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_against_ref(got, ref, min_points=1):
    """Cells and counts exactly map_ref's; centroids within count 2^-51 max|x_a| per coordinate (the bound
    tests/test_gpu_voxel.py::_check_centroids derives), max|x_a| over every world-frame point merged into the
    voxel.  Returns the worst error / bound."""
    cells, cent, cnt = got
    r_cells, r_cent, r_cnt, amax = ref.get(min_points)
    assert cells.dtype == np.int32 and cnt.dtype == np.int32
    assert cells.shape == r_cells.shape and np.array_equal(cells, r_cells)
    assert np.array_equal(cnt, r_cnt)
    bound = r_cnt[:, None] * 2.0 ** -51 * amax
    err = np.abs(cent - r_cent)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0
    print("max centroid error / bound:", worst, "rows", len(cells))
    assert np.all(err <= bound)
    return worst


# 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("name", ["n1", "n63", "n64", "n65", "n129", "n20000", "lattice"])
def test_single_insert_equals_the_filter_bit_for_bit(eng, name, dim):
    pts, leaf = _points(name, dim)
    f_xyz, f_cnt = gicp.voxel_downsample(pts, leaf, return_counts=True)
    eng.map_reset(leaf, 100.0, dim)
    eng.map_insert(np.eye(dim + 1), points=pts)
    cells, cent, cnt = eng.map_get()
    assert eng.map_size() == len(f_xyz)
    assert np.array_equal(cent, f_xyz) and np.array_equal(cnt, f_cnt)
    assert np.array_equal(cells, voxel_ref(pts, leaf)[2])


# 2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("leaf", [0.1, 0.25])
def test_merging_posed_scans(eng, leaf, dim):
    rng = np.random.default_rng(11)
    ref = MapRef(dim, leaf, 12.0)
    eng.map_reset(leaf, 12.0, dim)
    for k, t in enumerate([[0.3, -0.2, 0.1], [0.9, 0.4, -0.3], [-0.5, 0.7, 0.2]]):
        pts = rng.uniform(-2.0, 2.0, (5000, dim))
        T = _pose(dim, k, t)
        eng.map_insert(T, points=pts)
        ref.insert(pts, T)
        _check_against_ref(eng.map_get(), ref)
    assert eng.map_get()[2].sum() == 15000 and eng.map_get()[2].max() > 1


# 3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_a_voxel_spanning_waves_across_inserts(eng, dim):
    rng = np.random.default_rng(12)
    one = rng.uniform(3.0, 3.25, (5000, dim))
    ref = MapRef(dim, 0.25, 50.0)
    eng.map_reset(0.25, 50.0, dim)
    for _ in range(2):
        eng.map_insert(np.eye(dim + 1), points=one)
        ref.insert(one, np.eye(dim + 1))
    cells, cent, cnt = eng.map_get()
    assert len(cells) == 1 and cnt[0] == 10000
    _check_against_ref((cells, cent, cnt), ref)
    dense, dleaf = _points("dense_between", dim)
    ref = MapRef(dim, dleaf, 50.0)
    eng.map_reset(dleaf, 50.0, dim)
    for _ in range(2):
        eng.map_insert(np.eye(dim + 1), points=dense)
        ref.insert(dense, np.eye(dim + 1))
    got = eng.map_get()
    assert got[2].max() >= 10000
    _check_against_ref(got, ref)


# 4 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("leaf,max_range", [(0.25, 1.0), (0.25, 0.6), (4.0, 5e-324)])
def test_window_forgets_and_starts_again(eng, leaf, max_range, dim):
    """A at the origin, B at a centre three quarters of a window away (part of A's voxels and part of B's points fall outside
    the cube), then A at the origin again.  (0.25, 0.6): R = 3, the window's faces cut through occupied cells.
    (4.0, 5e-324): max_range / leaf rounds to 0, so R = 0 -- the pose's own cell alone."""
    rng = np.random.default_rng(13)
    ref = MapRef(dim, leaf, max_range)
    R = ref.R
    assert R == {1.0: 4, 0.6: 3, 5e-324: 0}[max_range]
    w = (2 * R + 1) * leaf
    A = rng.uniform(-0.7 * w, 0.7 * w, (4000, dim))        # wider than the window
    B = rng.uniform(-0.7 * w, 0.7 * w, (4000, dim))
    c0 = _pose(dim, 0, [0.01, 0.02, 0.03])
    c0[:dim, :dim] = np.eye(dim)
    c1 = _pose(dim, 1, [0.75 * w, -0.2 * w, 0.1 * w])       # the windows overlap in part
    eng.map_reset(leaf, max_range, dim)
    eng.map_insert(c0, points=A)
    ref.insert(A, c0)
    first = eng.map_get()
    _check_against_ref(first, ref)
    assert np.abs(first[0]).max() == R and 0 < first[2].sum() < len(A)        # up to the cube's faces, points cut off
    eng.map_insert(c1, points=B)
    ref.insert(B, c1)
    second = eng.map_get()
    _check_against_ref(second, ref)
    kept = (first[0][:, None, :] == second[0][None, :, :]).all(-1).any(1)     # A's voxels that survived
    assert (R == 0 and not kept.any()) or (0 < kept.sum() < len(kept))
    eng.map_insert(c0, points=A)
    ref.insert(A, c0)
    third = eng.map_get()
    _check_against_ref(third, ref)
    hit = (first[0][:, None, :] == third[0][None, :, :]).all(-1)
    assert hit.any(1).all()                                  # every voxel of the first insert is back
    again = third[2][hit.argmax(1)]
    assert np.array_equal(again[~kept], first[2][~kept])     # dropped by the second insert: A's counts, not doubled
    assert np.all(again[kept] >= 2 * first[2][kept])


# 4b --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_widest_accepted_window(eng, dim):
    """Leaf 1.0 and max_range 2^20 - 1 (3-D) or 2^30 - 1 (2-D): 2 R + 1 = 2^21 - 1 or 2^31 - 1 cells per axis,
    the widest accepted window (63 and 62 key bits); one more is refused.  An insert centred on a negative cell
    with points (at cell + 0.5, exact in fp64) in the window's lowest and highest corner cells, in the cells
    next to them, one cell outside on either side of every axis, 70 in one cell and 2000 scattered; a second
    insert re-centres by one cell on every axis, so the lowest corner voxel is forgotten and the cell beyond the
    highest corner is now inside.  Cells and counts exactly map_ref's, centroids within its bound."""
    R = 2 ** 20 - 1 if dim == 3 else 2 ** 30 - 1
    with pytest.raises(ValueError, match="window too wide"):
        eng.map_reset(1.0, float(R + 1), dim)
    eng.map_reset(1.0, float(R), dim)
    ref = MapRef(dim, 1.0, float(R))
    assert ref.R == R
    rng = np.random.default_rng(18)
    t = np.array([-5000.25, -77.5, -123456.75][:dim])
    c = np.floor(t).astype(np.int64)
    assert np.all(c < 0)
    step = np.eye(dim, dtype=np.int64)

    def scan(centre, seed_cells, n):
        lo, hi = centre - R, centre + R
        cells = [rng.integers(-R, R + 1, (n, dim)) + centre, lo[None], hi[None], lo + step, hi - step,
                 lo - step, hi + step, np.tile(c + R // 3, (70, 1)), seed_cells]
        cells = np.concatenate(cells)
        return cells[rng.permutation(len(cells))]

    def insert(cells, trans):
        T = np.eye(dim + 1)
        T[:dim, dim] = trans
        pts = (cells.astype(np.float64) + 0.5) - trans          # the sensor-frame points: exact, and exact back
        assert np.array_equal(pts + trans, cells + 0.5)
        eng.map_insert(T, points=pts)
        ref.insert(pts, T)
        got = eng.map_get()
        _check_against_ref(got, ref)
        return got

    first_cells = scan(c, np.zeros((0, dim), dtype=np.int64), 2000)
    first = insert(first_cells, t)
    assert np.array_equal(first[0][0], c - R) and np.array_equal(first[0][-1], c + R)
    assert len(first[0]) == len(np.unique(first_cells, axis=0)) - 2 * dim and first[2].max() == 70
    assert np.array_equal(first[1], first[0] + 0.5)
    # the second insert: centred one cell further on every axis; 500 of the first scan's cells are hit again
    second_cells = scan(c + 1, first_cells[:500], 1500)
    second = insert(second_cells, t + 1.0)
    seen = {tuple(r) for r in second[0].tolist()}
    assert tuple(c - R) not in seen and tuple(c + R + 1) in seen          # forgotten; the new highest corner
    assert np.array_equal(second[0][-1], c + 1 + R) and second[2].max() >= 140 and np.sum(second[2] == 2) >= 400
    assert eng.map_size() == len(second[0]) == len(ref)


# 5 ---------------------------------------------------------------------------------------------------------
def _sequence(e, dim):
    rng = np.random.default_rng(14)
    e.map_reset(0.25, 3.0, dim)
    for k, t in enumerate([[0.0, 0.0, 0.0], [1.5, 0.5, 0.2], [3.5, -0.5, 0.1]]):
        e.map_insert(_pose(dim, k, t), points=rng.uniform(-3.0, 3.0, (5000, dim)))
    return e.map_get()


@pytest.mark.parametrize("dim", [3, 2])
def test_determinism_across_resets_and_engines(eng, dim):
    a = _sequence(eng, dim)
    b = _sequence(eng, dim)
    other = gicp.Engine(0)
    try:
        c = _sequence(other, dim)
    finally:
        other.close()
    assert len(a[0]) > 100 and _same(a, b) and _same(a, c)


# 6 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("voxel", [None, 0.1])
def test_device_insert_equals_host_insert(eng, voxel, dim):
    rng = np.random.default_rng(15)
    pts = rng.uniform(-3.0, 3.0, (6000, dim))
    p = gicp.default_params(dim, **P3)
    T = _pose(dim, 2, [0.4, -0.6, 0.2])
    if voxel:
        eng.set_voxel(voxel)
    eng.set_source(pts, p)
    host = eng.points("source") if voxel else pts
    assert (len(host) < len(pts)) == bool(voxel)
    eng.map_reset(0.25, 4.0, dim)
    eng.map_insert(T, which="source")
    dev = eng.map_get()
    eng.map_reset(0.25, 4.0, dim)
    eng.map_insert(T, points=host)
    assert len(dev[0]) > 100 and _same(dev, eng.map_get())
    eng.set_target(pts, p)                                  # the target cloud as well
    eng.map_reset(0.25, 4.0, dim)
    eng.map_insert(T, which="target")
    assert _same(dev, eng.map_get())


# 7 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("min_points", [1, 3])
def test_map_as_target_equals_the_same_cloud_set_as_target(eng, min_points, dim):
    if dim == 3:
        src, tgt, _ = S.scene_pair_3d(20000)
        p, leaf = gicp.default_params(3, **P3), 0.5
    else:
        src, tgt, _ = S.segment_scene_2d(5000)
        p, leaf = gicp.default_params(2, **P2), 5.0
    eng.map_reset(leaf, 1000.0, dim)
    eng.map_insert(np.eye(dim + 1), points=tgt)
    eng.map_insert(np.eye(dim + 1), points=src)             # some voxels now hold several points
    cells, cent, cnt = eng.map_get()
    keep = cnt >= min_points
    assert 0 < keep.sum() and (min_points == 1 or keep.sum() < len(keep))
    eng.set_source(src, p)
    eng.map_to_target(p, min_points)
    other = gicp.Engine(0)
    try:
        other.set_target(cent[keep], p)
        other.set_source(src, p)
        assert eng.n_tgt == other.n_tgt == int(keep.sum()) and eng.dim == dim
        assert np.array_equal(eng.points("target"), cent[keep])
        assert np.array_equal(eng.points("target"), other.points("target"))
        assert np.array_equal(eng.covariances("target"), other.covariances("target"))
        assert np.array_equal(eng.neighbor_counts("target"), other.neighbor_counts("target"))
        assert _same(eng.graph(), other.graph())
        pa = gicp.default_params(dim, max_iterations=10, tolerance=0.0, fixed_iterations=1, **(P3 if dim == 3 else P2))
        Ta, ra = eng.align(None, pa)
        Tb, rb = other.align(None, pa)
        assert ra["correspondences"] > 0
        assert np.array_equal(Ta, Tb) and ra["final_loss"] == rb["final_loss"] and ra["iterations"] == rb["iterations"] == 10
    finally:
        other.close()


# 8 ---------------------------------------------------------------------------------------------------------
def _state_error(fn, match):
    with pytest.raises(_lib.GicpError, match=match) as ei:
        fn()
    assert ei.value.code == _lib.GICP_E_STATE


def test_errors_carry_the_library_text(eng):
    pts = np.random.default_rng(16).uniform(-1.0, 1.0, (100, 3))
    p = gicp.default_params(3, **P3)
    # before gicp_map_reset
    _state_error(lambda: eng.map_insert(np.eye(4), points=pts), "gicp_map_reset first")
    _state_error(lambda: eng.map_get(), "gicp_map_reset first")
    _state_error(lambda: eng.map_to_target(p), "gicp_map_reset first")
    assert eng.map_size() == 0
    for leaf, rng_, match in [(0.0, 1.0, "leaf"), (float("nan"), 1.0, "leaf"), (-1.0, 1.0, "leaf"), (float("inf"), 1.0, "leaf"),
                              (0.1, 0.0, "max_range"), (0.1, float("inf"), "max_range"), (0.1, -2.0, "max_range"),
                              (1e-3, 1e4, "window too wide")]:
        with pytest.raises(ValueError, match=match):
            eng.map_reset(leaf, rng_, 3)
    with pytest.raises(ValueError, match="dim"):
        eng.map_reset(0.1, 1.0, 4)
    eng.map_reset(1e-3, 1e4, 2)                              # 2 10^7 + 1 cells per axis fit 2-D's 2^31
    eng.map_reset(0.1, 5.0, 3)
    _state_error(lambda: eng.map_insert(np.eye(4), which="source"), "cloud not set")
    with pytest.raises(ValueError, match="empty"):
        eng.map_to_target(p)
    bad_T = np.eye(4)
    bad_T[1, 3] = np.nan
    with pytest.raises(ValueError, match="T contains non-finite"):
        eng.map_insert(bad_T, points=pts)
    far = np.eye(4)
    far[2, 3] = 0.1 * 2.0 ** 31
    with pytest.raises(ValueError, match="axis 2"):
        eng.map_insert(far, points=pts)
    bad = pts.copy()
    bad[3, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        eng.map_insert(np.eye(4), points=bad)
    with pytest.raises(ValueError, match="dimension differs"):
        eng.map_insert(np.eye(3), points=pts[:, :2])
    eng.set_source(pts[:, :2], gicp.default_params(2, **P2))
    eng.map_dim = 2
    with pytest.raises(ValueError, match="dimension differs"):
        eng.map_insert(np.eye(3), which="source")
    eng.map_dim = 3
    assert eng.map_size() == 0                               # nothing above changed the map
    eng.map_insert(np.eye(4), points=pts + 1000.0)           # every point outside the window: still empty
    assert eng.map_size() == 0
    with pytest.raises(ValueError, match="empty"):
        eng.map_to_target(p)
    eng.map_insert(np.eye(4), points=pts)
    with pytest.raises(ValueError, match="min_points"):
        eng.map_to_target(p, 10 ** 6)
    with pytest.raises(ValueError, match="min_points"):
        eng.map_to_target(p, 0)
    assert eng.map_size() > 0


def test_staged_targets_and_the_map_are_independent(eng):
    src, tgt, _ = S.scene_pair_3d(4000)
    p = gicp.default_params(3, max_iterations=5, **P3)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    eng.stage_target(tgt, p)
    eng.map_reset(0.2, 50.0, 3)
    eng.map_insert(np.eye(4), which="target")
    eng.map_to_target(p)                                     # cancels nothing
    m = eng.map_size()
    assert eng.n_tgt == m < len(tgt)
    eng.commit_target()                                      # the staged build is still there
    assert eng.n_tgt == len(tgt) and eng.n_src == m and eng.map_size() == m
    T, res = eng.align(None, p)
    assert np.all(np.isfinite(T)) and res["correspondences"] > 0


# 9 ---------------------------------------------------------------------------------------------------------
MAP_LEAF, MAP_RANGE = 0.4, 30.0


def test_scan_to_map_odometry_vs_oracle_and_truth():
    """Teacher-forced: the reference map is fed with the GPU's poses, so both maps hold the same cells, and every
    frame the oracle registers the scan against the reference map's centroids from the same start pose.
    Leaf 0.4 m and range 30 m: 4.1k .. 5.8k voxels on this stream; the oracle's own loop (its poses fed back)
    stays within 8.7e-4 rad and 0.036 m per frame of the generator's motion, against the bounds 2e-3 rad and
    0.1 m of tests/test_odometry.py."""
    from golden_util import pose_err
    from gicp.odometry import Odometry
    frames = list(S.lidar_stream(5, beams=16, azimuths=600, step=0.15, along_path=True))
    prm = dict(max_iterations=40, tolerance=1e-10, **P3)
    odo = Odometry(3, params=gicp.default_params(3, **prm), init="identity", map_voxel_size=MAP_LEAF, map_range=MAP_RANGE)
    s2s = Odometry(3, params=gicp.default_params(3, **prm), init="identity")
    ref = MapRef(3, MAP_LEAF, MAP_RANGE)
    try:
        for k, (scan, pose) in enumerate(frames):
            start = odo.pose.copy()
            T, res = odo.step(scan)
            s2s.step(scan)
            if T is None:
                ref.insert(scan, odo.pose)
                continue
            r_cent = ref.get()[1]
            Po, *_ = O.gicp(scan, r_cent, T0=start, **prm)
            a, t = pose_err(odo.pose, Po)
            print(f"frame {k}: map rows {len(r_cent)}, GPU vs oracle {a:.3e} rad {t:.3e} m, iterations {res['iterations']}")
            assert a < 1e-6 and t < 1e-5, (k, a, t)
            np.testing.assert_allclose(T, np.linalg.inv(odo.pose) @ start, atol=1e-12)
            Ttrue = np.linalg.inv(pose) @ frames[k - 1][1]
            assert S.rotation_angle_error(T, Ttrue) < 2e-3 and S.translation_error(T, Ttrue) < 0.1
            ref.insert(scan, odo.pose)
            cells = odo.eng.map_get()[0]
            assert np.array_equal(cells, ref.get()[0])       # identical cells: the same map on both sides
        end_true = np.linalg.inv(frames[0][1]) @ frames[-1][1]
        for name, o in (("scan-to-map", odo), ("scan-to-scan", s2s)):
            print(f"{name}: final pose error {S.rotation_angle_error(o.pose, end_true):.3e} rad, "
                  f"{S.translation_error(o.pose, end_true):.3e} m")
        assert len(odo.poses) == len(frames) and odo.timing["map_s"] > 0
    finally:
        odo.eng.close()
        s2s.eng.close()
