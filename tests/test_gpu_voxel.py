"""Voxel-grid downsampling on the device (gicp_voxel.hip): the one-shot call against the NumPy restatement
(tests/voxel_ref.py), and the filter fused into the cloud builds against the unfused path, bit for bit."""
import functools

import numpy as np
import pytest

from voxel_ref import voxel_abs_max, voxel_ref

gicp = pytest.importorskip("gicp")
from gicp import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
P2 = dict(max_distance_correspondence=20.0, max_distance_nearest_neighbors=25.0)


def _points(name, dim):
    """The clouds of the cases below, (points, leaf)."""
    rng = np.random.default_rng(5)
    if name.startswith("n"):           # wave edges of the segmented scan: several points per voxel
        return rng.uniform(-1.0, 1.0, (int(name[1:]), dim)), 0.5
    if name == "uniform_0.1":          # a leaf no double represents
        return rng.uniform(-8.0, 8.0, (20000, dim)), 0.1
    if name == "uniform_0.25":         # an exact leaf
        return rng.uniform(-8.0, 8.0, (20000, dim)), 0.25
    if name == "uniform_1":            # ~5 points per voxel in 3-D (the min_points cases)
        return rng.uniform(-8.0, 8.0, (20000, dim)), 1.0
    if name == "lattice":              # every point exactly on a cell face, negative coordinates included
        return rng.integers(-12, 12, (3000, dim)) * 0.25, 0.25
    if name == "dense_between":        # one voxel of 5,000 points (79 waves) between sparse neighbours
        dense = rng.uniform(10.0, 11.0, (5000, dim))
        sparse = rng.uniform(0.0, 20.0, (300, dim))
        pts = np.concatenate([sparse[:150], dense, sparse[150:]])
        return pts[rng.permutation(len(pts))], 1.0
    if name == "single_voxel":         # all 10,000 points in one voxel
        return rng.uniform(3.0, 3.25, (10000, dim)), 0.25
    if name == "widest":               # the widest accepted key: 2^21 cells per axis in 3-D (63 bits), 2^31 in 2-D (62)
        return _widest(dim)[0], 1.0
    raise KeyError(name)


WIDEST_LOW = {3: (-1234567, -7, -2000001), 2: (-1234567891, -3)}     # lowest cells: negative, no powers of two


def _widest(dim):
    """(points, lowest cell per axis, highest cell per axis): about 3000 points at cell + 0.5 (leaf 1.0, exact in
    fp64) whose cells span exactly 2^21 (3-D) or 2^31 (2-D) cells on every axis: both extreme corner cells (key
    0 and the all-ones key), 70 points in one cell, a cell next to each corner, the rest scattered."""
    rng = np.random.default_rng(17)
    span = 2 ** 21 if dim == 3 else 2 ** 31
    lo = np.array(WIDEST_LOW[dim], dtype=np.int64)
    hi = lo + span - 1
    cells = rng.integers(0, span, (2900, dim)) + lo
    one = lo + span // 3
    step = np.eye(dim, dtype=np.int64)
    cells = np.concatenate([cells, lo[None], hi[None], lo + step, hi - step, np.tile(one, (70, 1))])
    cells = cells[rng.permutation(len(cells))]
    return cells.astype(np.float64) + 0.5, lo, hi


@functools.lru_cache(maxsize=None)
def _case(name, dim, min_points=1):
    """(points, leaf, gpu centroids, gpu counts, reference centroids, counts, cells, max |x| per voxel):
    computed once per case and shared by the tests (read only)."""
    pts, leaf = _points(name, dim)
    g_xyz, g_cnt = gicp.voxel_downsample(pts, leaf, min_points=min_points, return_counts=True)
    r_xyz, r_cnt, r_cells = voxel_ref(pts, leaf, min_points)
    out = (pts, leaf, g_xyz, g_cnt, r_xyz, r_cnt, r_cells, voxel_abs_max(pts, leaf, min_points))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _check_exact(case):
    pts, leaf, g_xyz, g_cnt, r_xyz, r_cnt, r_cells, _ = case
    assert g_xyz.shape == r_xyz.shape and g_cnt.dtype == np.int32
    assert np.array_equal(np.floor(g_xyz / leaf), r_cells)      # the kept cells and their order
    assert np.array_equal(g_cnt, r_cnt)


def _check_centroids(case):
    """|gpu - ref| <= count 2^-51 max|x_a| per coordinate: either side's sum of `count` doubles errs by at
    most (count - 1) 2^-53 sum|x| <= (count - 1) 2^-53 count max|x|, so its mean by (count - 1) 2^-53 max|x|,
    plus one rounding of the division (2^-53 max|x|): count 2^-53 max|x| per side, 2^-52 for both, and a
    factor 2 of slack."""
    _, _, g_xyz, g_cnt, r_xyz, r_cnt, _, amax = case
    bound = r_cnt[:, None] * 2.0 ** -51 * amax
    err = np.abs(g_xyz - r_xyz)
    print("max centroid error / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


CASES = ["n1", "n63", "n64", "n65", "n129", "uniform_0.1", "uniform_0.25", "lattice"]


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("name", CASES)
def test_membership_and_order_are_exact(name, dim):
    _check_exact(_case(name, dim))


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("name", CASES)
def test_centroids_within_the_derived_bound(name, dim):
    _check_centroids(_case(name, dim))


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("name", ["dense_between", "single_voxel"])
def test_voxels_that_span_waves(name, dim):
    case = _case(name, dim)
    _check_exact(case)
    _check_centroids(case)
    assert case[3].max() >= 5000
    if name == "single_voxel":
        assert len(case[2]) == 1 and case[3][0] == 10000


@pytest.mark.parametrize("dim", [3, 2])
def test_widest_accepted_key(dim):
    """Cells spanning exactly the limit on every axis (63 key bits in 3-D, 62 in 2-D), the lowest cell negative:
    membership, order and counts exact against voxel_ref, centroids within the derived bound, the first and the
    last row the two corner cells; one more point one cell beyond the range, on each axis and either side in
    turn, is the first refused key."""
    case = _case("widest", dim)
    _check_exact(case)
    _check_centroids(case)
    pts, lo, hi = _widest(dim)
    cells, cnt = case[6], case[3]
    span = 2 ** 21 if dim == 3 else 2 ** 31
    assert np.array_equal(cells.max(axis=0) - cells.min(axis=0) + 1, np.full(dim, span))
    assert np.array_equal(cells[0], lo) and np.array_equal(cells[-1], hi) and np.all(lo < 0)
    assert cnt.max() == 70 and len(cells) > 2900
    assert np.array_equal(case[2], cells + 0.5)                 # every centroid is its cell's centre, exactly
    for a in range(dim):
        for edge, step in ((hi, 1), (lo, -1)):
            beyond = edge.astype(np.float64) + 0.5
            beyond[a] += step
            with pytest.raises(ValueError, match=f"voxel grid too wide: axis {a}"):
                gicp.voxel_downsample(np.concatenate([pts, beyond[None]]), 1.0)
    again = gicp.voxel_downsample(pts, 1.0, return_counts=True)          # ... and a refusal changes nothing
    assert np.array_equal(again[0], case[2]) and np.array_equal(again[1], cnt)


def test_determinism_across_calls_and_engines():
    pts, leaf = _points("uniform_0.25", 3)
    dense, dleaf = _points("dense_between", 3)
    a = gicp.voxel_downsample(pts, leaf, return_counts=True)
    b = gicp.voxel_downsample(pts, leaf, return_counts=True)
    e2 = gicp.Engine(0)
    try:
        c = e2.voxel_downsample(pts, leaf, return_counts=True)
        d2 = e2.voxel_downsample(dense, dleaf)
    finally:
        e2.close()
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
    assert np.array_equal(gicp.voxel_downsample(dense, dleaf), d2)


@pytest.mark.parametrize("min_points", [2, 5])
def test_min_points_equals_reference(min_points):
    """The 20k uniform cloud at leaf 1: 4096 cells of ~4.9 points each, so both thresholds drop some voxels
    and keep others (at leaf 0.1 or 0.25 no voxel of this cloud holds 5 points)."""
    case = _case("uniform_1", 3, min_points)
    _check_exact(case)
    _check_centroids(case)
    full = _case("uniform_1", 3)
    assert 0 < len(case[2]) < len(full[2]) and case[3].min() >= min_points


def test_invalid_arguments_raise_with_the_library_text():
    pts, _ = _points("uniform_0.25", 3)
    with pytest.raises(ValueError, match="min_points"):
        gicp.voxel_downsample(pts, 0.25, min_points=10 ** 6)
    for leaf in (0.0, float("nan"), -1.0):
        with pytest.raises(ValueError, match="leaf must be finite and > 0"):
            gicp.voxel_downsample(pts, leaf)
    far = np.array([[0.0, 0.0, 0.0], [1e9, 0.0, 0.0]])
    with pytest.raises(ValueError, match="voxel grid too wide"):
        gicp.voxel_downsample(far, 1e-3)
    bad = pts.copy()
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        gicp.voxel_downsample(bad, 0.25)
    e = gicp.Engine(0)
    try:
        with pytest.raises(ValueError, match="leaf"):
            e.set_voxel(-0.5)
        with pytest.raises(ValueError, match="min_points"):
            e.set_voxel(0.1, 0)
    finally:
        e.close()


def _pair(dim):
    if dim == 3:
        src, tgt, _ = S.scene_pair_3d(20000)
        return src, tgt, gicp.default_params(3, **P3)
    src, tgt, _ = S.segment_scene_2d(5000)
    return src, tgt, gicp.default_params(2, **P2)


@pytest.mark.parametrize("dim", [3, 2])
def test_fused_equals_unfused_bit_for_bit(dim):
    src, tgt, p = _pair(dim)
    leaf = 0.1
    fsrc, ftgt = gicp.voxel_downsample(src, leaf), gicp.voxel_downsample(tgt, leaf)
    assert len(fsrc) < len(src) or dim == 2
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        a.set_voxel(leaf)
        a.set_target(tgt, p)
        a.set_source(src, p)
        b.set_target(ftgt, p)
        b.set_source(fsrc, p)
        for which, f in (("target", ftgt), ("source", fsrc)):
            assert a.cloud_size(which) == b.cloud_size(which) == len(f)
            assert np.array_equal(a.points(which), f) and np.array_equal(b.points(which), f)
            assert np.array_equal(a.covariances(which), b.covariances(which))
            assert np.array_equal(a.neighbor_counts(which), b.neighbor_counts(which))
        T = np.eye(dim + 1)
        sa, da = a.iterate(T, debug=True)
        sb, db = b.iterate(T, debug=True)
        assert sa[-1] > 0
        assert np.array_equal(sa, sb) and np.array_equal(da["index"], db["index"])
    finally:
        a.close()
        b.close()


def test_filter_off_is_the_unfiltered_build():
    src, tgt, p = _pair(3)
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        a.set_voxel(0.1)
        a.set_target(tgt, p)
        a.set_source(src, p)
        assert a.cloud_size("target") < len(tgt)
        a.set_voxel(0)
        a.set_target(tgt, p)
        a.set_source(src, p)
        b.set_target(tgt, p)
        b.set_source(src, p)
        assert a.cloud_size("target") == len(tgt) and a.cloud_size("source") == len(src)
        assert np.array_equal(a.points("source"), src)
        T = np.eye(4)
        assert np.array_equal(a.iterate(T), b.iterate(T))
    finally:
        a.close()
        b.close()


def test_stream_paths_agree_and_equal_the_prefiltered_pairs():
    from gicp.odometry import Odometry
    leaf = 0.25
    frames = [f for f, _ in S.lidar_stream(6, beams=16, azimuths=400)]
    prm = dict(max_iterations=30, tolerance=1e-9, **P3)
    out = {}
    for mode in ("sync", "staged", "borrow"):
        odo = Odometry(3, params=gicp.default_params(3, **prm), voxel_size=leaf, borrow=mode == "borrow")
        try:
            if mode == "sync":
                out[mode] = [odo.step(f)[0] for f in frames]
            else:
                out[mode] = [T for T, _ in odo.run(frames, depth=2)]
            assert odo.eng.cloud_size("target") < len(frames[-1])
        finally:
            odo.eng.close()
    # Engine.align on the pre-filtered pairs, scans promoted and started as the stream does
    filt = [gicp.voxel_downsample(f, leaf) for f in frames]
    p = gicp.default_params(3, **prm)
    e = gicp.Engine(0)
    ref = [None]
    try:
        e.set_target(filt[0], p)
        for f in filt[1:]:
            e.target_to_source()
            e.set_target(f, p)
            ref.append(e.align(ref[-1], p)[0])
    finally:
        e.close()
    for mode in out:
        assert len(out[mode]) == len(frames) and out[mode][0] is None
        for k in range(1, len(frames)):
            assert np.array_equal(out[mode][k], ref[k]), (mode, k)


def test_drop_in_with_voxel_size():
    src, tgt, _ = S.scene_pair_3d(20000)
    kw = dict(max_iterations=10, tolerance=1e-9, verbose=False, **P3)
    fsrc, ftgt = gicp.voxel_downsample(src, 0.1), gicp.voxel_downsample(tgt, 0.1)
    out = gicp.gicp(src, tgt, voxel_size=0.1, **kw)
    ref = gicp.gicp(fsrc, ftgt, **kw)
    assert out[2].shape == (len(fsrc), 3, 3) and out[3].shape == (len(ftgt), 3, 3)
    assert np.max(np.abs(out[0] - ref[0])) <= 1e-9
    assert len(out[4]) == len(ref[4]) and all(np.array_equal(x, y) for x, y in zip(out[4], ref[4]))
    assert gicp._engine(0).voxel == (0.0, 1)     # the shared engine's setting does not outlive the call
