"""Motion compensation on the device (gicp_sweep.hip): the one-shot de-skew against the
matrix-exponential reference (tests/deskew_ref.py) and the host function, the de-skew fused into the cloud
builds against the unfused path bit for bit, errors and recovery, and Odometry(deskew=True) against a hand
loop."""
import functools

import numpy as np
import pytest

import deskew_ref as R

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from gicp.odometry import Odometry  # noqa: E402

pytestmark = pytest.mark.gpu

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
P2 = dict(max_distance_correspondence=20.0, max_distance_nearest_neighbors=25.0)


# ---- 1. the one-shot against the reference ---------------------------------------------------------------

@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_one_shot_against_expm_and_the_host_function(dim, n):
    """Every angle class at every wave edge: one point, a wave less one, a full wave, one more, and more than
    one block with a partial last wave.  The stamps repeat, go negative and exceed 1 (deskew_ref.case)."""
    for angle in R.ANGLES:
        pts, stamps, xi, M, want = R.case(dim, angle, n)
        got = gicp.deskew(pts, stamps, M, R.REF)
        what = f"gpu dim {dim} n {n} |w| {angle:g}"
        R.check_against_reference(got, pts, stamps, xi, want, what)
        R.check_against_reference(got, pts, stamps, xi, gicp.deskew_host(pts, stamps, M, R.REF), what + " vs host")
        at_ref = stamps == R.REF
        assert np.all(got[at_ref] == pts[at_ref])
    assert np.all(gicp.deskew(pts, stamps, np.eye(dim + 1), R.REF) == pts)


# ---- 2. determinism --------------------------------------------------------------------------------------

def test_determinism_across_calls_and_engines():
    e2 = gicp.Engine(0)
    try:
        for dim in (3, 2):
            pts, stamps, _, M, _ = R.case(dim, 0.3, 4097)
            a = gicp.deskew(pts, stamps, M, R.REF)
            assert np.array_equal(a, gicp.deskew(pts, stamps, M, R.REF))
            assert np.array_equal(a, e2.deskew(pts, stamps, M, R.REF))
    finally:
        e2.close()


# ---- 3. / 4. fused equals unfused, bit for bit -----------------------------------------------------------

def _motion(dim, angle, speed, seed=3):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim)
    v *= speed / np.linalg.norm(v)
    w = [angle] if dim == 2 else np.array([0.2, -0.1, 1.0]) * angle / np.linalg.norm([0.2, -0.1, 1.0])
    return R.motion_of(np.concatenate([w, v]))


def _stamps(n, seed):
    """Column-like stamps in [0, 1): 360 distinct values, repeated."""
    return np.random.default_rng(seed).integers(0, 360, n) / 360.0


@functools.lru_cache(maxsize=None)
def _sweeps(name):
    """(source, source stamps, target, target stamps, motion, ref, params, voxel leaf) of a case; read only."""
    if name == "room":                 # the 3000-point room under a typical sweep: 0.5 m, 2 degrees
        src, tgt, _ = S.scene_pair_3d(3000)
        out = (src, _stamps(len(src), 1), tgt, _stamps(len(tgt), 2), _motion(3, 0.035, 0.5), 0.5, P3, 1.0)
    elif name == "segments":           # a 2-D cloud (px): 5 px, 1 degree
        src, tgt, _ = S.segment_scene_2d(2000)
        out = (src, _stamps(len(src), 1), tgt, _stamps(len(tgt), 2), _motion(2, 0.0175, 5.0), 0.5, P2, 8.0)
    elif name == "lever":              # 1.5 rad per stamp unit on a 40 m lever arm: the de-skewed extent leaves the raw one
        rng = np.random.default_rng(4)
        src = np.array([40.0, 0.0, 1.0]) + rng.uniform(-1.0, 1.0, (2000, 3))
        tgt = np.array([40.0, 0.0, 1.0]) + rng.uniform(-1.0, 1.0, (2000, 3))
        M = R.motion_of(np.array([0.0, 0.0, 1.5, 0.3, 0.0, 0.0]))
        out = (src, _stamps(2000, 1), tgt, _stamps(2000, 2), M, 0.0, P3, 0.5)
    elif name == "negative":           # every coordinate negative before and after
        rng = np.random.default_rng(5)
        src, tgt = rng.uniform(-30.0, -20.0, (2000, 3)), rng.uniform(-30.0, -20.0, (2000, 3))
        out = (src, _stamps(2000, 1), tgt, _stamps(2000, 2), _motion(3, 0.035, 0.5), 0.5, P3, 1.0)
    elif name == "zeros":              # the room flattened onto z = -0.0, moved in its plane; some x = -0.0 at the reference stamp
        src, tgt, _ = S.scene_pair_3d(3000)
        src, tgt = src.copy(), tgt.copy()
        src[:, 2] = tgt[:, 2] = -0.0
        ss, st = _stamps(len(src), 1), _stamps(len(tgt), 2)
        for c, s in ((src, ss), (tgt, st)):
            c[:40, 0] = -0.0
            s[:20] = 0.5
        M = R.motion_of(np.array([0.0, 0.0, 0.035, 0.4, 0.3, 0.0]))
        out = (src, ss, tgt, st, M, 0.5, P3, 0.5)
    else:
        raise KeyError(name)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def _state(e, T):
    """Everything the comparison covers, read from an engine with both clouds set."""
    out = {}
    for which in ("target", "source"):
        out[which] = (e.points(which), e.covariances(which), e.neighbor_counts(which))
    out["graph"] = e.graph()
    out["stats"] = e.iterate(T, debug=True)
    return out


def _assert_same(a, b, what):
    for which in ("target", "source"):
        for x, y, part in zip(a[which], b[which], ("points", "covariances", "neighbor_counts")):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, which, part)
    assert np.array_equal(a["graph"][0], b["graph"][0]) and np.array_equal(a["graph"][1], b["graph"][1]), (what, "graph")
    (sa, da), (sb, db) = a["stats"], b["stats"]
    assert sa[-1] > 0, (what, "no correspondences")
    assert np.array_equal(sa, sb), (what, "statistics")
    for k in da:
        assert np.array_equal(da[k], db[k]), (what, k)


@functools.lru_cache(maxsize=None)
def _unfused(name, voxel):
    """The reference of a case: plain builds of gicp.deskew's output, computed once."""
    src, ss, tgt, st, M, ref, P, leaf = _sweeps(name)
    dim = src.shape[1]
    p = gicp.default_params(dim, **P)
    d_src, d_tgt = gicp.deskew(src, ss, M, ref), gicp.deskew(tgt, st, M, ref)
    e = gicp.Engine(0)
    try:
        if voxel:
            e.set_voxel(leaf)
        e.set_target(d_tgt, p)
        e.set_source(d_src, p)
        if not voxel:
            assert np.array_equal(e.points("target"), d_tgt) and np.array_equal(e.points("source"), d_src)
        else:
            assert e.cloud_size("target") < len(tgt)
        return _state(e, np.eye(dim + 1))
    finally:
        e.close()


def _fused(name, voxel, how):
    src, ss, tgt, st, M, ref, P, leaf = _sweeps(name)
    dim = src.shape[1]
    p = gicp.default_params(dim, **P)
    e = gicp.Engine(0)
    try:
        if voxel:
            e.set_voxel(leaf)
        if how == "set":
            e.set_target(tgt, p, stamps=st, motion=M, ref=ref)
        else:
            e.stage_target(tgt, p, borrow=how == "borrow", stamps=st, motion=M, ref=ref)
            e.commit_target()
        e.set_source(src, p, stamps=ss, motion=M, ref=ref)
        return _state(e, np.eye(dim + 1))
    finally:
        e.close()


@pytest.mark.parametrize("voxel", [False, True], ids=["plain", "voxel"])
@pytest.mark.parametrize("how", ["set", "stage", "borrow"])
@pytest.mark.parametrize("name", ["room", "segments"])
def test_fused_equals_unfused_bit_for_bit(name, how, voxel):
    _assert_same(_fused(name, voxel, how), _unfused(name, voxel), (name, how, voxel))


@pytest.mark.parametrize("voxel", [False, True], ids=["plain", "voxel"])
@pytest.mark.parametrize("name", ["lever", "negative", "zeros"])
def test_bounds_are_those_of_the_deskewed_points(name, voxel):
    """Raw bounds, or an ordered-integer encoding that mishandles a sign, give another Morton frame (and with
    the filter other cells): the index, the covariances' order of summation and the graph then differ."""
    src, ss, tgt, st, M, ref, _, _ = _sweeps(name)
    d_tgt = gicp.deskew(tgt, st, M, ref)
    if name == "lever":
        assert d_tgt[:, 1].max() > tgt[:, 1].max() + 20.0 and d_tgt[:, 0].min() < tgt[:, 0].min() - 20.0
    if name == "negative":
        assert d_tgt.max() < 0.0 and gicp.deskew(src, ss, M, ref).max() < 0.0
    if name == "zeros":
        assert np.all(d_tgt[:, 2] == 0.0) and np.signbit(tgt[:, 2]).all()
    _assert_same(_fused(name, voxel, "set"), _unfused(name, voxel), (name, voxel))


# ---- 5. errors and recovery ------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["source", "target"])
@pytest.mark.parametrize("fault", ["nan_stamp", "not_rigid"])
def test_a_refused_sweep_leaves_no_half_built_cloud(which, fault):
    src, ss, tgt, st, M, ref, P, _ = _sweeps("room")
    p = gicp.default_params(3, **P)
    T = np.eye(4)
    e = gicp.Engine(0)
    try:
        e.set_target(tgt, p, stamps=st, motion=M, ref=ref)
        e.set_source(src, p, stamps=ss, motion=M, ref=ref)
        other = "target" if which == "source" else "source"
        before = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        pts, stamps = (src, ss) if which == "source" else (tgt, st)
        bad_stamps, bad_M = np.array(stamps), np.array(M)
        if fault == "nan_stamp":
            bad_stamps[len(stamps) // 2] = np.nan
            text = "non-finite stamps"
        else:
            bad_M[:3, :3] *= 1.0 + 1e-6
            text = "motion is not rigid"
        build = e.set_source if which == "source" else e.set_target
        with pytest.raises(ValueError, match=text):
            build(pts, p, stamps=bad_stamps, motion=bad_M, ref=ref)
        assert e.cloud_size(which) == 0                       # NOT SET
        with pytest.raises(_lib.GicpError) as ei:
            e.iterate(T)
        assert ei.value.code == _lib.GICP_E_STATE
        with pytest.raises(_lib.GicpError):
            e.covariances(which)
        after = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        assert all(np.array_equal(x, y) for x, y in zip(before, after))   # the other cloud is untouched
        build(pts, p, stamps=stamps, motion=M, ref=ref)       # a good rebuild: a fresh context's bits
        _assert_same(_state(e, T), _unfused("room", False), (which, fault))
        # refused before the build begins: a staged sweep no build would take uses no slot
        with pytest.raises(ValueError, match="motion is not rigid"):
            e.stage_target(tgt, p, stamps=st, motion=np.array(M) * 1.001, ref=ref)
        with pytest.raises(_lib.GicpError):
            e.commit_target()                                  # nothing was staged
        with pytest.raises(ValueError, match="non-finite stamps"):
            e.deskew(pts, bad_stamps if fault == "nan_stamp" else np.full(len(pts), np.inf), M, ref)
    finally:
        e.close()


# ---- 6. Odometry against a hand loop ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stream():
    scans = [f for f, _ in S.lidar_stream_skewed(5, beams=16, azimuths=600, step=0.15, along_path=True)]
    for f in scans:
        f.setflags(write=False)
    return tuple(scans)


def _params():
    return gicp.default_params(3, max_iterations=30, tolerance=1e-9, **P3)


MAP = dict(map_voxel_size=0.5, map_range=40.0)


def _poses(odo, scans, how):
    try:
        if how == "run":
            for _ in odo.run(list(scans), depth=1):
                pass
        else:
            for s in scans:
                odo.step(s)
        return [P.copy() for P in odo.poses]
    finally:
        odo.eng.close()


def test_odometry_scan_to_map_equals_a_hand_loop():
    """Scan-to-map: frame k is de-skewed by P_{k-2}^-1 P_{k-1} of the poses found so far (the identity before
    there are two), to mid-sweep.  The hand loop predicts that from a plain Odometry's poses, de-skews with
    gicp.deskew (another context) and feeds the plain Odometry: every pose has the same bits."""
    scans = _stream()
    got = _poses(Odometry(3, params=_params(), deskew=True, **MAP), scans, "step")
    plain = Odometry(3, params=_params(), **MAP)
    try:
        for s in scans:
            P = plain.poses
            M = np.linalg.inv(P[-2]) @ P[-1] if len(P) >= 2 else np.eye(4)
            plain.step(gicp.deskew(s[:, :3], s[:, 3], M, 0.5))
        want = [P.copy() for P in plain.poses]
    finally:
        plain.eng.close()
    assert len(got) == len(want) == len(scans)
    assert np.linalg.norm(want[-1][:3, 3]) > 0.3            # it moved: 4 steps of 0.15 m
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), k


@pytest.mark.parametrize("how", ["run", "step"])
def test_odometry_scan_to_scan_equals_a_hand_loop(how):
    """Scan-to-scan: the motion is the inverse of the latest registration known when the scan's build starts.
    step() builds frame k after registration k - 1; run(depth=1) stages frame k during step k - 1, before that
    step's registration, so it knows registration k - 2 (the identity while there is none)."""
    scans = _stream()
    got = _poses(Odometry(3, params=_params(), deskew=True), scans, how)
    lag = 2 if how == "run" else 1
    plain = Odometry(3, params=_params())
    try:
        Ts = [None]                                          # Ts[k]: registration of frame k against k - 1
        for k, s in enumerate(scans):
            known = Ts[k - lag] if k - lag >= 1 else None
            M = np.linalg.inv(known) if known is not None else np.eye(4)
            T, _ = plain.step(gicp.deskew(s[:, :3], s[:, 3], M, 0.5))
            if k:
                Ts.append(T)
        want = [P.copy() for P in plain.poses]
    finally:
        plain.eng.close()
    assert len(got) == len(want) == len(scans)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), k


@pytest.mark.parametrize("mode", ["scan", "map"])
def test_odometry_without_deskew_ignores_the_stamp_column(mode):
    scans = _stream()
    kw = MAP if mode == "map" else {}
    got = _poses(Odometry(3, params=_params(), deskew=False, **kw), scans, "step")
    want = _poses(Odometry(3, params=_params(), **kw), [np.ascontiguousarray(s[:, :3]) for s in scans], "step")
    assert len(got) == len(scans) and all(np.array_equal(a, b) for a, b in zip(got, want))
