"""Motion compensation, the parts that need no GPU: the skewed-sweep generator's conventions,
the host twist and the host de-skew against the matrix-exponential reference (tests/deskew_ref.py), the
refusals, and the new entry points' argument checks, which must not touch HIP."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import expm, logm

import deskew_ref as R

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402


def _twist_of(X):
    return np.array([X[2, 1], X[0, 2], X[1, 0], X[0, 3], X[1, 3], X[2, 3]])


def test_generator_casts_every_ray_from_the_pose_at_its_stamp():
    """One noise-free skewed sweep: moved to the frame at `ref` by the reference de-skew under the true motion
    and then to the world by the pose the generator reports, every point lies where its own ray's pose
    P_k expm(tau log(M)) puts it, to 1e-9 m.  This pins M = P(tau)^-1 P(tau + 1), the sign of tau - ref and
    the frame of the reported pose.  The world points also lie on the scene, within the caster's reach."""
    ref = 0.5
    kw = dict(beams=8, azimuths=200, seed=7, step=0.5)
    (scan, pose), = S.lidar_stream_skewed(1, ref=ref, noise=0.0, **kw)
    P = S.lidar_trajectory(2, seed=7, step=0.5)
    assert scan.shape[1] == 4 and len(scan) > 1000
    assert set(np.unique(scan[:, 3])) <= set(S.lidar_stamps(8, 200))
    X = logm(np.linalg.inv(P[0]) @ P[1]).real
    xi = _twist_of(X)
    assert np.max(np.abs(pose - P[0] @ expm(ref * X))) <= 1e-12
    at_ref = R.deskew_ref(scan[:, :3], scan[:, 3], xi, ref)
    world = at_ref @ pose[:3, :3].T + pose[:3, 3]
    want = np.empty_like(world)
    for tau in np.unique(scan[:, 3]):
        Pt = P[0] @ expm(tau * X)
        m = scan[:, 3] == tau
        want[m] = scan[m, :3] @ Pt[:3, :3].T + Pt[:3, 3]
    assert np.max(np.abs(world - want)) <= 1e-9
    # the skew is real: the raw points, posed at `ref`, miss by centimetres
    raw = scan[:, :3] @ pose[:3, :3].T + pose[:3, 3]
    assert np.max(np.linalg.norm(raw - want, axis=1)) > 0.1
    # every world point is on a surface of the room: inside its walls, to rounding
    assert np.all(np.abs(want[:, :2]) <= 20.0 + 1e-9) and np.all((want[:, 2] >= -1e-9) & (want[:, 2] <= 8.0 + 1e-9))


def test_lidar_stamps_and_per_ray_caster():
    st = S.lidar_stamps(3, 4)
    assert np.array_equal(st, np.tile([0.0, 0.25, 0.5, 0.75], 3))
    # with one origin for every ray the per-ray caster finds the ranges lidar_scan's caster finds
    scene = S.lidar_scene()
    pose = S.lidar_trajectory(1)[0]
    dirs = S.lidar_dirs(4, 50)
    pts = S.lidar_scan(scene, pose, dirs, np.random.default_rng(0), noise=0.0)
    best = S.lidar_cast(scene, np.broadcast_to(pose[:3, 3], dirs.shape), dirs @ pose[:3, :3].T)
    hit = np.isfinite(best)
    assert hit.sum() == len(pts)
    assert np.allclose(np.linalg.norm(pts, axis=1), best[hit], rtol=0, atol=1e-12)


def test_se3_exp_and_log_against_expm():
    for k, ang in enumerate(R.ANGLES):
        xi = R.twist(3, ang, k)
        T = S.se3_exp(xi)
        assert np.max(np.abs(T - R.motion_of(xi))) <= 1e-13
        assert np.max(np.abs(S.se3_log(T) - xi)) <= 1e-12 * (1 + R.SPEED)


@pytest.mark.parametrize("dim", [2, 3])
def test_twist_recovers_the_generating_twist(dim):
    """gicp_motion_twist(expm(xi^)) = xi to 1e-12 (1 + max|xi|): the matrix exponential is accurate to a few
    ulp of its entries (<= 1 in R, <= |v| in t), and Log at no more than a quarter turn amplifies that by a
    factor of order one; a careful fp64 Log measures 5.5e-16 of this scale."""
    worst = 0.0
    for k, ang in enumerate(R.ANGLES):
        for seed in range(4):
            xi = R.twist(dim, ang, 10 * k + seed)
            got = gicp.motion_twist(R.motion_of(xi))
            worst = max(worst, float(np.max(np.abs(got - xi)) / (1.0 + np.max(np.abs(xi)))))
    print(f"twist dim {dim}: max error / scale = {worst:.3e}")
    assert worst <= 1e-12
    assert np.array_equal(gicp.motion_twist(np.eye(dim + 1)), np.zeros(3 if dim == 2 else 6))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("angle", R.ANGLES)
def test_host_deskew_against_expm(dim, angle):
    pts, stamps, xi, M, want = R.case(dim, angle, 200)
    got = gicp.deskew_host(pts, stamps, M, R.REF)
    R.check_against_reference(got, pts, stamps, xi, want, f"host dim {dim} |w| {angle:g}")


@pytest.mark.parametrize("dim", [2, 3])
def test_zero_shift_and_zero_twist_return_the_input_exactly(dim):
    pts, stamps, xi, M, _ = R.case(dim, 0.3, 200)
    got = gicp.deskew_host(pts, stamps, M, R.REF)
    at_ref = stamps == R.REF
    assert at_ref.sum() == 40 and np.all(got[at_ref] == pts[at_ref])
    assert np.all(got[~at_ref] != pts[~at_ref])
    assert np.all(gicp.deskew_host(pts, stamps, np.eye(dim + 1), R.REF) == pts)
    # the last row of the motion is not read
    M2 = M.copy()
    M2[dim] = np.nan
    assert np.array_equal(gicp.deskew_host(pts, stamps, M2, R.REF), got)


def _bad_motions(dim):
    good = R.motion_of(R.twist(dim, 0.3, 1))
    nan = good.copy()
    nan[0, dim] = np.nan
    inf = good.copy()
    inf[1, 0] = np.inf
    scaled = good.copy()
    scaled[:dim, :dim] *= 1.0 + 1e-8                    # max|R^T R - I| = 2e-8 > 1e-9
    sheared = good.copy()
    sheared[0, 1] += 1e-6
    mirror = good.copy()
    mirror[:dim, 0] *= -1.0                             # orthogonal, det -1
    turn = R.motion_of(R.twist(dim, 1.6, 1))            # just past a quarter turn
    half = R.motion_of(R.twist(dim, 3.0, 1))
    return dict(nan=nan, inf=inf, scaled=scaled, sheared=sheared, mirror=mirror, turn=turn, half=half)


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(dim):
    pts, stamps, xi, M, _ = R.case(dim, 0.3, 200)
    lib = _lib.load()
    out = np.full_like(pts, -7.0)
    xi_out = np.full(6, -7.0)
    for name, bad in _bad_motions(dim).items():
        bad = np.ascontiguousarray(bad)
        assert lib.gicp_motion_twist(dim, _lib.dptr(bad), _lib.dptr(xi_out)) == _lib.GICP_E_INVALID, name
        rc = lib.gicp_deskew_host(_lib.dptr(pts), _lib.dptr(stamps), len(pts), dim, _lib.dptr(bad), R.REF, _lib.dptr(out))
        assert rc == _lib.GICP_E_INVALID and np.all(out == -7.0), name
        with pytest.raises(ValueError):
            gicp.deskew_host(pts, stamps, bad, R.REF)
    # a motion just inside the limits is taken: a rotation orthogonal to 1e-10, a turn just short of a quarter
    near = np.array(M)
    near[:dim, :dim] *= 1.0 + 2e-11
    assert lib.gicp_motion_twist(dim, _lib.dptr(near), _lib.dptr(xi_out)) == _lib.GICP_OK
    gicp.motion_twist(R.motion_of(R.twist(dim, 1.55, 1)))
    Mc = np.ascontiguousarray(M)
    for bad_ref in (np.nan, np.inf):
        rc = lib.gicp_deskew_host(_lib.dptr(pts), _lib.dptr(stamps), len(pts), dim, _lib.dptr(Mc), bad_ref, _lib.dptr(out))
        assert rc == _lib.GICP_E_INVALID and np.all(out == -7.0)
    for bad_stamp in (np.nan, np.inf, -np.inf):
        st = np.array(stamps)
        st[137] = bad_stamp
        rc = lib.gicp_deskew_host(_lib.dptr(pts), _lib.dptr(st), len(pts), dim, _lib.dptr(Mc), R.REF, _lib.dptr(out))
        assert rc == _lib.GICP_E_INVALID and np.all(out == -7.0)
    rc = lib.gicp_deskew_host(_lib.dptr(pts), None, len(pts), dim, _lib.dptr(Mc), R.REF, _lib.dptr(out))   # stamps == NULL
    assert rc == _lib.GICP_E_INVALID and np.all(out == -7.0)
    badp = np.array(pts)
    badp[3, 1] = np.nan
    rc = lib.gicp_deskew_host(_lib.dptr(badp), _lib.dptr(stamps), len(pts), dim, _lib.dptr(Mc), R.REF, _lib.dptr(out))
    assert rc == _lib.GICP_E_INVALID and np.all(out == -7.0)
    for d in (1, 4):
        assert lib.gicp_motion_twist(d, _lib.dptr(Mc), _lib.dptr(xi_out)) == _lib.GICP_E_INVALID
    with pytest.raises(ValueError, match="one value per point"):
        gicp.deskew_host(pts, stamps[:-1], M, R.REF)
    with pytest.raises(ValueError, match="motion must be"):
        gicp.deskew_host(pts, stamps, np.eye(dim + 2), R.REF)


def test_null_context_is_invalid_without_hip():
    lib = _lib.load()
    pts = np.zeros((4, 3))
    st = np.zeros(4)
    out = np.full((4, 3), -7.0)
    M = np.eye(4)
    assert lib.gicp_deskew(None, _lib.dptr(pts), _lib.dptr(st), 4, 3, _lib.dptr(M), 0.0, _lib.dptr(out)) == _lib.GICP_E_INVALID
    assert np.all(out == -7.0)
    sw = _lib.Sweep()
    sw.stamps = _lib.dptr(st)
    for k, v in enumerate(M.ravel()):
        sw.motion[k] = v
    p = gicp.default_params(3)
    assert lib.gicp_set_target_sweep(None, _lib.dptr(pts), 4, 3, C.byref(p), C.byref(sw)) == _lib.GICP_E_INVALID
    assert lib.gicp_set_source_sweep(None, _lib.dptr(pts), 4, 3, C.byref(p), 0, 1, C.byref(sw)) == _lib.GICP_E_INVALID
    assert lib.gicp_stage_target_sweep(None, _lib.dptr(pts), 4, 3, C.byref(p), 0, C.byref(sw)) == _lib.GICP_E_INVALID
    assert lib.gicp_set_target_sweep(None, _lib.dptr(pts), 4, 3, C.byref(p), None) == _lib.GICP_E_INVALID


def test_new_entry_points_are_bound_and_hashed():
    for name in ("gicp_motion_twist", "gicp_deskew_host", "gicp_deskew", "gicp_set_target_sweep",
                 "gicp_set_source_sweep", "gicp_stage_target_sweep"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.load().gicp_version() >= 102
    i = _lib.HASH_SRCS.index("csrc/gicp_sweep.hip")
    assert _lib.HASH_SRCS[i - 1] == "csrc/gicp_voxel.hip" and "csrc/gicp_sweep.h" in _lib.HASH_SRCS
    assert C.sizeof(_lib.Sweep) == 8 + 8 + 16 * 8
    for f in (gicp.deskew, gicp.deskew_host, gicp.motion_twist):
        assert callable(f)
    assert hasattr(gicp.Engine, "deskew")
    import inspect
    for m in ("set_target", "set_source", "stage_target"):
        assert {"stamps", "motion", "ref"} <= set(inspect.signature(getattr(gicp.Engine, m)).parameters)
    from gicp.odometry import Odometry
    sig = inspect.signature(Odometry.__init__).parameters
    assert sig["deskew"].default is False and sig["deskew_ref"].default == 0.5
