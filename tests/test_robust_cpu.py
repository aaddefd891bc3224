"""CPU-side checks of the robust kernels (include/gicp_hip.h GICP_ROBUST_*): the parameters
and their names, the refusals that need no device, the NumPy reference's weight functions, and what the
kernels are for -- the outlier scene of tests/robust_ref.py, run with the reference loop alone."""
import ctypes as C

import numpy as np
import pytest

import fake_device
import robust_ref as R
from oracle import gicp_oracle as O

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402


def test_defaults_and_names():
    for dim in (2, 3):
        p = gicp.default_params(dim)
        assert p.robust_kernel == 0 and p.robust_scale == 0.0
    assert _lib.ROBUST_KERNELS == {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3, "gm": 3, "tukey": 4}
    for name, code in _lib.ROBUST_KERNELS.items():
        assert gicp.default_params(3, robust_kernel=name, robust_scale=0.5).robust_kernel == code
        assert gicp.default_params(3, robust_kernel=code).robust_kernel == code
    p = gicp.default_params(3, robust_kernel="cauchy", robust_scale=0.01)
    assert (p.robust_kernel, p.robust_scale) == (2, 0.01)
    assert gicp.default_params(3, robust_kernel=None).robust_kernel == 0
    assert _lib.load().gicp_version() >= 101


def test_params_struct_matches_the_header_layout():
    """The two fields are appended with explicit padding: offsets by the C rules for
    {..., double mse_relative_epsilon; int32 robust_kernel; int32 pad_robust; double robust_scale}."""
    P = _lib.Params
    end = P.mse_relative_epsilon.offset + 8
    assert (P.robust_kernel.offset, P.pad_robust.offset, P.robust_scale.offset) == (end, end + 4, end + 8)
    assert C.sizeof(P) == end + 16


def test_refusals_before_the_device(monkeypatch):
    """mode='faithful' replays the reference, which has no such weights; an unknown name is refused.  Both
    before any engine is touched (the fake device's contexts are never created)."""
    fake = fake_device.install(monkeypatch)
    src, tgt, _ = S.segment_scene_2d(400)
    kw = dict(max_distance_correspondence=20.0, max_distance_nearest_neighbors=25.0, verbose=False)
    with pytest.raises(ValueError, match="faithful"):
        gicp.gicp(src, tgt, robust_kernel="huber", robust_scale=1.0, mode="faithful", **kw)
    with pytest.raises(ValueError, match="robust_kernel"):
        gicp.gicp(src, tgt, robust_kernel="welsch", robust_scale=1.0, **kw)
    with pytest.raises(ValueError, match="robust_kernel"):
        gicp.default_params(3, robust_kernel="welsch")
    for scale in (None, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="robust_scale"):
            gicp.gicp(src, tgt, robust_kernel="cauchy", robust_scale=scale, **kw)
    assert not fake._ctx


def test_odometry_takes_the_kernel_by_name(monkeypatch):
    fake_device.install(monkeypatch)
    from gicp.odometry import Odometry
    odo = Odometry(3, robust_kernel="cauchy", robust_scale=0.01, max_iterations=7)
    assert (odo.params.robust_kernel, odo.params.robust_scale, odo.params.max_iterations) == (2, 0.01, 7)
    with pytest.raises(ValueError, match="robust_kernel"):
        Odometry(3, robust_kernel="welsch", robust_scale=0.01)


@pytest.mark.parametrize("c", [0.01, 0.05, 3.0])
def test_weight_functions_at_zero_and_at_the_scale(c):
    c2 = c * c
    at_c2 = {"none": 1.0, "huber": 1.0, "cauchy": 0.5, "geman_mcclure": 0.25, "tukey": 0.0}
    for kind, v in at_c2.items():
        assert R.KINDS[kind] == _lib.ROBUST_KERNELS[kind]          # the reference's codes are the library's
        assert R.weight(kind, 0.0, c) == 1.0
        assert R.weight(kind, -1e-30, c) == 1.0                    # e is clamped at 0
        np.testing.assert_allclose(R.weight(kind, c2, c), v, rtol=0, atol=4e-16)
        assert R.weight(R.KINDS[kind], c2, c) == R.weight(kind, c2, c)
        # continuity at e = c^2 (Huber's and Tukey's branch point): |w'| <= 2 / c^2 for every kernel
        for e in (c2 * (1 - 1e-9), c2 * (1 + 1e-9)):
            assert abs(R.weight(kind, e, c) - v) <= 4e-9
    e = np.linspace(0.0, 9 * c2, 1001)
    for kind in R.ROBUST:
        w = R.weight(kind, e, c)
        assert np.all((w >= 0) & (w <= 1)) and np.all(np.diff(w) <= 0)
    assert np.all(R.weight("tukey", e[e >= c2], c) == 0.0)
    np.testing.assert_allclose(R.weight("huber", 4 * c2, c), 0.5, rtol=1e-15)


def test_pass_reference_scales_the_statistics():
    """pass_reference's statistics are O.stats of w W: equal to the plain ones under kernel 0, and the count
    slot never depends on the kernel."""
    rng = np.random.default_rng(2)
    tgt = rng.uniform(0, 2, (300, 3))
    src = tgt[:120] + rng.normal(0, 0.02, (120, 3))
    C_s, _ = O.covariances(src, 1.0)
    C_t, cnt_t = O.covariances(tgt, 1.0)
    T = np.eye(4)
    idx0, _, W0, st0, e0, w0 = R.pass_reference(src, tgt, T, 0.5, C_s, C_t, kind="none")
    idx1, _, W1, st1, e1, w1 = R.pass_reference(src, tgt, T, 0.5, C_s, C_t, kind="cauchy", c=float(np.sqrt(np.median(e0))))
    assert np.array_equal(idx0, idx1) and np.array_equal(e0, e1) and np.all(w0[idx0 >= 0] == 1.0)
    assert st1[-1] == st0[-1] == np.sum(idx0 >= 0)
    np.testing.assert_allclose(W1, W0 * w1[:, None, None], rtol=0, atol=0)
    np.testing.assert_allclose(st1[-2], np.sum(w1 * e1), rtol=1e-12)   # c0 = sum w r^T W r
    assert 0.0 < st1[-2] < st0[-2]


# ---------------------------------------------------------------------------------- the outlier scene
@pytest.fixture(scope="module")
def outlier_runs():
    """The reference loop on the outlier scene, every kernel under both covariance models, and again on a
    target perturbed by 1e-9 relative noise: {(model, kind): (T, T_perturbed)}, plus the true pose."""
    src, tgt, T_gt = R.outlier_scene()
    tgt_p = tgt * (1.0 + 1e-9 * np.random.default_rng(0).standard_normal(tgt.shape))
    C_s, _ = O.covariances(src, R.OUTLIER_DN)
    out = {}
    for cloud, slot in ((tgt, 0), (tgt_p, 1)):
        C_t, cnt_t = O.covariances(cloud, R.OUTLIER_DN)
        for model in R.OUTLIER_SCALE:
            for kind in ("none",) + R.ROBUST:
                T, _ = R.loop(src, cloud, kind, R.outlier_scale(kind, model), R.OUTLIER_DC, R.OUTLIER_DN,
                              R.OUTLIER_ITERS, model, clouds=(C_s, C_t, cnt_t))
                out.setdefault((model, kind), [None, None])[slot] = T
    return out, T_gt


@pytest.mark.parametrize("model", sorted(R.OUTLIER_SCALE))
def test_outlier_scene_reference_loop(outlier_runs, model):
    """A fifth of the target moved by 18 cm: Cauchy and Geman-McClure end with at most a quarter of the plain
    loop's translation error (measured: profiles/robust/README.md)."""
    runs, T_gt = outlier_runs
    err = {k: S.translation_error(runs[(model, k)][0], T_gt) for k in ("none",) + R.ROBUST}
    print(model, {k: f"{1e3 * v:.2f} mm" for k, v in err.items()})
    assert err["none"] > 0.02
    for kind in ("cauchy", "geman_mcclure"):
        assert err[kind] <= err["none"] / 4, (kind, err)


@pytest.mark.parametrize("model", sorted(R.OUTLIER_SCALE))
@pytest.mark.parametrize("kind", R.ROBUST)
def test_outlier_scene_endpoint_is_well_conditioned(outlier_runs, model, kind):
    """What the 1e-6 end-to-end bound of test_gpu_robust.py rests on: 1e-9 relative noise on the target
    moves the reference loop's own endpoint by less than 1e-7 (rad, m), the redescending kernels included."""
    runs, _ = outlier_runs
    T, Tp = runs[(model, kind)]
    dr, dt = S.rotation_angle_error(T, Tp), S.translation_error(T, Tp)
    print(model, kind, f"{dr:.2e} rad {dt:.2e} m")
    assert dr < 1e-7 and dt < 1e-7
