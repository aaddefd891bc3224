"""GPU parity of the robust kernels (include/gicp_hip.h GICP_ROBUST_*) against the NumPy
reference tests/robust_ref.py: one pass (all kernels x covariance models, 3-D and 2-D, the smallest shapes),
what must not change (correspondences, distances, count, sum of squared distances), the top weights, the
device loop against the host loop and against three shards, the drop-in end to end on the outlier scene,
scan-to-map odometry, and the refusals."""
import numpy as np
import pytest

import edge_ref as E
import gpu_helpers as H
import robust_ref as R
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gicp import synthetic as S  # noqa: E402

MODELS = {"plane_to_plane": 0, "point_to_point": 1, "point_to_plane": 2}


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


def _pose3():
    """The 1.5 degree pose of test_gpu_extensions._pose()."""
    T = np.eye(4)
    T[:3, :3] = S.axis_angle([1.0, -2.0, 0.5], np.deg2rad(1.5))
    T[:3, 3] = [0.05, -0.02, 0.01]
    return T


def _scene(eng, src, tgt, base, T):
    """The clouds, their covariances as the engine computes them (the covariance tests check those), and the pose."""
    p = gicp.default_params(src.shape[1], **base)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    return dict(src=src, tgt=tgt, base=base, T=T, C_s=eng.covariances("source"), C_t=eng.covariances("target"),
                cnt_t=eng.neighbor_counts("target"))


@pytest.fixture(scope="module")
def scene3d(eng):
    src, tgt, _ = S.scene_pair_3d(20000)
    return _scene(eng, src, tgt, H.P3, _pose3())


@pytest.fixture(scope="module")
def scene2d(eng):
    src, tgt, _ = S.segment_scene_2d(4000)
    return _scene(eng, src, tgt, H.P2, H.ladder_pose(src))


def _params(sc, model, **kw):
    return gicp.default_params(sc["src"].shape[1], cov_model=MODELS[model], **sc["base"], **kw)


def _median_scale(e, idx):
    ok = idx >= 0
    return float(np.sqrt(np.median(e[ok]))) if ok.any() and np.median(e[ok]) > 0 else 1.0


def check_robust_pass(eng, sc, model, kind, c=None, populated=True):
    """One pass with the kernel against the reference, and against the same pass with kernel 0 for what the
    kernel must leave alone.  c = None: the median whitened residual of the accepted pairs."""
    src, tgt, T = sc["src"], sc["tgt"], sc["T"]
    d_c = sc["base"]["max_distance_correspondence"]
    p0 = _params(sc, model)
    eng.set_target(tgt, p0)
    eng.set_source(src, p0)
    st0, dbg0 = eng.iterate(T, debug=True)
    sum0 = eng.pass_info()["sum_sq"]
    idx, _, W, _ = E.pass_reference(src, tgt, T, d_c, sc["C_s"], sc["C_t"], model, sc["cnt_t"])
    if c is None:
        c = _median_scale(R.reweight(src, tgt, idx, W, T, "none", 1.0)[1], idx)
    q, e, w, Ww = R.reweight(src, tgt, idx, W, T, kind, c)
    ref = O.stats(src, q, Ww, idx, T)
    ok = idx >= 0
    inside = float(np.mean(e[ok] < c * c)) if ok.any() else 0.0
    print(f"{model} {kind} n={len(src)}: c = {c:.4g}, {inside:.3f} of {int(ok.sum())} pairs inside, "
          f"mean w {np.mean(w[ok]) if ok.any() else 0:.3f}")
    if populated:
        assert 0.1 <= inside <= 0.9, inside
    eng.set_source(src, _params(sc, model, robust_kernel=kind, robust_scale=c))
    st, dbg = eng.iterate(T, debug=True)
    info = eng.pass_info()
    assert np.array_equal(dbg["index"], idx) and np.array_equal(dbg["index"], dbg0["index"])
    assert np.array_equal(dbg["distance"], dbg0["distance"])
    assert st[-1] == st0[-1] == ok.sum()
    assert info["sum_sq"] == sum0, (info["sum_sq"], sum0)                       # bit for bit
    np.testing.assert_allclose(dbg["weight"], Ww, rtol=1e-9, atol=1e-15 if model == "plane_to_plane" else 1e-12)
    np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * max(np.max(np.abs(ref)), 1e-300))
    return c, st, idx, Ww


# 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("kind", R.ROBUST)
def test_pass_3d_vs_reference(eng, scene3d, model, kind):
    check_robust_pass(eng, scene3d, model, kind)


@pytest.mark.parametrize("kind", R.ROBUST)
def test_pass_2d_vs_reference(eng, scene2d, kind):
    check_robust_pass(eng, scene2d, "plane_to_plane", kind)


# 2 ---------------------------------------------------------------------------------------------------------
def _patch(eng, n_src):
    src, tgt = E.dense_patch(3, n_src, 200)
    return _scene(eng, src, tgt, H.P3, H.ladder_pose(src))


@pytest.mark.parametrize("n_src", [1, 65])
@pytest.mark.parametrize("kind", R.ROBUST)
def test_pass_smallest_shapes(eng, n_src, kind):
    """One point, and one full wave plus one lane, against 200 targets: every covariance model.  (With one
    point, c is its own whitened residual: the branch point of Huber and Tukey, where both are continuous.)"""
    sc = _patch(eng, n_src)
    for model in sorted(MODELS):
        check_robust_pass(eng, sc, model, kind, populated=n_src > 1)


def test_tukey_with_every_weight_zero(eng):
    """c far below every residual: the correspondences stand, every statistic but the count is zero, the pass
    and the loop succeed, and the loop leaves the pose where it started."""
    sc = _patch(eng, 65)
    c, st, idx, Ww = check_robust_pass(eng, sc, "plane_to_plane", "tukey", c=1e-12, populated=False)
    assert np.all(Ww == 0) and np.sum(idx >= 0) == 65
    assert np.all(st[:-1] == 0) and st[-1] == 65
    _, dbg = eng.iterate(sc["T"], debug=True)
    assert np.all(dbg["index"] >= 0) and np.all(dbg["weight"] == 0)
    p = _params(sc, "plane_to_plane", robust_kernel="tukey", robust_scale=c, max_iterations=5)
    T, res = eng.align(sc["T"], p)
    assert np.array_equal(T, sc["T"]) and res["final_loss"] == 0.0 and res["correspondences"] == 65
    T, res = eng.align(sc["T"], _params(sc, "plane_to_plane", max_iterations=5))   # and the engine goes on
    assert np.all(np.isfinite(T)) and not np.array_equal(T, sc["T"])


# 3 ---------------------------------------------------------------------------------------------------------
def test_kernel_none_ignores_the_scale(eng, scene3d):
    sc = scene3d
    out = []
    for kw in (dict(), dict(robust_kernel=0, robust_scale=123.0)):
        p = _params(sc, "plane_to_plane", fixed_iterations=1, max_iterations=10, **kw)
        eng.set_target(sc["tgt"], p)
        eng.set_source(sc["src"], p)
        st = eng.iterate(sc["T"])
        T, res = eng.align(None, p)
        out.append((st, T, res["final_loss"]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# 4 ---------------------------------------------------------------------------------------------------------
def test_top_weights_under_cauchy(eng, scene3d):
    """gicp_top_weights ranks det(w W): the argsort of the reference's (as test_top_weights_vs_argsort)."""
    sc = scene3d
    c, _, idx, Ww = check_robust_pass(eng, sc, "plane_to_plane", "cauchy")
    det = np.linalg.det(Ww)
    ref = np.argsort(det, kind="stable")[-5:]
    _, si, ti, dt = eng.iterate_top(sc["T"], 5)
    np.testing.assert_allclose(dt, det[ref], rtol=1e-9)
    np.testing.assert_allclose(det[si], det[ref], rtol=1e-9)
    if len(np.unique(np.round(det[ref] / det[ref].max(), 6))) == 5:
        assert np.array_equal(si, ref)
    assert np.array_equal(ti, idx[si])


# 5 ---------------------------------------------------------------------------------------------------------
def test_device_loop_matches_host_loop_and_three_shards(eng, scene3d):
    """gicp_align under Huber == the host loop of gicp_iterate + gicp.solve_pose over the same passes (atol
    1e-10, as test_pcl_criteria_device_matches_host_loop), and == the loop with the source dealt to three
    shards on three engines of this GPU whose statistics meet in a host hook (atol 1e-9, the bound of
    test_two_ranks_one_gpu_1m_30_iterations; the shards' sums, rtol 1e-12 as test_sharded_statistics_sum_to_full)."""
    sc = scene3d
    src, tgt = sc["src"], sc["tgt"]
    idx, _, W, _ = E.pass_reference(src, tgt, np.eye(4), 0.5, sc["C_s"], sc["C_t"])
    c = _median_scale(R.reweight(src, tgt, idx, W, np.eye(4), "none", 1.0)[1], idx)
    p = _params(sc, "plane_to_plane", robust_kernel="huber", robust_scale=c, fixed_iterations=1, max_iterations=15)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    Tdev, res = eng.align(None, p)
    assert res["iterations"] == 15
    T = np.eye(4)
    for _ in range(15):
        T, loss = gicp.solve_pose(eng.iterate(T), T)
    print(f"device vs host loop: {np.max(np.abs(Tdev - T)):.2e}")
    np.testing.assert_allclose(Tdev, T, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res["final_loss"], loss, rtol=1e-9)
    full = eng.iterate(np.eye(4))
    engines = [gicp.Engine(0) for _ in range(3)]
    try:
        parts = []
        for r, e in enumerate(engines):
            e.set_target(tgt, p)
            e.set_source(src, p, shard=r, nshards=3)
            parts.append(e.iterate(np.eye(4)))
        np.testing.assert_allclose(np.sum(parts, axis=0), full, rtol=1e-12, atol=1e-12 * np.max(np.abs(full)))
        xchg = gicp._ThreadSum(3, timeout=60.0)
        for r, e in enumerate(engines):
            e.set_allreduce(lambda buf, r=r: xchg(r, buf), nranks=3, rank=r)

        def run(r, e):
            try:
                return e.align(None, p)
            except BaseException:
                xchg.abort()
                raise

        outs = gicp._run_ranks(engines, run)
    finally:
        for e in engines:
            e.close()
    assert all(np.array_equal(o[0], outs[0][0]) for o in outs)
    print(f"three shards vs one: {np.max(np.abs(outs[0][0] - Tdev)):.2e}")
    np.testing.assert_allclose(outs[0][0], Tdev, rtol=0, atol=1e-9)
    assert outs[0][1]["correspondences"] == res["correspondences"]


# 6 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def outlier():
    """The outlier scene with its oracle covariances, and a cache of the runs on it."""
    src, tgt, T_gt = R.outlier_scene()
    C_s, _ = O.covariances(src, R.OUTLIER_DN)
    C_t, cnt_t = O.covariances(tgt, R.OUTLIER_DN)
    return dict(src=src, tgt=tgt, T_gt=T_gt, clouds=(C_s, C_t, cnt_t), gpu={})


def _gpu_run(sc, model, kind):
    key = (model, kind)
    if key not in sc["gpu"]:
        kw = dict() if kind == "none" else dict(robust_kernel=kind, robust_scale=R.outlier_scale(kind, model))
        sc["gpu"][key] = gicp.gicp(sc["src"], sc["tgt"], max_iterations=R.OUTLIER_ITERS, tolerance=0,
                                   max_distance_correspondence=R.OUTLIER_DC, max_distance_nearest_neighbors=R.OUTLIER_DN,
                                   method=model, full_output=False, verbose=False, **kw)[:2]
    return sc["gpu"][key]


@pytest.mark.parametrize("model", sorted(R.OUTLIER_SCALE))
@pytest.mark.parametrize("kind", R.ROBUST)
def test_gicp_end_to_end_on_the_outlier_scene(outlier, model, kind):
    """The drop-in with a kernel == the reference's IRLS loop, 25 iterations each, to 1e-6 rad / 1e-6 m (the
    bound of test_gicp_methods_end_to_end_vs_oracle; test_robust_cpu.py shows that 1e-9 noise moves the
    reference's endpoint by < 1e-7 for every kernel, so none needs the teacher-forced comparison).  And the
    point of it: Cauchy and Geman-McClure end with at most a quarter of the plain loop's translation error."""
    sc = outlier
    T, all_T = _gpu_run(sc, model, kind)
    assert len(all_T) == R.OUTLIER_ITERS + 1
    To, _ = R.loop(sc["src"], sc["tgt"], kind, R.outlier_scale(kind, model), R.OUTLIER_DC, R.OUTLIER_DN,
                   R.OUTLIER_ITERS, model, clouds=sc["clouds"])
    a, t = S.rotation_angle_error(T, To), S.translation_error(T, To)
    plain = S.translation_error(_gpu_run(sc, model, "none")[0], sc["T_gt"])
    err = S.translation_error(T, sc["T_gt"])
    print(f"{model} {kind}: GPU vs reference {a:.2e} rad {t:.2e} m; error {1e3 * err:.2f} mm, plain {1e3 * plain:.2f} mm")
    assert a < 1e-6 and t < 1e-6, (a, t)
    if kind in ("cauchy", "geman_mcclure"):
        assert err <= plain / 4, (err, plain)


@pytest.mark.parametrize("inner", ["cg", "newton"])
def test_gicp_2d_fast_mode_either_inner_solver(scene2d, inner):
    """mode='fast' in 2-D: the kernel reaches the host loop (inner='cg') and the device loop.  The engine the
    call used gives the reference's Cauchy statistics at the identity, and the call's first update is the
    inner solver's answer to exactly those."""
    sc = scene2d
    src, tgt, I = sc["src"], sc["tgt"], np.eye(3)
    idx, _, W, _ = E.pass_reference(src, tgt, I, H.P2["max_distance_correspondence"], sc["C_s"], sc["C_t"])
    c = _median_scale(R.reweight(src, tgt, idx, W, I, "none", 1.0)[1], idx)
    q, _, _, Ww = R.reweight(src, tgt, idx, W, I, "cauchy", c)
    ref = O.stats(src, q, Ww, idx, I)
    T, all_T, *_ = gicp.gicp(src, tgt, max_iterations=2, tolerance=0, mode="fast", inner=inner, full_output=False,
                             verbose=False, robust_kernel="cauchy", robust_scale=c, **H.P2)
    assert len(all_T) == 3 and np.all(np.isfinite(T))
    st = gicp._engine(0).iterate(I)
    np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * np.max(np.abs(ref)))
    if inner == "cg":
        x, _ = gicp._cg_inner(st, np.zeros(3), I)
        assert np.array_equal(all_T[1], gicp._offset_to_T(x))
    else:   # device solve against host solve: the rotation to 1e-10, as in 3-D; a rotation that far off moves a
        # point at the cloud's radius (coordinates to 1000 px here) by radius x 1e-10, and with it the translation
        T1 = gicp.solve_pose(st, I)[0]
        print(f"device vs host solve: R {np.max(np.abs(all_T[1][:2, :2] - T1[:2, :2])):.2e}, "
              f"t {np.max(np.abs(all_T[1][:2, 2] - T1[:2, 2])):.2e} px")
        np.testing.assert_allclose(all_T[1][:2, :2], T1[:2, :2], rtol=0, atol=1e-10)
        np.testing.assert_allclose(all_T[1][:2, 2], T1[:2, 2], rtol=0, atol=1e-10 * np.max(np.linalg.norm(src, axis=1)))


# 7 ---------------------------------------------------------------------------------------------------------
def test_scan_to_map_odometry_with_cauchy():
    """Scan-to-map with robust_kernel='cauchy' through Odometry's **kw: every frame within the per-frame bounds
    of tests/test_gpu_map.py test 9 (2e-3 rad, 0.1 m) of the generator's motion."""
    from gicp.odometry import Odometry
    frames = list(S.lidar_stream(4, beams=16, azimuths=600, step=0.15, along_path=True))
    odo = Odometry(3, init="identity", map_voxel_size=0.4, map_range=30.0, robust_kernel="cauchy", robust_scale=0.01,
                   max_iterations=40, tolerance=1e-10, **H.P3)
    try:
        assert odo.params.robust_kernel == 2
        for k, (scan, pose) in enumerate(frames):
            T, res = odo.step(scan)
            if T is None:
                continue
            Ttrue = np.linalg.inv(pose) @ frames[k - 1][1]
            a, t = S.rotation_angle_error(T, Ttrue), S.translation_error(T, Ttrue)
            print(f"frame {k}: {a:.3e} rad {t:.3e} m, {res['iterations']} iterations")
            assert a < 2e-3 and t < 0.1, (k, a, t)
        assert len(odo.poses) == len(frames)
    finally:
        odo.eng.close()


# 8 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(robust_kernel=7, robust_scale=1.0), dict(robust_kernel=-1, robust_scale=1.0),
                                 dict(robust_kernel=2, robust_scale=0.0), dict(robust_kernel=2, robust_scale=float("nan")),
                                 dict(robust_kernel=4, robust_scale=-1.0), dict(robust_kernel=1, robust_scale=float("inf"))])
def test_refusals(eng, bad):
    sc = _patch(eng, 65)
    good = _params(sc, "plane_to_plane", max_iterations=3)
    p = _params(sc, "plane_to_plane", max_iterations=3, **bad)
    with pytest.raises(ValueError, match="robust"):
        eng.set_source(sc["src"], p)
    with pytest.raises(ValueError, match="robust"):
        eng.set_target(sc["tgt"], p)
    eng.set_target(sc["tgt"], good)
    eng.set_source(sc["src"], good)
    with pytest.raises(ValueError, match="robust"):
        eng.align(None, p)
    T, res = eng.align(None, good)           # the engine works afterwards, with the parameters it had
    assert np.all(np.isfinite(T)) and res["iterations"] == 3
    st = eng.iterate(np.eye(4))
    assert st[-1] == 65
