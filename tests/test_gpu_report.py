"""GPU tests of the registration report (gicp_evaluate, include/gicp_hip.h "registration report"):
H and b against the NumPy restatement tests/report_ref.py on the oracle's weights, the overlap table and the
quantiles against the engine's own per-point arrays, the shapes at which the kernels of csrc/gicp_eval.hip can go
wrong (a lone lane, a wave edge, a workgroup edge, several workgroups, the 65 536 and 262 144 rows above which
k_eval_sums and k_sel_hist take their second paths; every value equal; nothing accepted; ties across a rank, at
257 rows and at 262 401), what the call leaves behind, a degenerate scene, the refusals, and Odometry(report=...)."""
import numpy as np
import pytest

import edge_ref as E
import gpu_helpers as H
import report_ref as RR
import robust_ref as R

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from oracle import gicp_oracle as O  # noqa: E402

P3, P2 = H.P3, H.P2
MODELS = {"plane_to_plane": 0, "point_to_point": 1, "point_to_plane": 2}
QS = (0.0, 0.25, 0.5, 0.9, 1.0)


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


def _pose3():
    """2 degrees and 0.1 m."""
    T = np.eye(4)
    T[:3, :3] = S.axis_angle([1.0, -2.0, 0.5], np.deg2rad(2.0))
    T[:3, 3] = [0.06, -0.05, 0.06]
    return T


def _scene(eng, src, tgt, base, T):
    p = gicp.default_params(src.shape[1], **base)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    return dict(src=src, tgt=tgt, base=base, T=T, C_s=eng.covariances("source"), C_t=eng.covariances("target"),
                cnt_t=eng.neighbor_counts("target"))


@pytest.fixture(scope="module")
def scene3d(eng):
    src, tgt, _ = S.scene_pair_3d(3000)
    return _scene(eng, src, tgt, P3, _pose3())


@pytest.fixture(scope="module")
def scene2d(eng):
    src, tgt, _ = S.segment_scene_2d(2000)
    return _scene(eng, src, tgt, P2, H.ladder_pose(src))


def _set(eng, sc, **kw):
    p = gicp.default_params(sc["src"].shape[1], **sc["base"], **kw)
    eng.set_target(sc["tgt"], p)
    eng.set_source(sc["src"], p)
    return p


def _thresholds(sc):
    dc = sc["base"]["max_distance_correspondence"]
    return (0.0, dc / 4, dc / 2, dc)


def check_against_debug(eng, src, tgt, T, thr, qs, what=""):
    """One evaluate against the engine's own pass at the same pose: the scalars and H bit for bit, the overlap
    table against the per-point arrays (counts exact, sums within n 2^-52 sum: the terms are non-negative, so
    every summation order stays inside that), dist_q bit for bit, white_q within 1e-12 max s."""
    rep = eng.evaluate(T, thresholds=thr, quantiles=qs)
    st, dbg = eng.iterate(T, debug=True)
    info = eng.pass_info()
    idx, dist, W = dbg["index"], dbg["distance"], dbg["weight"]
    ok = idx >= 0
    n = int(ok.sum())
    assert rep["n_source"] == len(src) and rep["n_matched"] == st[-1] == n, what
    assert rep["loss"] == st[-2] and rep["sum_sq"] == info["sum_sq"], what
    Hm, b = gicp.information(st, T)
    assert np.array_equal(rep["H"], Hm) and np.array_equal(rep["b"], b), what
    nw = Hm.shape[0] - src.shape[1]
    for key, A in (("eig", Hm), ("eig_rot", Hm[:nw, :nw]), ("eig_trans", Hm[nw:, nw:])):
        assert np.array_equal(rep[key], gicp.sym_eig(A)[0]), (what, key)
    cnt, ssq = RR.overlap_ref(dist, idx, thr)
    assert np.array_equal(rep["inliers"], cnt), (what, rep["inliers"], cnt)
    err = np.abs(rep["inlier_sum_sq"] - ssq)
    print(f"{what}: n = {n} of {len(src)}, inliers {cnt}, |sum - ref| / sum = {err / np.maximum(ssq, 1e-300)}")
    assert np.all(err <= max(n, 1) * 2.0 ** -52 * ssq), (what, err, ssq)
    assert np.array_equal(rep["fitness"], cnt / len(src))
    s = RR.whitened(src, RR.matches(tgt, idx), W, idx, T)
    for pi in qs:
        if n == 0:
            assert np.isnan(rep["dist_q"][pi]) and np.isnan(rep["white_q"][pi]), what
            continue
        assert rep["dist_q"][pi] == np.quantile(dist[ok], pi, method="lower"), (what, pi)
        ws = np.quantile(s, pi, method="lower")
        assert abs(rep["white_q"][pi] - ws) <= 1e-12 * s.max(), (what, pi, rep["white_q"][pi], ws)
    return rep, st, dbg


# 1 --------------------------------------------------------------------------------------------------------
def _check_information(eng, sc, model, kind):
    src, tgt, T = sc["src"], sc["tgt"], sc["T"]
    d_c = sc["base"]["max_distance_correspondence"]
    idx, _, W, _ = E.pass_reference(src, tgt, T, d_c, sc["C_s"], sc["C_t"], model, sc["cnt_t"])
    kw = dict(cov_model=MODELS[model])
    if kind != "none":
        e = R.reweight(src, tgt, idx, W, T, "none", 1.0)[1]
        c = float(np.sqrt(np.median(e[idx >= 0])))
        W = R.reweight(src, tgt, idx, W, T, kind, c)[3]
        kw.update(robust_kernel=kind, robust_scale=c)
    _set(eng, sc, **kw)
    rep = eng.evaluate(T)
    Hr, br = RR.information_ref(src, RR.matches(tgt, idx), W, idx, T)
    n = int(np.sum(idx >= 0))
    print(f"{model} {kind} d={src.shape[1]}: {n} of {len(src)} accepted; max|H - ref| / max|ref| = "
          f"{np.max(np.abs(rep['H'] - Hr)) / np.max(np.abs(Hr)):.2e}, b: {np.max(np.abs(rep['b'] - br)) / np.max(np.abs(br)):.2e}")
    assert 0.1 * len(src) < n < 0.9 * len(src) or src.shape[1] == 2
    np.testing.assert_allclose(rep["H"], Hr, rtol=1e-9, atol=1e-9 * np.max(np.abs(Hr)))
    np.testing.assert_allclose(rep["b"], br, rtol=1e-9, atol=1e-9 * np.max(np.abs(br)))
    st = eng.iterate(T)
    Hm, b = gicp.information(st, T)
    assert np.array_equal(rep["H"], Hm) and np.array_equal(rep["b"], b)
    assert rep["n_matched"] == st[-1] == n and rep["loss"] == st[-2]
    assert rep["sum_sq"] == eng.pass_info()["sum_sq"]


@pytest.mark.parametrize("kind", ["none", "cauchy"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_information_3d(eng, scene3d, model, kind):
    _check_information(eng, scene3d, model, kind)


@pytest.mark.parametrize("kind", ["none", "cauchy"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_information_2d(eng, scene2d, model, kind):
    _check_information(eng, scene2d, model, kind)


# 2, 3 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_overlap_table_and_quantiles(eng, scene3d, scene2d, dim):
    sc = scene3d if dim == 3 else scene2d
    _set(eng, sc)
    thr = _thresholds(sc)
    rep, _, dbg = check_against_debug(eng, sc["src"], sc["tgt"], sc["T"], thr, QS, f"scene {dim}-D")
    ok = dbg["index"] >= 0
    if dim == 3:
        assert 300 < ok.sum() < 2700                         # the accepted and the rejected set are both large
    assert rep["inliers"][-1] == ok.sum() and rep["inliers"][0] <= rep["inliers"][1] <= rep["inliers"][2]
    again = eng.evaluate(sc["T"], thresholds=thr, quantiles=QS)
    fresh = gicp.Engine(0)
    try:
        _set(fresh, sc)
        other = fresh.evaluate(sc["T"], thresholds=thr, quantiles=QS)
    finally:
        fresh.close()
    for r in (again, other):                                 # the same bits on a second call and a fresh engine
        assert np.array_equal(r["inlier_sum_sq"], rep["inlier_sum_sq"]) and np.array_equal(r["inliers"], rep["inliers"])
        assert r["dist_q"] == rep["dist_q"] and r["white_q"] == rep["white_q"]
        assert np.array_equal(r["H"], rep["H"]) and np.array_equal(r["eigvec"], rep["eigvec"])


def test_quantiles_under_a_robust_kernel_and_eight_ranks(eng, scene3d):
    """W~ = w W in white_q, and the full width of the spec: 8 thresholds, 8 probabilities."""
    sc = scene3d
    _set(eng, sc, robust_kernel="cauchy", robust_scale=0.5, cov_model=MODELS["point_to_plane"])
    dc = sc["base"]["max_distance_correspondence"]
    thr = tuple(dc * k / 8 for k in range(1, 9))
    qs = (0.0, 0.01, 0.3, 0.5, 0.77, 0.9, 0.999, 1.0)
    check_against_debug(eng, sc["src"], sc["tgt"], sc["T"], thr, qs, "cauchy, point to plane, 8 + 8")


# 4 --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prefix_cloud():
    src, tgt, _ = S.scene_pair_3d(4097, 3000)
    return src, tgt


@pytest.fixture(scope="module")
def long_prefix_cloud():
    """262 401 source rows = 1025 workgroups of k_eval_values and one row: above both thresholds of the report's
    second code paths.  k_eval_sums gives each of its 256 threads a run of ceil(workgroups / 256)
    partials, longer than one from 65 537 rows on; k_sel_hist has at most kSelGridMax = 1024 workgroups and takes
    the keys beyond 262 144 by its grid stride."""
    src, tgt, _ = S.scene_pair_3d(262401, 3000)
    return src, tgt


def _block_edge_probabilities(m):
    """8 probabilities for m accepted rows: 0, 1, and six whose rank floor(pi (m - 1)) is the last row of a 256-row
    block of the sorted values or the first row of the next (asserted): the first block's end, the middle's, the
    last whole one's."""
    assert m > 1024
    ends = (255, 256 * (m // 512) - 1, 256 * ((m - 2) // 256) - 1)
    ranks = [r for e in ends for r in (e, e + 1)]
    qs = (0.0,) + tuple((r + 0.5) / (m - 1) for r in ranks) + (1.0,)
    assert [int(np.floor(pi * (m - 1))) for pi in qs[1:-1]] == ranks and ranks[-1] < m - 1
    assert sorted(set(ranks)) == ranks and all(r % 256 in (0, 255) for r in ranks)
    return qs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 65536, 65537, 262144, 262145, 262401])
def test_source_sizes(eng, prefix_cloud, long_prefix_cloud, n):
    src, tgt = prefix_cloud if n <= 4097 else long_prefix_cloud
    src = np.ascontiguousarray(src[:n])
    p = gicp.default_params(3, max_distance_correspondence=1.0, max_distance_nearest_neighbors=1.0)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    thr, qs = (0.0, 0.25, 0.5, 1.0), QS
    if n > 4097:                                             # the full width of the spec: 8 thresholds, 8 probabilities
        thr = (0.0, 0.05, 0.125, 0.25, 0.5, 0.75, 0.9, 1.0)
        qs = _block_edge_probabilities(int(eng.iterate(_pose3())[-1]))
        assert len(qs) == 8 and len(set(qs)) == 8
    rep, _, _ = check_against_debug(eng, src, tgt, _pose3(), thr, qs, f"prefix {n}")
    if n >= 63:                                              # (these clouds are sparse: about a quarter is rejected)
        assert 0 < rep["n_matched"] < n


def test_every_value_equal(eng):
    tgt = S.scene_pair_3d(3000)[1]
    p = gicp.default_params(3, **P3)
    eng.set_target(tgt, p)
    eng.set_source(tgt, p)
    rep, _, dbg = check_against_debug(eng, tgt, tgt, np.eye(4), (0.0, 0.25), QS, "source = target")
    assert np.array_equal(dbg["index"], np.arange(len(tgt))) and not dbg["distance"].any()
    assert list(rep["inliers"]) == [len(tgt), len(tgt)] and not rep["inlier_sum_sq"].any()
    assert all(v == 0.0 for v in rep["dist_q"].values()) and all(v == 0.0 for v in rep["white_q"].values())
    assert rep["loss"] == 0.0 and not rep["b"].any() and rep["eig"][0] > 0


def test_nothing_accepted(eng):
    pts = H.planar_lattice()
    p = gicp.default_params(3, **P3)
    eng.set_target(pts, p)
    eng.set_source(pts, p)
    T = np.eye(4)
    T[2, 3] = 10 * P3["max_distance_correspondence"]
    rep, _, dbg = check_against_debug(eng, pts, pts, T, (0.0, 0.5), QS, "10 d_c away")     # returns: GICP_OK
    assert np.all(dbg["index"] == -1)
    assert rep["n_matched"] == 0 and not rep["inliers"].any() and not rep["inlier_sum_sq"].any()
    assert all(np.isnan(v) for v in rep["dist_q"].values()) and all(np.isnan(v) for v in rep["white_q"].values())
    for key in ("H", "b", "eig", "eig_rot", "eig_trans"):
        assert not rep[key].any(), key
    assert rep["loss"] == 0.0 and rep["sum_sq"] == 0.0
    assert np.all(np.isnan(rep["inlier_rmse"])) and not rep["fitness"].any()


def test_ties_across_a_rank(eng):
    """A unit-lattice target; 128 sources offset by exactly 0.25 and 129 by exactly 0.375 along x from distinct
    lattice points: 257 values, so index floor(pi 256) crosses from the 0.25s to the 0.375s exactly at pi = 0.5."""
    g = np.stack(np.meshgrid(np.arange(7.0), np.arange(7.0), np.arange(7.0), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(8)
    tgt = g[rng.permutation(len(g))]
    src = tgt[rng.permutation(len(tgt))[:257]].copy()
    off = np.where(rng.permutation(257) < 128, 0.25, 0.375)
    src[:, 0] += off
    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.5,
                            cov_model=MODELS["point_to_point"])
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    below, above = np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)
    qs = (0.0, below, 0.5, above, 1.0)
    rep, _, dbg = check_against_debug(eng, src, tgt, np.eye(4), (0.25, 0.375), qs, "lattice ties")
    assert np.array_equal(dbg["distance"], off)
    want = {0.0: 0.25, below: 0.25, 0.5: 0.375, above: 0.375, 1.0: 0.375}
    assert rep["dist_q"] == want and rep["white_q"] == want             # W = I: s = dist, exactly
    assert list(rep["inliers"]) == [128, 257]
    assert list(rep["inlier_sum_sq"]) == [128 * 0.0625, 128 * 0.0625 + 129 * 0.140625]


def test_two_values_at_full_scale(eng):
    """test_ties_across_a_rank at 262 401 rows (1025 workgroups and one row: k_eval_sums' runs of 5 partials,
    k_sel_hist's grid stride) against a 65^3 lattice: every key of a class is the same 64 bits, so every round of
    the select takes the one-add-per-wave branch with counts above 2^16 in a bin, and k_sel_narrow's prefix sum
    runs over them.  131 201 rows at 0.25, 131 200 at 0.375: rank floor(0.5 (n - 1)) = 131 200 is the last 0.25.
    Every partial sum of the squares is a multiple of 2^-6 below 2^53: exact in any order."""
    g = np.stack(np.meshgrid(*(np.arange(65.0),) * 3, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(9)
    tgt = g[rng.permutation(len(g))]
    n, n1 = 262401, 131201
    n2 = n - n1
    src = tgt[rng.permutation(len(tgt))[:n]].copy()
    off = np.where(rng.permutation(n) < n1, 0.25, 0.375)
    src[:, 0] += off
    assert int(np.floor(0.5 * (n - 1))) == n1 - 1 and np.sum(off == 0.25) == n1
    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.5,
                            cov_model=MODELS["point_to_point"])
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    below, above = np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)
    first = (n1 + 0.5) / (n - 1)                             # the first 0.375
    qs = (0.0, below, 0.5, above, first, 1.0)
    rep, _, dbg = check_against_debug(eng, src, tgt, np.eye(4), (0.25, 0.375), qs, "lattice ties, 262 401 rows")
    assert np.array_equal(dbg["distance"], off)
    assert rep["n_matched"] == n
    want = {pi: 0.25 if int(np.floor(pi * (n - 1))) < n1 else 0.375 for pi in qs}     # the rank in fp64, as specified
    assert want[0.5] == 0.25 and want[first] == 0.375 and int(np.floor(first * (n - 1))) == n1
    assert rep["dist_q"] == want and rep["white_q"] == want             # W = I: s = dist, exactly
    assert list(rep["inliers"]) == [n1, n]
    assert list(rep["inlier_sum_sq"]) == [n1 * 0.0625, n1 * 0.0625 + n2 * 0.140625]
    again = eng.evaluate(np.eye(4), thresholds=(0.25, 0.375), quantiles=qs)
    assert np.array_equal(again["inlier_sum_sq"], rep["inlier_sum_sq"]) and np.array_equal(again["inliers"], rep["inliers"])
    assert again["dist_q"] == rep["dist_q"] and again["white_q"] == rep["white_q"]


# 5 --------------------------------------------------------------------------------------------------------
def test_evaluate_changes_no_later_result(scene3d):
    sc = scene3d
    prm = dict(max_iterations=12, tolerance=1e-9, **P3)
    other = gicp.default_params(3, max_distance_correspondence=0.2, max_distance_nearest_neighbors=1.0,
                                cov_model=MODELS["point_to_plane"], robust_kernel="huber", robust_scale=0.05)
    T = sc["T"]
    out = []
    for with_eval in (False, True):
        e = gicp.Engine(0)
        try:
            _set(e, sc)
            Ta, ra = e.align(None, gicp.default_params(3, **prm))
            if with_eval:
                rep = e.evaluate(Ta, other, thresholds=[0.1], quantiles=[0.5])
                assert rep["n_matched"] > 0
            st = e.iterate(T)
            if with_eval:
                e.evaluate(T, other, thresholds=[0.1], quantiles=[0.5])
            e.reset_cache()
            Tb, rb = e.align(None, gicp.default_params(3, **prm))
            out.append((Ta, st, Tb, rb["iterations"], rb["final_loss"]))
        finally:
            e.close()
    a, b = out
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])        # align -> evaluate(other d_c, model, kernel) -> iterate: the same statistics
    assert np.array_equal(a[2], b[2]) and a[3:] == b[3:]   # ... -> reset_cache -> align: the same again,
    assert np.array_equal(b[2], a[0])                       # which is a fresh engine's align


# 6 --------------------------------------------------------------------------------------------------------
def test_degenerate_plane(eng):
    """A 2000-point plane z = 0 with 2 mm noise against itself, point to plane: in-plane translation and the
    rotation about the normal are unconstrained.  The normals of such a plane, estimated over neighbourhoods
    0.3 m and more across, tilt by about noise / extent < 0.01 rad, and the three weakest directions leave
    span{v_x, v_y, w_z} by about that tilt: bound 0.1.  Their eigenvalues carry tilt^2 of the strong ones: bound
    1e-2 of the fourth."""
    rng = np.random.default_rng(12)
    pts = np.concatenate([rng.uniform(-5.0, 5.0, (2000, 2)), rng.normal(0.0, 0.002, (2000, 1))], axis=1)
    p = gicp.default_params(3, cov_model=MODELS["point_to_plane"], **P3)
    eng.set_target(pts, p)
    eng.set_source(pts, p)
    T = np.eye(4)
    rep, _, _ = check_against_debug(eng, pts, pts, T, (0.0, 0.5), (0.5,), "plane")
    C_t, cnt_t = eng.covariances("target"), eng.neighbor_counts("target")
    idx, _, W, _ = E.pass_reference(pts, pts, T, 0.5, eng.covariances("source"), C_t, "point_to_plane", cnt_t)
    Hr, _ = RR.information_ref(pts, RR.matches(pts, idx), W, idx, T)
    for key, vkey, A in (("eig", "eigvec", Hr), ("eig_rot", "vec_rot", Hr[:3, :3]), ("eig_trans", "vec_trans", Hr[3:, 3:])):
        w, V = np.linalg.eigh(A)
        lmax = w[-1]
        assert np.max(np.abs(rep[key] - w)) <= 1e-9 * lmax, (key, rep[key], w)
        gaps = np.diff(w)
        for k in range(len(w)):
            if (k == 0 or gaps[k - 1] > 1e-3 * lmax) and (k == len(w) - 1 or gaps[k] > 1e-3 * lmax):
                u, v = rep[vkey][:, k], V[:, k]
                assert min(np.max(np.abs(u - v)), np.max(np.abs(u + v))) <= 1e-6, (key, k)
    print("eig(H)", rep["eig"], "eig_rot", rep["eig_rot"], "eig_trans", rep["eig_trans"])
    assert rep["eig"][2] <= 1e-2 * rep["eig"][3]
    weak = rep["eigvec"][:, :3]
    outside = np.delete(weak, [2, 3, 4], axis=0)             # the components along w_x, w_y, v_z
    assert np.max(np.linalg.norm(outside, axis=0)) <= 0.1, np.linalg.norm(outside, axis=0)
    assert rep["eig_trans"][1] <= 1e-2 * rep["eig_trans"][2] and rep["eig_rot"][0] <= 1e-2 * rep["eig_rot"][1]


# 7 --------------------------------------------------------------------------------------------------------
def test_errors_carry_the_library_text(eng, scene3d):
    sc = scene3d
    p = _set(eng, sc)
    T = sc["T"]
    for kw, match in ((dict(thresholds=[0.500001]), "threshold must be finite and in"),
                      (dict(thresholds=[-1e-9]), "threshold must be finite and in"),
                      (dict(thresholds=[np.inf]), "threshold must be finite and in"),
                      (dict(thresholds=[np.nan]), "threshold must be finite and in"),
                      (dict(quantiles=[1.0000001]), "probability must be in"),
                      (dict(quantiles=[-0.1]), "probability must be in"),
                      (dict(quantiles=[np.nan]), "probability must be in"),
                      (dict(thresholds=[0.1] * 9), "n_thresholds must be 0..GICP_REPORT_MAX"),
                      (dict(quantiles=[0.5] * 9), "n_quantiles must be 0..GICP_REPORT_MAX")):
        with pytest.raises(ValueError, match=match):
            eng.evaluate(T, **kw)
    tight = gicp.default_params(3, max_distance_correspondence=0.2, max_distance_nearest_neighbors=1.0)
    with pytest.raises(ValueError, match="threshold must be finite and in"):
        eng.evaluate(T, tight, thresholds=[0.3])             # d_c of the pass, not the one in force
    assert eng.evaluate(T, thresholds=[0.3])["inliers"][0] > 0
    bad = T.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        eng.evaluate(bad)
    lib, ctx = _lib.load(), eng._ctx
    assert lib.gicp_evaluate(ctx, None, None, None, None) == _lib.GICP_E_INVALID
    assert b"out must not be NULL" in lib.gicp_last_error(ctx)
    neg = _lib.ReportSpec()
    neg.n_thresholds = -1
    assert lib.gicp_evaluate(ctx, None, None, neg, _lib.Report()) == _lib.GICP_E_INVALID
    assert b"n_thresholds" in lib.gicp_last_error(ctx)
    with pytest.raises(ValueError, match="robust_scale"):
        eng.evaluate(T, gicp.default_params(3, robust_kernel="huber", robust_scale=0.0, **P3))

    def state_error(e, match):
        with pytest.raises(_lib.GicpError, match=match) as ei:
            e.evaluate()
        assert ei.value.code == _lib.GICP_E_STATE

    fresh = gicp.Engine(0)
    try:
        state_error(fresh, "set_target and set_source first")
        fresh.set_target(sc["tgt"], p)
        state_error(fresh, "set_target and set_source first")
        fresh.set_source(sc["src"], p, shard=0, nshards=2)
        state_error(fresh, "unsharded source")
        fresh.set_source(sc["src"], p)
        fresh.set_allreduce(lambda buf: buf)
        state_error(fresh, "communicator, host hook or peer exchange")
        fresh.set_allreduce(None)
        assert fresh.evaluate()["n_source"] == len(sc["src"])
    finally:
        fresh.close()
    assert eng.evaluate(T)["n_matched"] > 0                  # the refusals left the engine usable


def test_a_communicator_is_refused(scene3d):
    """(Its own test: creating the one-rank RCCL communicator takes seconds.)"""
    e = gicp.Engine(0)
    try:
        e.comm_init(1, 0, gicp.Engine.comm_unique_id())
        _set(e, scene3d)
        with pytest.raises(_lib.GicpError, match="communicator, host hook or peer exchange") as ei:
            e.evaluate(scene3d["T"])
        assert ei.value.code == _lib.GICP_E_STATE
    finally:
        e.close()


# 8 --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lidar_frames():
    return list(S.lidar_stream(5, beams=16, azimuths=600, step=0.15, along_path=True))


@pytest.mark.parametrize("mode", ["scan_to_scan", "scan_to_map"])
def test_odometry_report(lidar_frames, mode):
    from gicp.odometry import Odometry
    kw = dict(map_voxel_size=0.4, map_range=30.0) if mode == "scan_to_map" else {}
    dc = P3["max_distance_correspondence"]
    spec = dict(thresholds=[dc / 4, dc / 2, dc], quantiles=[0.5, 0.9])
    runs = []
    for report in (None, spec):
        odo = Odometry(3, params=gicp.default_params(3, max_iterations=40, tolerance=1e-10, **P3), report=report, **kw)
        try:
            out = [odo.step(scan) for scan, _ in lidar_frames]
            runs.append(([P.copy() for P in odo.poses], out))
        finally:
            odo.eng.close()
    (poses0, out0), (poses1, out1) = runs
    assert len(poses0) == len(poses1) == len(lidar_frames)
    for A, B in zip(poses0, poses1):
        assert np.array_equal(A, B)                          # the report reads the registration, it steers nothing
    assert all(r is None or "report" not in r for _, r in out0) and out1[0] == (None, None)
    for k, (T, res) in enumerate(out1[1:], 1):
        rep = res["report"]
        print(f"{mode} frame {k}: matched {rep['n_matched']} of {rep['n_source']}, fitness {rep['fitness']}, "
              f"dist_q {rep['dist_q']}, eig {rep['eig']}")
        assert rep["n_matched"] > 0 and rep["n_source"] == len(lidar_frames[k - 1 if mode == "scan_to_scan" else k][0])
        assert np.all(np.isfinite(rep["eig"])) and np.all(np.diff(rep["eig"]) >= 0)
        assert rep["dist_q"][0.5] <= rep["dist_q"][0.9] <= dc
        assert rep["white_q"][0.5] <= rep["white_q"][0.9]
        assert rep["inliers"][-1] == rep["n_matched"]
