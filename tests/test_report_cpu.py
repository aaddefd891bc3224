"""The registration report without a GPU (include/gicp_hip.h "registration report"): the host-only
entry points gicp_information and gicp_sym_eig against the NumPy restatement tests/report_ref.py and np.linalg.eigh,
and the Python wrapper and Odometry(report=...) on the NumPy fake of the device entry points
(tests/fake_device.py) with gicp_evaluate added on top of report_ref."""
import ctypes as C

import numpy as np
import pytest

import edge_ref as E
import report_ref as RR
import robust_ref as R
from golden_util import load, names

gicp = pytest.importorskip("gicp")
from fake_device import E_INVALID, E_STATE, OK, PASS_INFO, _arr  # noqa: E402
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from oracle import gicp_oracle as O  # noqa: E402
from test_map_cpu import FakeMapLib  # noqa: E402

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
MODELS = {"plane_to_plane": 0, "point_to_point": 1, "point_to_plane": 2}


def _pose3(deg=2.0, t=(0.06, -0.05, 0.06)):
    T = np.eye(4)
    T[:3, :3] = S.axis_angle([1.0, -2.0, 0.5], np.deg2rad(deg))
    T[:3, 3] = t
    return T


# ---- gicp_information ------------------------------------------------------------------------------------

def _check_information(src, q, W, idx, T, what):
    """H within 1e-12 max|H| of the per-point sum; b within 1e-12 of its own scale sqrt(max H_kk c0), the
    Cauchy-Schwarz bound of |sum J^T W r|."""
    st = O.stats(src, q, W, idx, T)
    H, b = gicp.information(st, T)
    Hr, br = RR.information_ref(src, q, W, idx, T)
    n = RR.twist_size(src.shape[1])
    assert H.shape == (n, n) and b.shape == (n,)
    scale = np.max(np.abs(Hr))
    c0 = RR.frozen_loss(src, q, W, idx, T)
    eh, eb = np.max(np.abs(H - Hr)), np.max(np.abs(b - br))
    print(f"{what}: |H - ref| = {eh:.2e} of max|H| {scale:.3g}; |b - ref| = {eb:.2e} of max|b| {np.max(np.abs(br)):.3g}")
    assert eh <= 1e-12 * scale, (what, eh, scale)
    assert eb <= 1e-12 * np.sqrt(np.max(np.diag(Hr)) * c0), (what, eb)
    assert np.array_equal(H, H.T) or np.max(np.abs(H - H.T)) <= 1e-12 * scale
    return H, b


@pytest.mark.parametrize("name", names())
def test_information_on_every_golden_2d_iteration(name):
    fx = load(name)
    src = fx["source"]
    assert src.shape[1] == 2
    for k in range(len(fx["W"])):
        _check_information(src, fx["q"][k], fx["W"][k], fx["idx"][k], fx["all_T"][k], f"{name}[{k}]")


@pytest.fixture(scope="module")
def room():
    src, tgt, _ = S.scene_pair_3d(3000)
    C_s, _ = O.covariances(src, P3["max_distance_nearest_neighbors"])
    C_t, cnt_t = O.covariances(tgt, P3["max_distance_nearest_neighbors"])
    return dict(src=src, tgt=tgt, C_s=C_s, C_t=C_t, cnt_t=cnt_t, T=_pose3())


def _room_pass(room, model, kind):
    src, tgt, T = room["src"], room["tgt"], room["T"]
    d_c = P3["max_distance_correspondence"]
    idx, dist, W, _ = E.pass_reference(src, tgt, T, d_c, room["C_s"], room["C_t"], model, room["cnt_t"])
    if kind != "none":
        e = R.reweight(src, tgt, idx, W, T, "none", 1.0)[1]
        c = float(np.sqrt(np.median(e[idx >= 0])))
        W = R.reweight(src, tgt, idx, W, T, kind, c)[3]
    return idx, dist, W, RR.matches(tgt, idx)


@pytest.mark.parametrize("kind", ["none", "cauchy"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_information_3d_room_and_finite_difference(room, model, kind):
    src, T = room["src"], room["T"]
    idx, _, W, q = _room_pass(room, model, kind)
    assert 300 < np.sum(idx >= 0) < 2700
    H, b = _check_information(src, q, W, idx, T, f"room {model} {kind}")
    # the sign and the side of the perturbation: d/dh loss(Exp(h e_k) T) = 2 b_k, loosely
    h = 1e-5
    fd = np.empty(6)
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        fd[k] = (RR.frozen_loss(src, q, W, idx, RR.perturbed(T, xi)) - RR.frozen_loss(src, q, W, idx, RR.perturbed(T, -xi))) / (2 * h)
    print("finite difference", fd, "2 b", 2 * b)
    assert np.max(np.abs(fd - 2 * b)) <= 1e-5 * np.max(np.abs(2 * b))
    # ... and a right perturbation, or the opposite sign, is not within that
    assert np.max(np.abs(fd + 2 * b)) > 1e-2 * np.max(np.abs(2 * b))


def test_information_2d_finite_difference():
    fx = load("segment_2k")
    src, q, W, idx, T = fx["source"], fx["q"][0], fx["W"][0], fx["idx"][0], fx["all_T"][0]
    T = T @ O.offset_to_T([3.0, -2.0, 0.02])      # away from the identity: the two perturbation sides differ
    _, b = _check_information(src, q, W, idx, T, "segment_2k moved")
    fd = np.empty(3)
    for k, h in enumerate((1e-7, 1e-4, 1e-4)):    # (coordinates ~1e3: a smaller angle step)
        xi = np.zeros(3)
        xi[k] = h
        fd[k] = (RR.frozen_loss(src, q, W, idx, RR.perturbed(T, xi)) - RR.frozen_loss(src, q, W, idx, RR.perturbed(T, -xi))) / (2 * h)
    assert np.max(np.abs(fd - 2 * b) / np.abs(2 * b)) <= 1e-5, (fd, 2 * b)


def test_information_argument_errors():
    st = np.zeros(74)
    with pytest.raises(ValueError):
        gicp.information(st, np.eye(3))                      # 2-D pose, 3-D statistics
    with pytest.raises(ValueError):
        gicp.information(np.zeros(26), np.full((3, 3), np.nan))
    lib = _lib.load()
    H, b = np.empty(36), np.empty(6)
    Tm = np.eye(4)
    assert lib.gicp_information(4, _lib.dptr(st), _lib.dptr(Tm), _lib.dptr(H), _lib.dptr(b)) == _lib.GICP_E_INVALID
    assert lib.gicp_information(3, None, _lib.dptr(Tm), _lib.dptr(H), _lib.dptr(b)) == _lib.GICP_E_INVALID
    H, b = gicp.information(st, Tm)                          # no correspondences: zeros
    assert not H.any() and not b.any()


# ---- gicp_sym_eig ----------------------------------------------------------------------------------------

def _eig_cases(n, rng):
    B = rng.normal(size=(n, n))
    Q = np.linalg.qr(rng.normal(size=(n, n)))[0]
    yield "spd", B @ B.T + 0.1 * np.eye(n)
    yield "spd scaled 1e8", 1e8 * (B @ B.T)
    yield "spd scaled 1e-8", 1e-8 * (B @ B.T)
    yield "graded", Q @ np.diag(10.0 ** (-2.0 * np.arange(n))) @ Q.T
    yield "rank 1", np.outer(B[:, 0], B[:, 0])
    if n > 2:
        yield "rank n - 2", B[:, :n - 2] @ B[:, :n - 2].T
    yield "zero", np.zeros((n, n))
    yield "diagonal", np.diag(rng.uniform(-3.0, 3.0, n))
    yield "identity", np.eye(n)
    lam = np.array([2.0] * (n - n // 2) + [5.0] * (n // 2))
    yield "repeated", Q @ np.diag(lam) @ Q.T
    yield "indefinite", 0.5 * (B + B.T)


@pytest.mark.parametrize("n", [1, 3, 6])
def test_sym_eig_against_eigh(n):
    rng = np.random.default_rng(10 + n)
    for seed in range(5):
        for what, A in _eig_cases(n, rng):
            w, V = gicp.sym_eig(A)
            As = 0.5 * (A + A.T)
            norm = np.linalg.norm(As, 2)
            assert np.all(np.diff(w) >= 0), (what, w)
            assert np.max(np.abs(w - np.linalg.eigvalsh(As))) <= 1e-12 * norm, (what, n, seed)
            tol = 1e-12 * max(norm, 1.0)
            assert np.max(np.abs(V @ np.diag(w) @ V.T - As)) <= tol, (what, n, seed)
            assert np.max(np.abs(V.T @ V - np.eye(n))) <= tol, (what, n, seed)


def test_sym_eig_uses_the_symmetric_part_and_refuses_bad_input():
    A = np.array([[2.0, 1.0, 0.0], [0.0, 3.0, 4.0], [0.0, 0.0, 1.0]])
    w, _ = gicp.sym_eig(A)
    np.testing.assert_allclose(w, np.linalg.eigvalsh(0.5 * (A + A.T)), atol=1e-14)
    with pytest.raises(ValueError):
        gicp.sym_eig(np.zeros((7, 7)))
    with pytest.raises(ValueError):
        gicp.sym_eig(np.array([[1.0, np.inf], [np.inf, 1.0]]))
    with pytest.raises(ValueError):
        gicp.sym_eig(np.zeros((2, 3)))


def test_reference_quantile_is_numpys_lower():
    """report_ref.lower_quantile states the definition; np.quantile(method='lower') is the same statistic."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 10, 11, 680, 1001):
        v = rng.uniform(0, 1, n)
        for pi in (0.0, 0.25, 0.5, 0.9, 1.0, 0.499, 0.501):
            assert RR.lower_quantile(v, pi) == np.quantile(v, pi, method="lower"), (n, pi)
    assert np.isnan(RR.lower_quantile([], 0.5))


# ---- the wrapper and Odometry(report=...) on the fake device ---------------------------------------------

class FakeReportLib(FakeMapLib):
    """The fake device plus gicp_evaluate from report_ref (H, b and the spectra from the real library's host
    entry points, as the library itself forms them), and the two host-only calls passed through."""

    def __init__(self, real, ndev=2):
        super().__init__(real, ndev)
        self.evaluations = 0

    def gicp_information(self, *a):
        return self._real.gicp_information(*a)

    def gicp_sym_eig(self, *a):
        return self._real.gicp_sym_eig(*a)

    def gicp_evaluate(self, ctx, T_ptr, p, spec, out):
        c = self._c(ctx)
        self.evaluations += 1
        if c.src is None or c.tgt is None:
            return self._fail(c, E_STATE, "set_target and set_source first")
        if c.nshards > 1:
            return self._fail(c, E_STATE, "gicp_evaluate needs an unsharded source (nshards == 1)")
        if c.hook is not None:
            return self._fail(c, E_STATE, "gicp_evaluate needs a context without a communicator, host hook or peer exchange")
        if not out:
            return self._fail(c, E_INVALID, "out must not be NULL")
        par = (p._obj if hasattr(p, "_obj") else p) if p else c.psrc
        sp = (spec._obj if hasattr(spec, "_obj") else spec) if spec else None
        nt, nq = (sp.n_thresholds, sp.n_quantiles) if sp else (0, 0)
        if not (0 <= nt <= 8 and 0 <= nq <= 8):
            return self._fail(c, E_INVALID, "n_thresholds / n_quantiles must be 0..GICP_REPORT_MAX")
        thr, qs = list(sp.thresholds[:nt]) if sp else [], list(sp.quantiles[:nq]) if sp else []
        if any(not (np.isfinite(t) and 0 <= t <= par.max_distance_correspondence) for t in thr):
            return self._fail(c, E_INVALID, "a threshold must be finite and in [0, max_distance_correspondence] of the pass")
        if any(not (0 <= v <= 1) for v in qs):
            return self._fail(c, E_INVALID, "a quantile probability must be in [0, 1]")
        src = c.src["pts"]
        d = src.shape[1]
        T = np.eye(d + 1) if not T_ptr else _arr(T_ptr, (d + 1, d + 1)).copy()
        if not np.all(np.isfinite(T)):
            return self._fail(c, E_INVALID, "pose contains non-finite values")
        force, c.psrc = c.psrc, par                         # this pass alone
        try:
            ext, per = self._pass(c, T)
        finally:
            c.psrc = force
        c.last_info = ext[len(ext) - PASS_INFO:]
        idx, W = per["idx"], np.where((per["idx"] >= 0)[:, None, None], per["W"], 0.0)
        ref = RR.report_ref(src, RR.matches(c.tgt["pts"], idx), W, idx, per["dist"], T, thr, qs)
        r = out._obj if hasattr(out, "_obj") else out
        n, nw = RR.twist_size(d), RR.twist_size(d) - d
        r.dim, r.n_thresholds, r.n_quantiles = d, nt, nq
        r.n_source, r.n_matched = len(src), ref["n_matched"]
        r.sum_sq, r.loss = ext[len(ext) - PASS_INFO + 3], ext[len(ext) - PASS_INFO - 2]
        H, b = np.empty((n, n)), np.empty(n)
        dp = _lib.dptr
        st = np.ascontiguousarray(ext[:O.stats_size(d)])
        self._real.gicp_information(d, dp(st), dp(np.ascontiguousarray(T)), dp(H), dp(b))
        for name, vec, A in (("eig", "eigvec", H), ("eig_rot", "vec_rot", H[:nw, :nw]), ("eig_trans", "vec_trans", H[nw:, nw:])):
            A = np.ascontiguousarray(A)
            w, V = np.empty(len(A)), np.empty(A.shape)
            self._real.gicp_sym_eig(len(A), dp(A), dp(w), dp(V))
            getattr(r, name)[:len(w)] = w.tolist()
            getattr(r, vec)[:V.size] = V.ravel().tolist()
        r.H[:n * n] = H.ravel().tolist()
        r.b[:n] = b.tolist()
        for k in range(nt):
            r.inliers[k], r.inlier_sum_sq[k] = int(ref["inliers"][k]), float(ref["inlier_sum_sq"][k])
        for k in range(8):
            r.dist_q[k] = ref["dist_q"][qs[k]] if k < nq else float("nan")
            r.white_q[k] = ref["white_q"][qs[k]] if k < nq else float("nan")
        return OK


@pytest.fixture
def fake(monkeypatch):
    lib = FakeReportLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", lib)
    monkeypatch.setattr(gicp, "_ENGINES", {})
    return lib


@pytest.fixture(scope="module")
def pair():
    src, tgt, _ = S.scene_pair_3d(1200)
    return src, tgt


def _engine(pair, **kw):
    src, tgt = pair
    p = gicp.default_params(3, **P3, **kw)
    eng = gicp.Engine(0)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    return eng, p


def test_evaluate_dict_on_the_fake_device(fake, pair):
    src, tgt = pair
    eng, _ = _engine(pair)
    T = _pose3(1.0, (0.03, -0.02, 0.02))
    thr, qs = (0.1, 0.25, 0.5), (0.0, 0.5, 0.9, 1.0)
    rep = eng.evaluate(T, thresholds=thr, quantiles=qs)
    st, dbg = eng.iterate(T, debug=True)
    ref = RR.report_ref(src, RR.matches(tgt, dbg["index"]), dbg["weight"], dbg["index"], dbg["distance"], T, thr, qs)
    assert rep["H"].shape == (6, 6) and rep["b"].shape == (6,) and rep["eigvec"].shape == (6, 6)
    assert rep["vec_rot"].shape == (3, 3) and rep["vec_trans"].shape == (3, 3)
    H, b = gicp.information(st, T)
    assert np.array_equal(rep["H"], H) and np.array_equal(rep["b"], b)
    assert np.array_equal(rep["eig"], gicp.sym_eig(H)[0]) and np.array_equal(rep["eig_trans"], gicp.sym_eig(H[3:, 3:])[0])
    np.testing.assert_allclose(rep["H"], ref["H"], rtol=0, atol=1e-12 * np.max(np.abs(ref["H"])))
    assert rep["n_source"] == len(src) and rep["n_matched"] == ref["n_matched"] == st[-1] > 0
    assert rep["loss"] == st[-2] and rep["sum_sq"] == eng.pass_info()["sum_sq"]
    assert np.array_equal(rep["inliers"], ref["inliers"]) and rep["inliers"].dtype == np.int64
    assert np.array_equal(rep["fitness"], ref["inliers"] / len(src))
    assert np.array_equal(rep["inlier_rmse"], np.sqrt(ref["inlier_sum_sq"] / ref["inliers"]))
    assert list(rep["dist_q"]) == list(qs) and rep["dist_q"] == ref["dist_q"] and rep["white_q"] == ref["white_q"]
    assert rep["inliers"][-1] == rep["n_matched"]           # tau = d_c, inclusive as d_c is
    none = eng.evaluate()                                   # identity, nothing asked
    assert none["inliers"].shape == (0,) and none["dist_q"] == {} and none["H"].shape == (6, 6)


def test_evaluate_2d_shapes_on_the_fake_device(fake):
    src, tgt, _ = S.segment_scene_2d(300)
    p = gicp.default_params(2, max_distance_correspondence=20.0, max_distance_nearest_neighbors=25.0)
    eng = gicp.Engine(0)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    rep = eng.evaluate(np.eye(3), thresholds=[5.0], quantiles=[0.5])
    assert rep["dim"] == 2 and rep["H"].shape == (3, 3) and rep["eig"].shape == (3,)
    assert rep["eig_rot"].shape == (1,) and rep["vec_rot"].shape == (1, 1) and rep["vec_trans"].shape == (2, 2)
    assert rep["eig_rot"][0] == rep["H"][0, 0]


def test_evaluate_restores_the_parameters_in_force(fake, pair):
    eng, p = _engine(pair)
    T = _pose3(1.0, (0.03, -0.02, 0.02))
    eng.align(None, gicp.default_params(3, max_iterations=2, **P3))
    before = eng.iterate(T)
    other = gicp.default_params(3, max_distance_correspondence=0.2, max_distance_nearest_neighbors=1.0,
                                cov_model=MODELS["point_to_point"])
    rep = eng.evaluate(T, other, thresholds=[0.2])
    assert rep["n_matched"] < before[-1]                    # the tighter d_c was used for that pass
    assert rep["eig_trans"][0] == pytest.approx(rep["n_matched"])   # W = I: H_vv = n I
    assert np.array_equal(eng.iterate(T), before)           # ... and for that pass alone
    same = eng.evaluate(T, thresholds=[0.5])                # params None: the values in force
    assert same["n_matched"] == before[-1]
    with pytest.raises(ValueError, match="threshold"):      # a failed evaluate leaves them alone too
        eng.evaluate(T, other, thresholds=[0.3])
    assert np.array_equal(eng.iterate(T), before)


def test_evaluate_argument_and_state_errors(fake, pair):
    src, tgt = pair
    eng, p = _engine(pair)
    for kw, match in ((dict(thresholds=[0.6]), "threshold"), (dict(thresholds=[-0.1]), "threshold"),
                      (dict(thresholds=[np.nan]), "threshold"), (dict(quantiles=[1.5]), "quantile"),
                      (dict(quantiles=[np.nan]), "quantile"), (dict(thresholds=[0.1] * 9), "GICP_REPORT_MAX"),
                      (dict(quantiles=[0.5] * 9), "GICP_REPORT_MAX")):
        with pytest.raises(ValueError, match=match):
            eng.evaluate(np.eye(4), **kw)
    bad = np.eye(4)
    bad[0, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        eng.evaluate(bad)
    fresh = gicp.Engine(0)
    with pytest.raises(_lib.GicpError) as ei:
        fresh.evaluate()
    assert ei.value.code == _lib.GICP_E_STATE
    eng.set_source(src, p, shard=0, nshards=2)
    with pytest.raises(_lib.GicpError, match="unsharded") as ei:
        eng.evaluate()
    assert ei.value.code == _lib.GICP_E_STATE
    eng.set_source(src, p)
    eng.set_allreduce(lambda buf: buf)
    with pytest.raises(_lib.GicpError, match="hook") as ei:
        eng.evaluate()
    assert ei.value.code == _lib.GICP_E_STATE


@pytest.fixture(scope="module")
def stream():
    return list(S.lidar_stream(4, beams=8, azimuths=240, step=0.15, along_path=True))


@pytest.mark.parametrize("mode", ["scan", "map"])
def test_odometry_report_on_the_fake_device(fake, stream, mode):
    from gicp.odometry import Odometry
    kw = dict(map_voxel_size=0.25, map_range=30.0) if mode == "map" else {}
    spec = dict(thresholds=[0.125, 0.25, 0.5], quantiles=[0.5, 0.9])

    def run(report):
        odo = Odometry(3, params=gicp.default_params(3, max_iterations=4, tolerance=1e-9, **P3), report=report, **kw)
        out = [odo.step(scan) for scan, _ in stream]
        return odo, out

    plain, out0 = run(None)
    assert fake.evaluations == 0 and "report_s" not in plain.timing        # report=None: no new entry point
    assert all(r is None or "report" not in r for _, r in out0)
    odo, out = run(spec)
    assert fake.evaluations == len(stream) - 1 and odo.timing["report_s"] > 0
    assert len(odo.poses) == len(plain.poses)
    for A, B in zip(odo.poses, plain.poses):
        assert np.array_equal(A, B)
    assert out[0] == (None, None)
    for T, res in out[1:]:
        rep = res["report"]
        assert rep["n_matched"] > 0 and np.all(np.isfinite(rep["eig"])) and np.all(np.diff(rep["eig"]) >= 0)
        assert rep["dist_q"][0.5] <= rep["dist_q"][0.9] <= 0.5
        assert np.all(np.diff(rep["inliers"]) >= 0) and rep["inliers"][-1] == rep["n_matched"]
    with pytest.raises(ValueError, match="report"):
        Odometry(3, report=dict(threshold=[0.1]))


def test_report_signatures_and_version():
    names_ = {"gicp_evaluate", "gicp_information", "gicp_sym_eig"}
    assert names_ <= set(_lib.SIGNATURES)
    lib = _lib.load()
    for n in names_:
        assert hasattr(lib, n), n
    assert lib.gicp_version() >= 103
    assert _lib.REPORT_MAX == 8 and C.sizeof(_lib.ReportSpec) == 8 + 16 * 8
    i = _lib.HASH_SRCS.index("csrc/gicp_eval.hip")
    assert _lib.HASH_SRCS[i - 1] == "csrc/gicp_sweep.hip"
