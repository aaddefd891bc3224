"""Batched registration on the GPU (gicp_batch_align): the covariances of batch clouds against the
oracle's criteria, one pass against edge_ref.pass_reference (ties, the d_c boundary, the three covariance models,
a robust kernel, a problem with no correspondence), the whole loop against Engine.align and the oracle's loop,
the independence of a problem from the rest of its batch, the context left untouched, and multistart.
test_batch_cpu.py asserts the preconditions these cases lean on."""
import numpy as np
import pytest

import batch_ref as B
import edge_ref as E
import gpu_helpers as H
import robust_ref as RR
from oracle import gicp_oracle as O

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


def _params(dim, **kw):
    return gicp.default_params(dim, **kw)


class _BatchCloud:
    """What gpu_helpers.check_covariances asks of an engine, answered from a batch's debug outputs."""

    def __init__(self, C, cnt):
        self.C, self.cnt = C, cnt

    def covariances(self, which="target"):
        return self.C

    def neighbor_counts(self, which="target"):
        return self.cnt


# ============================================================================= 1: covariances
@pytest.mark.parametrize("dim", [2, 3])
def test_covariances_of_batch_clouds(eng, dim):
    """k_batch_cov on clouds of 1, 2, 63, 64, 65, 255, 256, 257 and gicp_batch_max_points rows, all in one batch:
    gpu_helpers.check_covariances' criteria (counts exact, structure 1e-12, eigen-residual 1e-13, entries 1e-8
    where the eigen-gap is >= 1e-2, at most 2 % left out).  3-D also the planar lattice and the cloud whose point 0
    has 24 neighbours tied at its k-th distance (any 19 of them may complete the neighbourhood)."""
    assert B.COV_SIZES[-1] == gicp.batch_max_points(dim)
    clouds = [B.cov_cloud(dim, n) for n in B.COV_SIZES]
    if dim == 3:
        clouds += [H.planar_lattice(), E.tied_kth_cloud()[0]]
    p = H.ladder_params(dim, max_iterations=1, fixed_iterations=1)
    _, _, dbg = eng.align_batch(clouds, [(0, 0)], params=p, debug=True)
    for k, pts in enumerate(clouds[:len(B.COV_SIZES) + (1 if dim == 3 else 0)]):
        C, cnt = dbg["covariances"][k], dbg["neighbor_counts"][k]
        assert C.shape == (len(pts), dim, dim) and cnt.shape == (len(pts),)
        H.check_covariances(_BatchCloud(C, cnt), pts, 1.0)
    if dim == 3:
        pts, tied = E.tied_kth_cloud()
        C, cnt = dbg["covariances"][-1], dbg["neighbor_counts"][-1]
        _, cnt_or = O.covariances(pts, 1.0)
        assert np.array_equal(cnt, cnt_or) and cnt[0] == 20 and np.all(np.isfinite(C))
        assert E.cov_structure_error(C[cnt >= 3], O.EPSILON, O.RATIO).max() <= 1e-12
        res = E.tied_subset_residuals(pts, tied, 19, E.normal_of(C[:1], O.EPSILON, O.RATIO)[0])
        assert res <= H.RESIDUAL_BOUND, res
        rep = E.covariance_report(pts, 1.0, 20, O.EPSILON, O.RATIO, 3, C, cnt)
        assert rep["residual"][25:].max() <= H.RESIDUAL_BOUND


# ============================================================================= 2: one pass
def _check_pass(dbg, b, cs, ct, src, tgt, T, d_c, model="plane_to_plane", robust=None, what=""):
    """Problem b's pass against the oracle with gpu_helpers.check_pass's tolerances (index bit-exact, distance
    rtol 1e-12, statistics rtol 1e-9), from the batch's own covariances of clouds cs and ct."""
    C_s, C_t, cnt_t = dbg["covariances"][cs], dbg["covariances"][ct], dbg["neighbor_counts"][ct]
    if robust:
        idx, dist, _, ref, _, _ = RR.pass_reference(src, tgt, T, d_c, C_s, C_t, model, cnt_t, None, kind=robust[0], c=robust[1])
    else:
        idx, dist, _, ref = E.pass_reference(src, tgt, T, d_c, C_s, C_t, model, cnt_t, None)
    assert np.array_equal(dbg["index"][b], idx), (what, int(np.sum(dbg["index"][b] != idx)))
    np.testing.assert_allclose(dbg["distance"][b], dist, rtol=1e-12, err_msg=what)
    np.testing.assert_allclose(dbg["stats"][b], ref, rtol=1e-9, atol=1e-9 * max(np.max(np.abs(ref)), 1e-300), err_msg=what)
    return idx


PASS_SIZES = [(65, 257), (257, 65), (300, 300), (1, 64), (64, 1)]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("mode", ["plane_to_plane", "point_to_point", "point_to_plane", "huber"])
def test_one_pass_against_the_oracle(eng, dim, mode):
    """max_iterations = 1: every problem's debug outputs are those of the pass at its T0.  Dense patches of several
    size pairs (more source rows than a sweep holds, fewer than a wave, one row, one target), at the identity and
    at gpu_helpers.ladder_pose, under the three covariance models and one robust kernel."""
    model = "plane_to_plane" if mode == "huber" else mode
    robust = ("huber", 1e-3) if mode == "huber" else None
    clouds, pairs, T0 = [], [], []
    for n_src, n_tgt in PASS_SIZES:
        src, tgt = E.dense_patch(dim, n_src, n_tgt, seed=3)
        clouds += [src, tgt]
        for T in (np.eye(dim + 1), H.ladder_pose(src)):
            pairs.append((len(clouds) - 2, len(clouds) - 1))
            T0.append(T)
    p = H.ladder_params(dim, max_iterations=1, fixed_iterations=1, cov_model=_lib.COV_MODELS[model],
                        robust_kernel=robust[0] if robust else None, robust_scale=robust[1] if robust else None)
    T, res, dbg = eng.align_batch(clouds, pairs, np.array(T0), p, debug=True)
    accepted = 0
    for b, ((cs, ct), Tb) in enumerate(zip(pairs, T0)):
        idx = _check_pass(dbg, b, cs, ct, clouds[cs], clouds[ct], Tb, 0.5, model, robust, what=f"{mode} problem {b}")
        assert res[b]["iterations"] == 1 and res[b]["correspondences"] == int(np.sum(idx >= 0))
        accepted += int(np.sum(idx >= 0))
    assert accepted > 500


def test_exact_ties_and_the_d_c_boundary(eng):
    """Targets at exactly equal fp64 distances go to the lower row (edge_ref's lattice: 8-, 4- and 2-way ties and
    duplicated points, at the identity, a dyadic shift and the exact quarter turn); a source at exactly d_c is
    accepted and at the next double below d_c rejected, on 0.25 and on edge_ref.last_accepted_offset's d_c."""
    tgt = E.lattice_target()
    clouds, pairs, T0, want = [tgt], [], [], []
    cap = gicp.batch_max_points(3)                     # (the 2304 edge midpoints exceed a batch cloud)
    for kind, s in E.lattice_sources().items():
        s = s[:cap]
        for name, T in E.lattice_poses().items():
            s_in = E.inverse_moved(s, T)
            assert np.array_equal(O.apply_transformation(s_in, T), s)
            clouds.append(s_in)
            pairs.append((len(clouds) - 1, 0))
            T0.append(T)
            want.append(E.nearest_lowest_index(s, tgt, 0.5))
    p = H.ladder_params(3, max_iterations=1, fixed_iterations=1)
    _, res, dbg = eng.align_batch(clouds, pairs, np.array(T0), p, debug=True)
    for b, (idx, dist) in enumerate(want):
        assert np.all(idx >= 0) and np.array_equal(dbg["index"][b], idx), (b, int(np.sum(dbg["index"][b] != idx)))
        assert np.all(np.abs(dbg["distance"][b] - dist) <= np.spacing(dist))
        assert res[b]["correspondences"] == len(idx) and res[b]["status"] == 0
    # exactly at d_c, and just beyond
    off, d2, d_off = E.last_accepted_offset()
    n_unique = int(np.prod(E.LATTICE))
    edges = E.lattice_sources()["edges"][:cap]
    for src, d_c in ((edges, 0.25), (tgt[:n_unique] + off, d_off)):
        idx, dist = E.nearest_lowest_index(src, tgt, d_c)
        assert np.all(dist == d_c) and np.all(idx >= 0)
        for T in (np.eye(4), E.lattice_poses()["turn"]):
            s_in = E.inverse_moved(src, T)
            assert np.array_equal(O.apply_transformation(s_in, T), src)
            for dc, n_in in ((d_c, len(src)), (float(np.nextafter(d_c, 0)), 0)):
                q = _params(3, max_iterations=1, fixed_iterations=1, max_distance_correspondence=dc, max_distance_nearest_neighbors=1.0)
                Tb, rb, db = eng.align_batch([s_in, tgt], [(0, 1)], T, q, debug=True)
                assert np.all(db["distance"][0] == d_c) and rb[0]["correspondences"] == n_in
                assert np.array_equal(db["index"][0], idx if n_in else np.full(len(src), -1))
                if not n_in:
                    assert rb[0]["status"] == _lib.GICP_E_INVALID and np.array_equal(Tb[0], T)
                    assert np.all(db["stats"][0] == 0)


def test_a_problem_without_correspondences_fails_alone(eng):
    """A source 100 m from its target has no row within d_c: its solve fails, it reports GICP_E_INVALID and keeps
    T0, and the other problems of the batch come out bit for bit as they do without it."""
    src, tgt = E.dense_patch(3, 200, 220, seed=8)
    far = src + 100.0
    Ts = np.array([np.eye(4), H.ladder_pose(src), H.ladder_pose(src)])
    p = H.ladder_params(3, max_iterations=6)
    T, res, dbg = eng.align_batch([src, tgt, far], [(0, 1), (2, 1), (0, 1)], Ts, p, debug=True)
    assert res[1]["status"] == _lib.GICP_E_INVALID and res[1]["correspondences"] == 0
    assert np.array_equal(T[1], Ts[1]) and np.all(dbg["index"][1] == -1) and np.all(dbg["distance"][1] > 50.0)
    assert res[0]["status"] == 0 and res[2]["status"] == 0 and res[0]["correspondences"] > 100
    T2, res2, dbg2 = eng.align_batch([src, tgt], [(0, 1), (0, 1)], Ts[[0, 2]], p, debug=True)
    for a, b in ((0, 0), (2, 1)):
        assert T[a].tobytes() == T2[b].tobytes() and res[a] == res2[b]
        assert dbg["stats"][a].tobytes() == dbg2["stats"][b].tobytes()
    # every weight 0 under Tukey is no failure (gicp_align's rule): the pose stays, the status is 0
    q = H.ladder_params(3, max_iterations=3, robust_kernel="tukey", robust_scale=1e-9)
    T3, res3 = eng.align_batch([src, tgt], [(0, 1)], Ts[1], q)
    assert res3[0]["status"] == 0 and res3[0]["correspondences"] > 100 and np.array_equal(T3[0], Ts[1])


# ============================================================================= 3: the whole loop
def _engine_align(e, src, tgt, p, T0=None):
    e.set_target(tgt, p)
    e.set_source(src, p)
    return e.align(T0, p)


def _close_2d(a, b):
    th = np.arctan2(a[1, 0], a[0, 0]) - np.arctan2(b[1, 0], b[0, 0])
    return abs(th) < 1e-8 and np.max(np.abs(a[:2, 2] - b[:2, 2])) < 1e-6, (th, np.max(np.abs(a[:2, 2] - b[:2, 2])))


def _groups():
    """The 2-D fixtures by their parameters (one gicp_params serves a batch): the robot pairs and the static ones."""
    out = {}
    for name in B.FIXTURES:
        kw = B.fixture(name)[2]
        out.setdefault(tuple(sorted(kw.items())), []).append(name)
    return [(dict(k), names) for k, names in out.items()]


def test_fixed_iterations_against_engine_and_oracle_2d(eng):
    """fixed_iterations, max_iterations = 10 on the eleven convergent 2-D fixtures: every pose within 1e-8 rad and
    1e-6 px (test_2d_1m_fast_mode_vs_oracle's tolerances) of Engine.align's and of the oracle's fixed loop."""
    for kw, names in _groups():
        kw = dict(kw, max_iterations=10)
        p = _params(2, fixed_iterations=1, **kw)
        clouds, pairs = [], []
        for name in names:
            src, tgt, _ = B.fixture(name)
            clouds += [src, tgt]
            pairs.append((len(clouds) - 2, len(clouds) - 1))
        T, res = eng.align_batch(clouds, pairs, params=p)
        e2 = gicp.Engine(0)
        try:
            for b, name in enumerate(names):
                src, tgt, _ = B.fixture(name)
                Te, re_ = _engine_align(e2, src, tgt, p)
                To = O.gicp(src, tgt, inner="gn", source_cov="rotate", fixed_iterations=True, **kw)[0]
                assert res[b]["iterations"] == re_["iterations"] == 10 and res[b]["status"] == 0
                ok, err = _close_2d(T[b], Te)
                assert ok, (name, "engine", err)
                ok, err = _close_2d(T[b], To)
                assert ok, (name, "oracle", err)
        finally:
            e2.close()


def test_fixed_iterations_against_engine_and_oracle_3d(eng):
    """The small room pair, 10 fixed iterations: element-wise within 1e-9 (test_align_1m_vs_oracle_loop's tolerance)
    of Engine.align and of the oracle's fixed loop; twice in the batch, from the identity and from a second start."""
    src, tgt, Tgt = B.room_pair()
    kw = dict(max_iterations=10, tolerance=1e-6, **B.P3)
    p = _params(3, fixed_iterations=1, **kw)
    T1 = H.ladder_pose(src)
    T, res = eng.align_batch([src, tgt], [(0, 1), (0, 1)], np.array([np.eye(4), T1]), p)
    e2 = gicp.Engine(0)
    try:
        for b, T0 in enumerate((np.eye(4), T1)):
            Te, _ = _engine_align(e2, src, tgt, p, T0)
            To = O.gicp(src, tgt, inner="gn", source_cov="rotate", fixed_iterations=True, T0=T0, **kw)[0]
            assert res[b]["iterations"] == 10 and res[b]["status"] == 0
            assert np.max(np.abs(T[b] - Te)) < 1e-9, (b, np.max(np.abs(T[b] - Te)))
            assert np.max(np.abs(T[b] - To)) < 1e-9, (b, np.max(np.abs(T[b] - To)))
    finally:
        e2.close()
    assert S.rotation_angle_error(T[0], Tgt) < S.rotation_angle_error(np.eye(4), Tgt)


STOP_FIELDS = ("iterations", "converged", "converged_at", "stop_reason", "correspondences")


def test_stopping_rules_match_engine_align(eng):
    """With the stopping rules on, iterations, converged_at, stop_reason and correspondences equal Engine.align's:
    the loss rule on every fixture whose |delta loss| test_batch_cpu.py found clear of the tolerance and on the
    room pair, the PCL transform rule (2-D and 3-D), and max_iterations exhausted."""
    e2 = gicp.Engine(0)
    try:
        for kw, names in _groups():
            p = _params(2, **kw)
            clouds, pairs = [], []
            for name in names:
                src, tgt, _ = B.fixture(name)
                clouds += [src, tgt]
                pairs.append((len(clouds) - 2, len(clouds) - 1))
            T, res = eng.align_batch(clouds, pairs, params=p)
            for b, name in enumerate(names):
                src, tgt, _ = B.fixture(name)
                Te, re_ = _engine_align(e2, src, tgt, p)
                got, want = {k: res[b][k] for k in STOP_FIELDS}, {k: re_[k] for k in STOP_FIELDS}
                print(name, got)
                assert got == want and res[b]["stop_reason"] == "loss" and res[b]["status"] == 0, (name, got, want)
                ok, err = _close_2d(T[b], Te)
                assert ok, (name, err)
        src, tgt, _ = B.room_pair()
        cases = [("room loss", 3, src, tgt, dict(max_iterations=100, tolerance=1e-6, **B.P3), "loss", B.ROOM_ITERATIONS + 1)]
        for name in sorted(B.PCL_CASES):
            s, t, kw = B.pcl_case(name)
            cases.append((f"pcl {name}", s.shape[1], s, t, kw, "transform", B.PCL_CASES[name][1] + 1))
        s, t, kw = B.fixture("vis_s2")
        cases.append(("exhausted", 2, s, t, dict(kw, max_iterations=3), "none", 3))
        for what, dim, s, t, kw, reason, iters in cases:
            p = _params(dim, **kw)
            T, res = eng.align_batch([s, t], [(0, 1)], params=p)
            Te, re_ = _engine_align(e2, s, t, p)
            got, want = {k: res[0][k] for k in STOP_FIELDS}, {k: re_[k] for k in STOP_FIELDS}
            print(what, got)
            assert got == want, (what, got, want)
            assert res[0]["stop_reason"] == reason and res[0]["iterations"] == iters, (what, got)
    finally:
        e2.close()


# ============================================================================= 4: independence
def _bits(T, res, dbg, b):
    return T[b].tobytes(), tuple(sorted(res[b].items())), dbg["stats"][b].tobytes()


def test_a_problem_does_not_depend_on_its_batch(eng):
    """300 problems (more than there are CUs) of mixed sizes over shared and distinct clouds, run forwards, reversed
    and ten of them alone, on a second context, and again after an unrelated Engine.align: T_out, every result
    field and the statistics of each problem are the same bits everywhere."""
    rng = np.random.default_rng(12)
    clouds, base = [], []
    for name in B.FIXTURES[:6]:                       # the robot pairs: one parameter set
        src, tgt, _ = B.fixture(name)
        clouds += [src, tgt]
        base.append((len(clouds) - 2, len(clouds) - 1))
    for n in (1, 5, 70, 300, 700):                    # further sizes: subsets of the largest scan
        clouds.append(np.ascontiguousarray(np.resize(clouds[2], (n, 2)) + rng.normal(0, 0.5, (n, 2))))
    extra = [(len(clouds) - k, 3) for k in range(1, 6)] + [(2, len(clouds) - 1), (2, len(clouds) - 5)]
    pairs, T0 = [], []
    for b in range(300):
        pairs.append((base + extra)[b % len(base + extra)])
        T = np.eye(3)
        T[:2, :2] = O.rot2(rng.uniform(-0.05, 0.05))
        T[:2, 2] = rng.uniform(-3.0, 3.0, 2)
        T0.append(T)
    T0 = np.array(T0)
    p = _params(2, **B.fixture(B.FIXTURES[0])[2])
    T, res, dbg = eng.align_batch(clouds, pairs, T0, p, debug=True)
    assert sum(r["converged"] for r in res) >= 150 and len({r["iterations"] for r in res}) > 2
    want = [_bits(T, res, dbg, b) for b in range(300)]

    def same(e, what):
        Tr, rr, dr = e.align_batch(clouds, pairs[::-1], T0[::-1], p, debug=True)
        for b in range(300):
            assert _bits(Tr, rr, dr, 299 - b) == want[b], (what, "reversed", b)
        for b in (0, 7, 11, 12, 13, 64, 150, 255, 256, 299):
            cs, ct = pairs[b]
            Ta, ra, da = e.align_batch([clouds[cs], clouds[ct]], [(0, 1)], T0[b], p, debug=True)
            assert _bits(Ta, ra, da, 0) == want[b], (what, "alone", b)

    same(eng, "first context")
    e2 = gicp.Engine(0)
    try:
        same(e2, "second context")
    finally:
        e2.close()
    src, tgt, _ = B.room_pair()
    _engine_align(eng, src, tgt, _params(3, max_iterations=5, **B.P3))
    T2, res2, dbg2 = eng.align_batch(clouds, pairs, T0, p, debug=True)
    assert [_bits(T2, res2, dbg2, b) for b in range(300)] == want


# ============================================================================= 5: the context
def test_the_context_is_left_as_it_was(eng):
    """An engine with both clouds set under a voxel filter and a warm cache: iterate and align give the same bits
    before and after a batch call, cloud sizes, points and settings are unchanged, and the filter still applies to
    the next cloud (and never to batch clouds)."""
    src, tgt, _ = B.room_pair()
    p = _params(3, max_iterations=30, **B.P3)
    e = gicp.Engine(0)
    try:
        e.set_voxel(0.3)
        e.set_filter(max_range=50.0)
        settings = (e.voxel, dict(e.filter))
        e.set_target(tgt, p)
        e.set_source(src, p)
        n_t, n_s = e.cloud_size("target"), e.cloud_size("source")
        assert n_t < len(tgt) and n_s < len(src)
        e.align(None, p)                                  # warm cache
        T1 = H.ladder_pose(src)
        st0 = e.iterate(T1)
        Ta0, ra0 = e.align(None, p)
        pts0 = (e.points("target").tobytes(), e.points("source").tobytes())
        Tb, rb, db = e.align_batch([src, tgt], [(0, 1), (1, 0)], params=p, debug=True)
        assert len(db["covariances"][0]) == len(src) and len(db["index"][1]) == len(tgt)    # batch clouds: unfiltered
        assert (e.voxel, dict(e.filter)) == settings and e.voxel[0] == 0.3
        assert (e.cloud_size("target"), e.cloud_size("source")) == (n_t, n_s)
        assert (e.points("target").tobytes(), e.points("source").tobytes()) == pts0
        st1 = e.iterate(T1)
        Ta1, ra1 = e.align(None, p)
        assert st1.tobytes() == st0.tobytes() and Ta1.tobytes() == Ta0.tobytes()
        for k in ("iterations", "converged", "converged_at", "stop_reason", "correspondences", "final_loss", "mse"):
            assert ra1[k] == ra0[k], k
        e.set_target(tgt, p)
        assert e.cloud_size("target") == n_t               # the voxel filter is still in force
    finally:
        e.close()


# ============================================================================= 6: multistart
def test_multistart_against_sequential_aligns(eng):
    """gicp.multistart over yaw starts of one scan pair, three fixed iterations (the starts are still apart): its
    poses are Engine.align's from the same starts (1e-8 rad, 1e-6 px) and its choice the one the same rule makes
    from the sequential results, which no tie leaves to rounding."""
    src, tgt, kw = B.fixture("robot_p1_r360")
    kw = dict(kw, max_iterations=3, max_distance_correspondence=40.0)
    T0s = []
    for deg in (-30.0, -15.0, -5.0, 0.0, 10.0, 25.0):
        T0s.append(E.pose_about(src.mean(axis=0), O.rot2(np.deg2rad(deg)), [0.0, 0.0]))
    best, T, res = gicp.multistart(src, tgt, T0s, fixed_iterations=1, **kw)
    p = _params(2, fixed_iterations=1, **kw)
    e2 = gicp.Engine(0)
    try:
        seq = []
        for b, T0 in enumerate(T0s):
            Te, re_ = _engine_align(e2, src, tgt, p, T0)
            ok, err = _close_2d(T[b], Te)
            assert ok, (b, err)
            assert res[b]["correspondences"] == re_["correspondences"] and res[b]["iterations"] == 3
            np.testing.assert_allclose(res[b]["mse"], re_["mse"], rtol=1e-9)
            seq.append(dict(status=0, correspondences=re_["correspondences"], mse=re_["mse"]))
    finally:
        e2.close()
    keys = sorted((-r["correspondences"], r["mse"]) for r in seq)
    assert keys[0][0] < keys[1][0] or keys[1][1] - keys[0][1] > 1e-6 * keys[1][1], keys[:2]
    assert best == gicp.pick_start(seq) and res[best]["status"] == 0
    assert len({r["correspondences"] for r in res}) > 1
