"""A context's results must not depend on its call history.

One gicp_ctx keeps state between calls -- nearest-neighbour certificates, candidate lists, tile hints, the
pose ring, batch_hint, top_k_pref, grow-only device buffers, and psrc, which gicp_align rewrites -- and the
header promises that only the time depends on it.  Every step here is judged by two yardsticks:

  the oracle    O.correspondences for indices and accepted counts (bit-exact), E.pass_reference with the
                tolerances of gpu_helpers.check_pass for distances, weights and statistics;
  a fresh engine that performs only that step from cold: np.array_equal on statistics, index, distance,
                pose, final_loss, iterations, converged_at, correspondences and mse.

A: d_c schedules on a warm context; B: the covariance model switched on a warm context; C: cloud swaps
(size, dimension, promotion, voxel filter, staged targets, the map, shards) on one context; D: every build
path of a cloud (set_target, staged, staged with a borrowed buffer -- the last two run k_knn_cov with
split = 1) at the edges of k_knn_cov; E: batch_hint and top_k_pref; F: a failed build leaves no half-built
cloud; G: engines taken from creation to close through every optional buffer group, four in turn, leave no
device memory behind.  make_engine, check_pass, VARIANTS and the covariance criteria are tests/gpu_helpers.py's,
shared with test_gpu_edges.py."""
import ctypes as C
import itertools
import subprocess
import sys

import numpy as np
import pytest

import density_ref as D
import edge_ref as E
import gpu_helpers as G
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402

P = {3: G.P3, 2: G.P2}          # d_c 0.5 / d_n 1.0 on the 3-D room, d_c 20 / d_n 25 on the 2-D segments
CREEP = 2e-5                     # the per-pass displacement of test_pose_ring_wraps_under_live_certificates


def params(dim, **kw):
    return gicp.default_params(dim, **{**P[dim], **kw})


@pytest.fixture(scope="module")
def scenes():
    """{dim: (source, target, pose at which most points have a correspondence)}"""
    s3, t3, T3 = S.scene_pair_3d(4000)
    s2, t2, _ = S.segment_scene_2d(4000)
    return {3: (s3, t3, T3), 2: (s2, t2, np.eye(3))}


def crept(T, k=1):
    """T displaced by k * 2e-5 along the first axis."""
    out = np.array(T, dtype=np.float64)
    out[0, -1] += k * CREEP
    return out


def warm_up(e, T):
    """Two passes along a creeping pose: certificates, lists, hints and ring entries to go stale."""
    e.iterate(T)
    e.iterate(crept(T))


ALIGN_KEYS = ("iterations", "converged", "converged_at", "stop_reason", "final_loss", "correspondences", "mse")


def same_align(a, b, what):
    """Two (T, result[, trace]) of Engine.align, bit for bit."""
    assert np.array_equal(a[0], b[0]), (what, "pose", np.max(np.abs(a[0] - b[0])))
    for k in ALIGN_KEYS:
        assert a[1][k] == b[1][k], (what, k, a[1][k], b[1][k])
    if len(a) > 2:
        assert np.array_equal(a[2]["losses"], b[2]["losses"]), (what, "trace losses")
        assert np.array_equal(a[2]["poses"], b[2]["poses"]), (what, "trace poses")


def same_pass(a, b, what):
    """Two (statistics, debug) of Engine.iterate(debug=True), bit for bit (a row without a target within
    the screen holds -1, zeros and a non-finite distance: the same one in both)."""
    assert np.array_equal(a[0], b[0]), (what, "statistics", np.max(np.abs(a[0] - b[0])))
    for k in ("index", "distance", "weight"):
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), (what, k, int(np.sum(a[1][k] != b[1][k])))


def same_clouds(a, b, what, graph=True):
    """Covariances, neighbour counts and the target graph of two engines, bit for bit."""
    for which in ("target", "source"):
        assert np.array_equal(a.covariances(which), b.covariances(which)), (what, which, "covariances")
        assert np.array_equal(a.neighbor_counts(which), b.neighbor_counts(which)), (what, which, "counts")
    if graph:
        (ia, ra), (ib, rb) = a.graph(), b.graph()
        assert np.array_equal(ra, rb), (what, "graph radius")
        assert np.array_equal(ia, ib), (what, "graph index")


# ============================================================================= A: d_c schedule on a warm context
SCHEDULES = {3: (0.5, 1.5, 0.25, 1.0, 0.5), 2: (10.0, 20.0, 2.0, 10.0, 5.0)}
MIN_FLIPS = 900


@pytest.mark.parametrize("variant", list(G.VARIANTS))
@pytest.mark.parametrize("dim", [3, 2])
def test_d_c_schedule_on_a_warm_context(scenes, monkeypatch, dim, variant):
    """gicp_align changes psrc.max_distance_correspondence and resets no cache.  One engine, clouds set once;
    for every d_c of the schedule a one-iteration align at the scene's pose -- the first pass at the new d_c
    over certificates, empty-lane radii and lists built at the old one -- then an iterate 2e-5 away, which
    must run at the d_c the align left behind.  Every transition flips the accept status of at least 900 of
    the 4000 points (asserted from the oracle: 3-D 1922, 3986, 585, 3699, 1922 accepted; 2-D 3012, 3995, 468,
    3012, 1401).  The align's count is the oracle's exactly and the align is bit-identical to a cold engine
    given the same call; the iterate meets check_pass against the oracle at this d_c."""
    src, tgt, T = scenes[dim]
    moved = O.apply_transformation(src, T)
    accepted = [O.correspondences(moved, tgt, d_c)[0] >= 0 for d_c in SCHEDULES[dim]]
    print(f"{dim}-D accepted: {[int(a.sum()) for a in accepted]}")
    for a, b in zip(accepted, accepted[1:]):
        assert np.sum(a != b) >= MIN_FLIPS, int(np.sum(a != b))
    p0 = params(dim)
    e = G.make_engine(monkeypatch, **G.VARIANTS[variant])
    try:
        e.set_target(tgt, p0)
        e.set_source(src, p0)
        for step, d_c in enumerate(SCHEDULES[dim]):
            what = f"{dim}-D {variant} step {step} d_c {d_c}"
            pa = params(dim, max_distance_correspondence=d_c, max_iterations=1, fixed_iterations=1)
            warm = e.align(T, pa, trace=True)
            assert warm[1]["correspondences"] == int(accepted[step].sum()), (what, warm[1]["correspondences"])
            cold = G.make_engine(monkeypatch, **G.VARIANTS[variant])
            try:
                cold.set_target(tgt, p0)
                cold.set_source(src, p0)
                same_align(warm, cold.align(T, pa, trace=True), what)
            finally:
                cold.close()
            G.check_pass(e, src, tgt, crept(T), d_c, what=what)
    finally:
        e.close()


# ============================================================================= B: covariance model on a warm context
def test_cov_model_switched_on_a_warm_context(scenes, monkeypatch):
    """gicp_align changes psrc.cov_model and resets no cache: plane_to_plane -> point_to_point ->
    point_to_plane -> plane_to_plane on one engine, each an 8-iteration align from the identity (bit-identical
    to a cold engine given the same call) followed by one iterate at the align's pose, whose weights and
    statistics must be those of the model the align left in force (check_pass, model=...)."""
    src, tgt, _ = scenes[3]
    p0 = params(3)
    e = G.make_engine(monkeypatch)
    try:
        e.set_target(tgt, p0)
        e.set_source(src, p0)
        for step, model in enumerate(["plane_to_plane", "point_to_point", "point_to_plane", "plane_to_plane"]):
            what = f"step {step} {model}"
            pa = params(3, cov_model=_lib.COV_MODELS[model], max_iterations=8, fixed_iterations=1)
            warm = e.align(None, pa)
            assert warm[1]["iterations"] == 8 and warm[1]["correspondences"] > 500
            cold = G.make_engine(monkeypatch)
            try:
                cold.set_target(tgt, p0)
                cold.set_source(src, p0)
                same_align(warm, cold.align(None, pa), what)
            finally:
                cold.close()
            G.check_pass(e, src, tgt, warm[0], P[3]["max_distance_correspondence"], model=model, what=what)
    finally:
        e.close()


# ============================================================================= C: cloud swaps on one context
def check_step(e, monkeypatch, src, tgt, p, T, what, voxel=0.0, build=None, **env):
    """After a swap on the long-lived engine `e`, which now holds (src, tgt) set with p: the first pass at T
    and the clouds, bit for bit those of a fresh engine given only this pair (build(fresh) when the pair
    cannot simply be set); a second pass at T against the oracle and equal to the first; then two warm
    passes, so that the next swap finds state to go stale."""
    dim = src.shape[1]
    first = e.iterate(T, debug=True)
    fresh = G.make_engine(monkeypatch, **env)
    try:
        if voxel > 0:
            fresh.set_voxel(voxel)
        if build is not None:
            build(fresh)
        else:
            fresh.set_target(tgt, p)
            fresh.set_source(src, p)
        assert (e.cloud_size("source"), e.cloud_size("target")) == (fresh.cloud_size("source"), fresh.cloud_size("target"))
        if voxel > 0:   # per-point outputs refer to the filtered clouds: the oracle runs on the engine's points
            src, tgt = e.points("source"), e.points("target")
            assert np.array_equal(src, fresh.points("source")) and np.array_equal(tgt, fresh.points("target"))
        assert (e.n_src, e.n_tgt) == (len(src), len(tgt)), what
        same_clouds(e, fresh, what)
        same_pass(first, fresh.iterate(T, debug=True), what)
    finally:
        fresh.close()
    st, _ = G.check_pass(e, src, tgt, T, p.max_distance_correspondence, what=what)
    assert np.array_equal(st, first[0]), what
    warm_up(e, T)
    return first


def test_cloud_swaps_on_one_context(scenes, monkeypatch):
    """Grow-only buffers, hints, lists and certificates across clouds of other sizes and another dimension,
    promotions, the voxel filter switched on and off, staged targets and the map, on ONE engine; after every
    step check_step: the oracle, and a fresh engine that holds only the current pair, bit for bit
    (covariances, neighbour counts, graph index and radius, statistics, index, distance, weights)."""
    s3, t3, T3 = scenes[3]
    s2, t2, T2 = scenes[2]
    p3, p2 = params(3), params(2)
    moved = O.apply_transformation(s3, T3)      # the source registered: lies on the target
    I4 = np.eye(4)
    small_s, small_t = E.dense_patch(3, 65, 129)
    e = G.make_engine(monkeypatch)
    step = lambda *a, **kw: check_step(e, monkeypatch, *a, **kw)   # noqa: E731
    try:
        e.set_target(t3, p3)
        e.set_source(s3, p3)
        a = step(s3, t3, p3, T3, "1: 4000 x 4000")
        assert a[0][-1] > 1500
        e.set_source(s3[:65], p3)
        step(s3[:65], t3, p3, T3, "2: source of 65")
        e.set_source(s3[:1], p3)
        step(s3[:1], t3, p3, T3, "3: source of 1")
        e.set_source(s3, p3)
        b = step(s3, t3, p3, T3, "4: source of 4000 again")
        same_pass(a, b, "4 against 1")
        e.set_target(t3[:129], p3)               # the source and its warm state are kept
        step(s3, t3[:129], p3, T3, "5: target of 129 under a warm source")
        e.set_target(small_t, p3)                # ... and a target elsewhere in space (the dense patch)
        step(s3, small_t, p3, T3, "5b: a distant target of 129")
        e.set_target(t3, p3)
        b = step(s3, t3, p3, T3, "6: target of 4000 again")
        same_pass(a, b, "6 against 1")
        e.target_to_source()
        e.set_target(moved, p3)
        c = step(t3, moved, p3, I4, "7: target promoted, the moved source as target")
        assert c[0][-1] > 1500
        e.set_target(t2, p2)
        e.set_source(s2, p2)
        d2 = step(s2, t2, p2, T2, "8: the 2-D pair")
        assert d2[0][-1] > 3000
        e.set_target(t3, p3)
        e.set_source(s3, p3)
        b = step(s3, t3, p3, T3, "9: the 3-D pair again")
        same_pass(a, b, "9 against 1")
        e.set_voxel(0.25)
        e.set_target(t3, p3)
        e.set_source(s3, p3)
        step(s3, t3, p3, T3, "10: voxel filter 0.25", voxel=0.25)
        e.set_voxel(0)
        e.set_target(t3, p3)
        e.set_source(s3, p3)
        b = step(s3, t3, p3, T3, "10b: voxel filter off")
        same_pass(a, b, "10b against 1")
        # 11: two staged targets, committed one after the other with passes in between
        half = np.ascontiguousarray(t3[:1500])
        e.stage_target(moved, p3)
        e.stage_target(half, p3, borrow=True)
        e.commit_target()                        # source <- t3, target <- moved
        b = step(t3, moved, p3, I4, "11a: first staged target committed")
        same_pass(c, b, "11a against 7")
        e.commit_target()                        # source <- moved, target <- t3[:1500]
        step(moved, half, p3, I4, "11b: second staged target committed")
        # 12: the map's centroids as the target, the source kept
        e.map_reset(0.2, 1000.0, 3)
        e.map_insert(I4, points=t3)
        e.map_insert(I4, points=s3)
        _, cent, cnt = e.map_get()
        e.map_to_target(p3)
        assert e.n_tgt == len(cent) and np.all(cnt >= 1)
        step(moved, cent, p3, I4, "12: the map as target under a warm source")
        e.set_source(small_s, p3)
        e.set_target(small_t, p3)
        step(small_s, small_t, p3, G.ladder_pose(small_s), "13: 65 x 129 at the end")
    finally:
        e.cancel_stage()
        e.close()


def test_shards_switched_on_one_context(monkeypatch):
    """257 points in 16-point source tiles (test_shards_of_small_clouds's clouds): set_source with shard 0,
    1, 2 of 3 in turn on one engine, two passes each; the three statistics sum to the unsharded pass (1e-12,
    that test's tolerance), and back at one shard the clouds and the pass are bit-equal to a cold engine."""
    src, tgt = E.dense_patch(3, 257, 257)
    p = G.ladder_params(3)
    T = G.ladder_pose(src)
    env = dict(GICP_SRC_TILE="16")
    e = G.make_engine(monkeypatch, **env)
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        warm_up(e, T)
        parts = []
        for s in range(3):
            e.set_source(src, p, shard=s, nshards=3)
            parts.append(e.iterate(T))
            assert np.array_equal(parts[-1], e.iterate(T)), s
            e.iterate(crept(T))
        e.set_source(src, p)
        full = check_step(e, monkeypatch, src, tgt, p, T, "unsharded after three shards", **env)
        assert full[0][-1] >= 0.5 * len(src)
        np.testing.assert_allclose(np.sum(parts, axis=0), full[0], rtol=1e-12, atol=1e-12 * np.max(np.abs(full[0])))
    finally:
        e.close()


# ============================================================================= D: every build path of a cloud
PATHS = ("set_target", "staged", "staged_borrowed")
# Share of the points that the entrywise comparison may leave out (relative eigen-gap of the ORACLE's
# neighbourhood below 1e-2: the normal is then ill-determined whoever computes it) -- a figure of the cloud
# and the oracle alone.  2 % is check_covariances' default; the 4000-point room at d_n = 1.0 has 5.15 % such
# points (206 of 4000: 3- and 4-point neighbourhoods that are nearly collinear; computed from the oracle on
# the CPU), so the bound is that figure and a tenth of a per cent.
LEFT_OUT_ROOM_D_N_1 = 0.0525


def build_by(e, path, pts, p):
    """`pts` as the engine's target through one of the three build paths."""
    if path == "set_target":
        e.set_target(pts, p)
        return
    e.stage_target(np.ascontiguousarray(pts), p, borrow=path == "staged_borrowed")
    e.commit_target()


def _lattice_checks(e, pts, d_n, dim):
    cnt = e.neighbor_counts("target")
    _, cnt_or = O.covariances(pts, d_n, 20 if dim == 3 else 10)
    assert np.array_equal(cnt, cnt_or)
    inner = np.all((pts[:, :2] >= 1.0) & (pts[:, :2] <= 4.5), axis=1)
    assert np.all(cnt[inner] == (9 if d_n == 1.0 else 13))
    C = e.covariances("target")
    if dim == 3:
        want = np.diag([O.EPSILON, O.EPSILON, O.EPSILON * O.RATIO])
        assert np.all(cnt >= 3)
        assert np.max(np.abs(C - want)) <= 1e-12 * O.EPSILON, np.max(np.abs(C - want))
    else:
        # in the plane the lattice's neighbourhoods are isotropic away from the border (both eigenvalues of
        # the sample covariance equal: any normal will do), so the criteria are the counts, the structure
        # C = a I - m m^T, the eigen-residual, and the entries wherever the oracle's eigen-gap allows
        G.check_covariances(e, pts, d_n, max_left_out=1.0, k_neighbors=10)


def tied_neighbourhoods(pts, i, d_n, k):
    """The neighbourhoods a k-nearest search (self included, strictly nearer than d_n) may return for point i,
    by brute force in fp64: the points strictly nearer than the k-th candidate, plus every way to fill up
    to k from those exactly as far as it.  One index array per choice (one array when no tie decides)."""
    d2 = np.zeros(len(pts))
    for a in range(pts.shape[1]):
        d2 += (pts[:, a] - pts[i, a]) ** 2
    cand = np.nonzero(np.sqrt(d2) < d_n)[0]
    if len(cand) <= k:
        return [cand]
    dk = np.sort(d2[cand])[k - 1]
    sure, tie = cand[d2[cand] < dk], cand[d2[cand] == dk]
    return [np.concatenate([sure, c]).astype(np.int64) for c in itertools.combinations(tie, k - len(sure))]


def _lattice_2d_tied_checks(e, pts, d_n, k=10):
    """The 2-D lattice with the points at exactly 1.0 inside d_n: counts exactly the oracle's ({6, 8, 9} on
    the border, the cap 10 inside); C = a I - m m^T with the eigenvalues {eps ratio, eps} to 1e-12 on every
    row; on the rows no tie decides, the criteria of check_covariances against the oracle's neighbourhood
    (eigen-residual 1e-13, entries 1e-8 where the oracle's eigen-gap is >= 1e-2); on the rows whose k-th
    neighbour lies inside a tie, the normal is an eigenvector, to 1e-13, of the sample covariance of one of
    the neighbourhoods the tie allows (the criterion of test_tied_kth_neighbour)."""
    cnt = e.neighbor_counts("target")
    C = e.covariances("target")
    rep = E.covariance_report(pts, d_n, k, O.EPSILON, O.RATIO, 2, C, cnt)
    assert rep["count_ok"], int(np.sum(cnt != rep["counts"]))
    assert set(cnt.tolist()) == {6, 8, 9, 10} and np.all(rep["surface"])
    assert np.all(np.isfinite(C)) and rep["structure"].max() <= 1e-12, rep["structure"].max()
    hoods = [tied_neighbourhoods(pts, i, d_n, k) for i in range(len(pts))]
    free = np.array([len(h) == 1 for h in hoods])
    assert free.sum() == 44 and np.all(cnt[~free] == k) and np.all(cnt[free] < k)
    assert rep["residual"][free].max() <= G.RESIDUAL_BOUND, rep["residual"][free].max()
    wide = free & (rep["gap"] >= 1e-2)
    assert wide.sum() == 44 and rep["entry_err"][wide].max() <= 1e-8, rep["entry_err"][wide].max()   # (gaps >= 0.55)
    nrm = E.normal_of(C, O.EPSILON, O.RATIO)
    worst = 0.0
    for i in np.nonzero(~free)[0]:
        assert 2 <= len(hoods[i]) <= 6, (i, len(hoods[i]))
        worst = max(worst, min(E.eigen_residual(E.sample_covariance(pts[h]), nrm[i]) for h in hoods[i]))
    print(f"2-D lattice above 1.0: worst best-subset eigen-residual over the {int((~free).sum())} tied rows {worst:.2e}")
    assert worst <= G.RESIDUAL_BOUND, worst


def _line_checks(e, pts, u, dim):
    C = e.covariances("target")
    cnt = e.neighbor_counts("target")
    _, cnt_or = O.covariances(pts, 1.0)
    assert np.array_equal(cnt, cnt_or) and np.all(np.isfinite(C))
    assert E.cov_structure_error(C, O.EPSILON, O.RATIO).max() <= 1e-12
    n = E.normal_of(C, O.EPSILON, O.RATIO)
    assert np.max(np.abs(n @ u)) <= 1e-12, np.max(np.abs(n @ u))


def _coincident_checks(e, pts, dim):
    C = e.covariances("target")
    assert np.array_equal(e.neighbor_counts("target"), np.full(len(pts), O.default_k(dim))) and np.all(np.isfinite(C))
    assert E.cov_structure_error(C, O.EPSILON, O.RATIO).max() <= 1e-12


def _tied_checks(e, pts, tied):
    cnt = e.neighbor_counts("target")
    _, cnt_or = O.covariances(pts, 1.0)
    assert np.array_equal(cnt, cnt_or) and cnt[0] == 20
    C = e.covariances("target")
    assert np.all(np.isfinite(C))
    surf = cnt >= 3
    assert E.cov_structure_error(C[surf], O.EPSILON, O.RATIO).max() <= 1e-12
    n0 = E.normal_of(C[:1], O.EPSILON, O.RATIO)[0]
    res = E.tied_subset_residuals(pts, tied, 19, n0)
    assert res <= G.RESIDUAL_BOUND, res
    far = np.arange(25, len(pts))
    rep = E.covariance_report(pts, 1.0, 20, O.EPSILON, O.RATIO, 3, C, cnt)
    assert rep["residual"][far].max() <= G.RESIDUAL_BOUND, rep["residual"][far].max()


def _edge_clouds():
    """name -> (points, params, check(engine)) of section D."""
    out = {}
    lat = G.planar_lattice()
    for tag, d_n in (("1.0", 1.0), ("above_1.0", float(np.nextafter(1.0, 2)))):
        p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=d_n)
        out[f"lattice_3d_dn_{tag}"] = (lat, p, lambda e, d_n=d_n: _lattice_checks(e, lat, d_n, 3))
    # the 2-D form with k = 10.  At d_n = 1.0 the points at exactly 1.0 are excluded (interior: 9 neighbours);
    # with the next fp64 above 1.0 they count, the 100 inner points have 11 to 13 candidates and the k = 10 cut
    # falls inside the tie at distance 1.0, the 44 border points have 6, 8 or 9 and no tie
    lat2 = np.ascontiguousarray(lat[:, :2])
    p = gicp.default_params(2, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0, k_neighbors=10)
    out["lattice_2d_dn_1.0"] = (lat2, p, lambda e: _lattice_checks(e, lat2, 1.0, 2))
    above = float(np.nextafter(1.0, 2))
    p = gicp.default_params(2, max_distance_correspondence=0.5, max_distance_nearest_neighbors=above, k_neighbors=10)
    out["lattice_2d_dn_above_1.0"] = (lat2, p, lambda e: _lattice_2d_tied_checks(e, lat2, above))
    pts, tied = E.tied_kth_cloud()
    out["tied_kth_3d"] = (pts, params(3), lambda e: _tied_checks(e, pts, tied))
    u3 = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    line3 = np.array([3.0, -1.0, 2.0]) + np.arange(200)[:, None] * 0.05 * u3
    out["collinear_3d"] = (line3, params(3), lambda e: _line_checks(e, line3, u3, 3))
    u2 = np.array([1.0, 2.0]) / np.linalg.norm([1.0, 2.0])
    line2 = np.array([3.0, -1.0]) + np.arange(200)[:, None] * 0.05 * u2
    pl2 = gicp.default_params(2, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
    out["collinear_2d"] = (line2, pl2, lambda e: _line_checks(e, line2, u2, 2))
    same3 = np.tile(np.array([[0.375, -1.25, 2.5]]), (30, 1))
    out["coincident_3d"] = (same3, params(3), lambda e: _coincident_checks(e, same3, 3))
    same2 = np.ascontiguousarray(same3[:, :2])
    out["coincident_2d"] = (same2, pl2, lambda e: _coincident_checks(e, same2, 2))
    for dim in (3, 2):
        for n in (1, 63, 64, 65, 129):
            patch = E.dense_patch(dim, n, n)[1]
            out[f"size_{n}_{dim}d"] = (patch, G.ladder_params(dim),
                                       lambda e, patch=patch: G.check_covariances(e, patch, 1.0, "target"))
    # clouds whose grid the build cannot resolve (tests/density_ref.py): one cell for the whole core, tiles
    # kilometres wide around a dense core
    for name in DENSITY_CLOUDS:
        f = D.fixture(name)
        pd = gicp.default_params(f["dim"], **D.params_kw(f))
        out[name] = (f["target"], pd, lambda e, f=f, name=name: G.check_covariances(
            e, f["target"], f["d_n"], "target", max_left_out=D.max_left_out(name, "target")))
    return out


DENSITY_CLOUDS = ["stretched_3d", "halo_3d", "stretched_2d"]
EDGE_CLOUDS = ["lattice_3d_dn_1.0", "lattice_3d_dn_above_1.0", "lattice_2d_dn_1.0", "lattice_2d_dn_above_1.0",
               "tied_kth_3d", "collinear_3d", "collinear_2d", "coincident_3d", "coincident_2d"] + [f"size_{n}_{d}d" for d in (3, 2)
                                                                     for n in (1, 63, 64, 65, 129)] + ["size_4000_3d",
                                                                                                       "size_4000_2d"] + DENSITY_CLOUDS


@pytest.fixture(scope="module")
def edge_clouds(scenes):
    out = _edge_clouds()
    t3, t2 = scenes[3][1], scenes[2][1]
    out["size_4000_3d"] = (t3, params(3), lambda e: G.check_covariances(e, t3, 1.0, "target",
                                                                        max_left_out=LEFT_OUT_ROOM_D_N_1))
    out["size_4000_2d"] = (t2, params(2), lambda e: G.check_covariances(e, t2, 25.0, "target"))
    assert sorted(out) == sorted(EDGE_CLOUDS)
    return out


@pytest.fixture(scope="module")
def path_engine():
    e = gicp.Engine(0)
    yield e
    e.cancel_stage()
    e.close()


@pytest.mark.parametrize("cloud", EDGE_CLOUDS)
def test_every_build_path_agrees(path_engine, edge_clouds, cloud):
    """The same target through set_target (k_knn_cov split by sub-tile on these small clouds), a staged
    build and a staged build of a borrowed buffer (both split = 1, one wave per tile): for each path the
    criteria of the cloud's own edge test in test_gpu_edges.py -- neighbour counts exactly the oracle's,
    covariances within that test's tolerances -- and graph rows that cover their radius (every row, brute
    force); between the paths counts, graph radius and covariances bit-equal.

    Covariances are asserted with array_equal because the summation order in k_knn_cov does not depend on
    the split: a wave visits its own tile, then the others in ascending tile order (traverse_c), rows in
    ascending order inside a tile; the split only changes the culling box (qb) and which lanes of the wave
    hold a query, and culling skips nothing a lane takes (its keys exceed the lane's bound).  The lists of
    phase 1 are sorted keys, independent of the order they were met in.  So each lane adds the same rows
    in the same order whatever the split.  Measured on an MI355X: maximum |difference| between the paths 0.0
    on every cloud of this test."""
    pts, p, check = edge_clouds[cloud]
    e = path_engine
    got = {}
    for path in PATHS:
        build_by(e, path, pts, p)
        assert e.n_tgt == len(pts)
        check(e)
        idx, rad = e.graph()
        G.graph_rows_cover_their_radius(pts, idx, rad)
        got[path] = (e.covariances("target"), e.neighbor_counts("target"), rad)
    ref = got["set_target"]
    for path in PATHS[1:]:
        print(f"{cloud} {path}: max |C - C(set_target)| = {np.max(np.abs(got[path][0] - ref[0])):.3e}")
        assert np.array_equal(got[path][1], ref[1]), (path, "counts")
        assert np.array_equal(got[path][2], ref[2]), (path, "graph radius")
        assert np.array_equal(got[path][0], ref[0]), (path, "covariances", np.max(np.abs(got[path][0] - ref[0])))


# ============================================================================= E: other state carried between calls
SENTINEL = -7.25


def align_traced(e, T0, p, dim):
    """gicp_align_trace with every trace row prefilled with SENTINEL: (T, result dict, poses, losses), all
    `capacity` rows."""
    cap = int(p.max_iterations)
    poses = np.full((cap, dim + 1, dim + 1), SENTINEL)
    losses = np.full(cap, SENTINEL)
    tr = _lib.Trace(cap, 0, _lib.dptr(poses), _lib.dptr(losses), None, None, None)
    T0 = np.ascontiguousarray(T0, dtype=np.float64)
    Tout = np.empty((dim + 1, dim + 1))
    res = _lib.Result()
    _lib.check(e._lib.gicp_align_trace(e._ctx, _lib.dptr(T0), C.byref(p), _lib.dptr(Tout), C.byref(res), C.byref(tr)),
               e._ctx, "gicp_align_trace")
    r = res.as_dict()
    r["stop_reason"] = _lib.STOP_REASONS.get(r["stop_reason"], r["stop_reason"])
    return Tout, r, poses, losses


def test_batch_hint_changes_no_result(scenes, monkeypatch):
    """A long converging align (more than 8 iterations) leaves batch_hint behind: the next align on the
    context enqueues that many launches before its first host sync.  Started from the first one's result it
    stops after a few iterations, so most of those launches run after convergence and must exit at
    once: pose, iterations, converged_at and stop_reason bit-equal to a cold engine (whose first batch is 8),
    the trace rows of the executed iterations too, and the rows at or beyond `iterations` untouched.
    (max_iterations is 60: from the identity this scene needs 36 iterations to meet tolerance = 1e-9 -- the
    oracle's loop, on the CPU -- and an align that ends unconverged at a smaller cap leaves no batch_hint.)"""
    src, tgt, _ = scenes[3]
    p0 = params(3)
    pa = params(3, tolerance=1e-9, max_iterations=60)
    e = G.make_engine(monkeypatch)
    cold = G.make_engine(monkeypatch)
    try:
        for x in (e, cold):
            x.set_target(tgt, p0)
            x.set_source(src, p0)
        T1, r1 = e.align(np.eye(4), pa)
        assert r1["converged"] == 1 and r1["stop_reason"] == "loss" and 8 < r1["iterations"] < 60, r1
        warm = align_traced(e, T1, pa, 3)
        ref = align_traced(cold, T1, pa, 3)
        n = warm[1]["iterations"]
        assert 1 <= n <= 4 and warm[1]["converged"] == 1, warm[1]     # fewer than the first batch of either engine
        assert np.array_equal(warm[0], ref[0])
        for k in ALIGN_KEYS:
            assert warm[1][k] == ref[1][k], (k, warm[1][k], ref[1][k])
        for got in (warm, ref):
            assert np.all(got[2][n:] == SENTINEL) and np.all(got[3][n:] == SENTINEL)
            assert np.all(got[2][:n] != SENTINEL) and np.array_equal(got[2][0], T1)
        assert np.array_equal(warm[2], ref[2]) and np.array_equal(warm[3], ref[3])
    finally:
        e.close()
        cold.close()


def test_top_k_preference_changes_no_result(scenes, monkeypatch):
    """gicp_top_weights remembers the k of the last call and the next pass computes that k in its own
    stream sync: k = 5, 16, 1, 5 on one engine, each against the stable argsort of det(W) of the same pass
    (the criteria of test_top_weights_vs_argsort), and the second k = 5 bit-equal to the first."""
    src, tgt, T = scenes[3]
    p = params(3)
    e = G.make_engine(monkeypatch)
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        st0, dbg = e.iterate(T, debug=True)
        det = np.linalg.det(dbg["weight"])
        order = np.argsort(det, kind="stable")
        seen = {}
        for k in (5, 16, 1, 5):
            ref = order[-k:]
            st, si, ti, dt = e.iterate_top(T, k)
            assert np.array_equal(st, st0), k
            np.testing.assert_allclose(dt, det[ref], rtol=1e-9)
            np.testing.assert_allclose(det[si], det[ref], rtol=1e-9)
            if len(np.unique(np.round(det[ref], 6))) == k:
                assert np.array_equal(si, ref), k
            assert np.array_equal(ti, dbg["index"][si]), k
            if k in seen:
                for x, y in zip(seen[k], (si, ti, dt)):
                    assert np.array_equal(x, y), k
            seen[k] = (si, ti, dt)
    finally:
        e.close()


# ============================================================================= F: a failed build leaves no half-built cloud
def _state_error(fn):
    with pytest.raises(_lib.GicpError) as ei:
        fn()
    assert ei.value.code == _lib.GICP_E_STATE, ei.value


FAILURES = [(call, kind, dim) for call in ("set_target", "set_source") for kind, dim in
            (("k7", 3), ("k7", 2), ("non_finite", 3))] + [("map_to_target", "k7", 3), ("map_to_target", "k7", 2)]


@pytest.mark.parametrize("call,kind,dim", FAILURES, ids=[f"{c}-{k}-{d}d" for c, k, d in FAILURES])
def test_failed_build_leaves_no_half_built_cloud(scenes, monkeypatch, call, kind, dim):
    """gicp_set_target, gicp_set_source and gicp_map_to_target that fail -- k_neighbors = 7, which no
    k_knn_cov instance serves and which is only found out after the new tiles are in place, or a non-finite
    coordinate -- leave that cloud NOT SET: size 0, and GICP_E_STATE from gicp_iterate, gicp_align,
    gicp_get_covariances, gicp_get_neighbor_counts and gicp_get_graph (no pass is launched over new tiles
    with stale covariances, or from a source whose hints point into the old target's tiles).  The other
    cloud is untouched, and after a good rebuild the pass meets the oracle and everything is bit-equal to
    a fresh engine."""
    src, tgt, T = scenes[dim]
    p = params(dim)
    which = "source" if call == "set_source" else "target"
    other = "target" if which == "source" else "source"
    e = G.make_engine(monkeypatch)
    try:
        good = tgt
        if call == "map_to_target":
            e.map_reset(5.0 if dim == 2 else 0.2, 1e4, dim)
            e.map_insert(np.eye(dim + 1), points=tgt)
            good = e.map_get()[1]
            assert len(good) > 1000                                  # (1476 cells in 2-D, 3962 in 3-D)
        e.set_target(good, p)
        e.set_source(src, p)
        warm_up(e, T)
        before = (e.covariances(other), e.neighbor_counts(other), e.cloud_size(other))
        # the failing call
        bad_p = params(dim, k_neighbors=7) if kind == "k7" else p
        bad = (tgt if which == "target" else src)[:3000].copy()     # another size: new tiles, were they kept
        text = "unsupported k_neighbors"
        if kind == "non_finite":
            bad[1234, 1] = np.inf
            text = "non-finite"
        with pytest.raises(ValueError, match=text):                  # GICP_E_INVALID carrying the library's text
            if call == "map_to_target":
                e.map_to_target(bad_p)
            elif call == "set_target":
                e.set_target(bad, bad_p)
            else:
                e.set_source(bad, bad_p)
        # not set: refused on the host
        assert e.cloud_size(which) == 0 and e.cloud_size(other) == before[2]
        _state_error(lambda: e.iterate(T))
        _state_error(lambda: e.align(T, params(dim, max_iterations=2)))
        _state_error(lambda: e.covariances(which))
        _state_error(lambda: e.neighbor_counts(which))
        if which == "target":
            _state_error(e.graph)
        assert np.array_equal(e.covariances(other), before[0]) and np.array_equal(e.neighbor_counts(other), before[1])
        # a good rebuild of that cloud alone
        if call == "map_to_target":
            e.map_to_target(p)
        elif call == "set_target":
            e.set_target(good, p)
        else:
            e.set_source(src, p)
        assert np.array_equal(e.covariances(other), before[0]) and np.array_equal(e.neighbor_counts(other), before[1])
        check_step(e, monkeypatch, src, good, p, T, f"{call} {kind} {dim}-D after the rebuild")
    finally:
        e.close()


# ============================================================================= G: a context's whole lifecycle
BIG_M = 600_000                  # the larger target: 4 * BIG_M bytes is the bound on the memory growth below
TOP_K = 5


@pytest.fixture(scope="module")
def big_target(scenes):
    """BIG_M points of the room the 4000-point scenes are drawn from, in the target's frame."""
    return S.scene_pair_3d(4000, BIG_M)[1]


def lifecycle(e, monkeypatch, scenes, big, verify):
    """One engine from creation to close through every optional buffer group: the voxel filter, both clouds,
    the debug and top-k outputs, the trace rows, rotated covariances, a staged target committed and a borrowed
    one cancelled, a promotion, the map, and a larger target so that the grow paths run.  Returns what each
    step computed.  verify: every step is also held to the oracle and to a fresh engine that performs only
    that step (check_step and the criteria of sections A and E)."""
    s3, t3, T3 = scenes[3]
    p = params(3)
    I4 = np.eye(4)
    moved = O.apply_transformation(s3, T3)
    def step(src, tgt, p_, T, what, **kw):
        return check_step(e, monkeypatch, src, tgt, p_, T, what, **kw) if verify else e.iterate(T, debug=True)
    out = {}
    try:
        e.set_voxel(0.25)
        e.set_target(t3, p)
        e.set_source(s3, p)
        out["voxel"] = step(s3, t3, p, T3, "G: voxel filter 0.25", voxel=0.25)
        e.set_voxel(0)
        e.set_target(t3, p)
        e.set_source(s3, p)
        out["pair"] = step(s3, t3, p, T3, "G: 4000 x 4000")
        out["top"] = e.iterate_top(T3, TOP_K)
        pa = params(3, max_iterations=2, fixed_iterations=1)
        out["align"] = e.align(T3, pa, trace=True, top_k=TOP_K)
        R = S.axis_angle([1.0, -2.0, 0.5], 0.3)
        out["rot"] = e.rotated_covariances(R, "source")
        if verify:
            st, dbg = out["pair"]
            det = np.linalg.det(dbg["weight"])
            ref = np.argsort(det, kind="stable")[-TOP_K:]
            _, si, ti, dt = out["top"]
            assert np.array_equal(out["top"][0], st)
            np.testing.assert_allclose(dt, det[ref], rtol=1e-9)
            np.testing.assert_allclose(det[si], det[ref], rtol=1e-9)
            assert np.array_equal(ti, dbg["index"][si])
            _, res, tr = out["align"]
            assert res["iterations"] == 2 and np.array_equal(tr["poses"][0], T3)
            np.testing.assert_allclose(tr["top_det"][0], det[ref], rtol=1e-9)     # (the first pass ran at T3)
            assert np.array_equal(tr["top_tgt"][0], dbg["index"][tr["top_src"][0]])
            ref_rot = np.einsum("ab,nbc,dc->nad", R, e.covariances("source"), R)
            np.testing.assert_allclose(out["rot"], ref_rot, rtol=0, atol=1e-12 * np.abs(ref_rot).max())
            fresh = G.make_engine(monkeypatch)
            try:
                fresh.set_target(t3, p)
                fresh.set_source(s3, p)
                for x, y in zip(out["top"], fresh.iterate_top(T3, TOP_K)):
                    assert np.array_equal(x, y), "G: iterate_top"
                cold = fresh.align(T3, pa, trace=True, top_k=TOP_K)
                same_align(out["align"], cold, "G: align")
                for k in ("top_src", "top_tgt", "top_det"):
                    assert np.array_equal(out["align"][2][k], cold[2][k]), ("G: align", k)
                assert np.array_equal(out["rot"], fresh.rotated_covariances(R, "source")), "G: rotated covariances"
            finally:
                fresh.close()
        e.stage_target(moved, p)                 # copied into the slot's pinned buffer
        e.commit_target()                        # source <- t3, target <- moved
        out["staged"] = step(t3, moved, p, I4, "G: staged target committed")
        e.stage_target(np.ascontiguousarray(t3[:1500]), p, borrow=True)
        e.cancel_stage()
        e.target_to_source()                     # source <- moved, no target
        e.map_reset(0.2, 1000.0, 3)
        e.map_insert(I4, points=t3)
        e.map_insert(I4, which="source")
        cent = e.map_get()[1]
        e.map_to_target(p)

        def from_map(f):
            f.set_source(moved, p)
            f.map_reset(0.2, 1000.0, 3)
            f.map_insert(I4, points=t3)
            f.map_insert(I4, which="source")
            f.map_to_target(p)
        out["map"] = step(moved, cent, p, I4, "G: the map as target", build=from_map)
        e.set_target(big, p)
        out["big"] = step(moved, big, p, I4, "G: the larger target")
    finally:
        e.cancel_stage()
        e.close()
    return out


# The device's free memory as torch reports it, read in a child process: hipMemGetInfo counts the whole device,
# this process's allocations included, and torch brings its own HIP runtime, which finds no GPU when it is
# initialised in a process where the library's runtime already holds one (which of the two comes first would
# depend on the tests that ran before).  One child, started before the first cycle, answers every request.
MEM_PROBE = """
import sys, torch
torch.cuda.init()
print("ready", flush=True)
for _ in sys.stdin:
    torch.cuda.synchronize()
    print(torch.cuda.mem_get_info(0)[0], flush=True)
"""


def test_lifecycle_leaves_no_memory_behind(scenes, big_target, monkeypatch):
    """Four engines in turn, each created, taken through lifecycle() and closed (which synchronises its
    streams).  The first one's steps are held to the oracle and to fresh engines; the other three must compute
    the same bits.  The device's free memory (torch.cuda.mem_get_info after a synchronise, see MEM_PROBE) after
    the fourth close may lie below its value after the first by less than one per-point int32 buffer of the
    larger target, 4 * BIG_M bytes: a buffer that close() does not release would be lost three times over.
    BIG_M is chosen so that this bound is above the 2 MiB steps in which the counter moves on an MI355X
    (profiles/hostmem/README.md; measured growth there: 0 bytes, before and after the owners became DevBufs)."""
    probe = subprocess.Popen([sys.executable, "-c", MEM_PROBE], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def free_bytes():
        probe.stdin.write("\n")
        probe.stdin.flush()
        line = probe.stdout.readline()
        assert line.strip().isdigit(), f"the memory probe gave {line!r}"
        return int(line)

    try:
        first = lifecycle(G.make_engine(monkeypatch), monkeypatch, scenes, big_target, verify=True)
        assert probe.stdout.readline().strip() == "ready", "the memory probe could not initialise torch.cuda"
        free1 = free_bytes()
        for cycle in (2, 3, 4):
            again = lifecycle(G.make_engine(monkeypatch), monkeypatch, scenes, big_target, verify=False)
            for k in ("voxel", "pair", "staged", "map", "big"):
                same_pass(first[k], again[k], f"G: cycle {cycle} {k}")
            for x, y in zip(first["top"], again["top"]):
                assert np.array_equal(x, y), cycle
            same_align(first["align"], again["align"], f"G: cycle {cycle} align")
            assert np.array_equal(first["rot"], again["rot"]), cycle
        free4 = free_bytes()
    finally:
        probe.stdin.close()
        probe.wait(timeout=60)
    print(f"free after cycle 1: {free1}, after cycle 4: {free4}, growth {free1 - free4} bytes (bound {4 * BIG_M})")
    assert free1 - free4 < 4 * BIG_M, (free1, free4)
