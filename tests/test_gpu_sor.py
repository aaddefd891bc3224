"""Statistical outlier removal on the device (gicp_sor.hip): the one-shot against the NumPy restatement
(tests/sor_ref.py) bit for bit -- means, mu, sigma, thr, kept rows -- at every size and k where the kernels take another
path, on coincident and tied inputs, under a permutation of the rows and with the threshold put on a row's mean to the
ulp; the stage fused into every cloud build against a plain build of the survivors bit for bit (synchronous, staged,
borrowed, sharded, chained with the other filters); independence of the context's history; refusals; Odometry.

On stretched_3d, stretched_2d and offset_origin_3d the survivors are exactly the core (asserted on the CPU,
tests/test_sor_cpu.py), so the fused builds must equal the core-only builds of test_gpu_filter.py in every bit."""
import functools

import numpy as np
import pytest

import density_ref as D
import knn_ref as K
import sor_ref as R
import test_gpu_filter as TF      # the comparison of two engines' states, and the core-only builds it caches

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from gicp.odometry import Odometry  # noqa: E402

pytestmark = pytest.mark.gpu

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)


# ---- 1. the one-shot against the reference ---------------------------------------------------------------

def _cases():
    return [(dim, name) for dim in (2, 3) for name in R.case_table(dim, big=True)]


@pytest.mark.parametrize("dim,name", _cases())
def test_one_shot_matches_reference(dim, name):
    _, pts, k, ratio = R.case_table(dim, True)[name]
    R.check(gicp.sor_points, pts, k, ratio, R.expected(dim, name, True), name)


@pytest.mark.parametrize("dim", [2, 3])
def test_one_shot_equals_the_host_function(dim):
    for name in ("rows_3_k31", "rows_257_k8", "rows_4097_k16", "coincident_k31", f"lattice_k{2 * dim}"):
        _, pts, k, ratio = R.case_table(dim)[name]
        got = gicp.sor_points(pts, k, ratio, return_index=True, return_mean=True, return_stats=True)
        want = gicp.sor_points_host(pts, k, ratio, return_index=True, return_mean=True, return_stats=True)
        assert all(R.same_bits(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3], name


def test_a_clump_larger_than_k_survives():
    """offset_origin_3d at k = 8 (tests/test_sor_cpu.py has the figures): 12 returns about the origin are each other's
    neighbours and stay."""
    f = D.fixture("offset_origin_3d")
    R.check(gicp.sor_points, f["source"], 8, 1.0, None, "offset_origin_3d_k8")


@pytest.mark.parametrize("dim", [2, 3])
def test_permuted_rows_give_the_permuted_decisions(dim):
    """The means depend on the multiset of distances alone; the tree sums follow the row order, so mu and sigma may
    move in their last bits -- the reference is asked again, and the kept SET must be the permuted one here, where no
    mean is near the threshold."""
    for name in ("rows_4097_k8", "coincident_k8", "lattice_k8"):
        _, pts, k, ratio = R.case_table(dim)[name]
        keep, mean, (_, _, thr) = R.expected(dim, name)
        perm = np.random.default_rng([5, dim]).permutation(len(pts))
        p2 = np.ascontiguousarray(pts[perm])
        R.check(gicp.sor_points, p2, k, ratio, None, (name, "permuted"))
        _, idx, m2 = gicp.sor_points(p2, k, ratio, return_index=True, return_mean=True)
        assert R.same_bits(m2, np.ascontiguousarray(mean[perm])), name
        if np.abs(mean - thr).min() > 1e-9 * thr:
            assert np.array_equal(np.sort(perm[idx]), np.nonzero(keep)[0]), name


def _ulp_cases():
    return [(dim, name) for dim in (2, 3) for name in R.ulp_cases(dim, True)]


@pytest.mark.parametrize("dim,name", _ulp_cases())
def test_threshold_to_the_ulp(dim, name):
    """Per case: std_ratio = (mean_j - mu) / sigma for a row j above mu, and its two floating-point neighbours.  Device,
    host and reference agree on the kept set in all three runs (the 65 537-row case: device and reference, the host
    function is quadratic), and where a threshold is mean_j itself row j is kept."""
    host = [] if name in dict((c[0], c) for c in R.big_cases(dim)) else [gicp.sor_points_host]
    R.check_ulp(dim, name, [gicp.sor_points] + host, True)


def test_determinism_across_calls_and_engines():
    _, pts, k, ratio = R.case_table(3)["rows_4097_k16"]
    first = gicp.sor_points(pts, k, ratio, return_index=True, return_mean=True)
    e2 = gicp.Engine(0)
    try:
        for _ in range(2):
            again = e2.sor_points(pts, k, ratio, return_index=True, return_mean=True)
            assert all(R.same_bits(x, y) for x, y in zip(first, again))
    finally:
        e2.close()


# ---- 2. fused equals unfused, bit for bit ----------------------------------------------------------------

def _fused(name, how, shard=None):
    f = D.fixture(name)
    p = TF._params(f)
    e = gicp.Engine(0)
    try:
        e.set_sor(*R.CORE_SOR[name])
        if how == "set":
            e.set_target(f["target"], p)
        else:
            e.stage_target(f["target"], p, borrow=how == "borrow")
            e.commit_target()
        e.set_source(f["source"], p, *(shard or ()))
        assert e.n_tgt == int(f["core_target"].sum()) and e.n_src == int(f["core_source"].sum())
        return TF._state(e, f, shard is not None)
    finally:
        e.close()


def _unfused(name, shard=None):
    """A plain engine given the core (test_gpu_filter.py's reference, whose survivors are the same rows)."""
    f = D.fixture(name)
    assert np.array_equal(TF._survivors(name, "source"), f["source"][f["core_source"]])
    return TF._unfused(name, shard)


@pytest.mark.parametrize("name", sorted(R.CORE_SOR))
def test_fused_build_equals_the_core_only_build(name):
    TF._assert_same(_fused(name, "set"), _unfused(name), name)


@pytest.mark.parametrize("how", ["stage", "borrow"])
def test_staged_builds_filter_on_their_own_stream(how):
    TF._assert_same(_fused("stretched_3d", how), _unfused("stretched_3d"), how)


@pytest.mark.parametrize("rank", [0, 1])
def test_two_shards_filter_the_whole_cloud(rank):
    TF._assert_same(_fused("stretched_3d", "set", (rank, 2)), _unfused("stretched_3d", (rank, 2)), ("shard", rank))


def test_a_staged_build_uses_the_setting_in_force_when_staged():
    f = D.fixture("stretched_3d")
    p = TF._params(f)
    e = gicp.Engine(0)
    try:
        e.set_sor(*R.CORE_SOR["stretched_3d"])
        e.stage_target(f["target"], p)
        e.set_sor(None)                                  # off again before the commit
        assert e.sor == (0, 0.0)
        e.commit_target()
        assert np.array_equal(e.points("target"), f["target"][f["core_target"]])
        e.set_target(f["target"], p)
        assert e.n_tgt == len(f["target"])
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _chain():
    """Crop, radius outlier removal, statistical outlier removal and the voxel filter as four one-shots, each fed the
    one before; every stage removes rows."""
    f = D.fixture("stretched_3d")
    out = {}
    for which in ("source", "target"):
        centre = f[which][f["core_" + which]].mean(axis=0)
        x0 = f[which]
        x1 = gicp.filter_points(x0, center=centre, max_range=22.0)
        x2 = gicp.filter_points(x1, radius=0.8, min_neighbors=4)
        x3 = gicp.sor_points(x2, 8, 1.0)
        x4 = gicp.voxel_downsample(x3, 0.25)
        assert len(x0) > len(x1) > len(x2) > len(x3) > len(x4) > 1000, [len(x) for x in (x0, x1, x2, x3, x4)]
        assert R.same_bits(x3, np.ascontiguousarray(x2[R.sor(x2, 8, 1.0)[0]]))
        out[which] = (centre, x3, x4)
    return out


@pytest.mark.parametrize("voxel", [False, True])
def test_stage_order_equals_the_one_shots_chained(voxel):
    f = D.fixture("stretched_3d")
    p = TF._params(f)
    ch = _chain()
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        a.set_sor(8, 1.0)
        if voxel:
            a.set_voxel(0.25)
        for which, build in (("target", a.set_target), ("source", a.set_source)):
            a.set_filter(center=ch[which][0], max_range=22.0, radius=0.8, min_neighbors=4)
            build(f[which], p)
        b.set_target(ch["target"][2 if voxel else 1], p)
        b.set_source(ch["source"][2 if voxel else 1], p)
        for which in ("source", "target"):
            assert R.same_bits(a.points(which), ch[which][2 if voxel else 1]), which
        TF._assert_same(TF._state(a, f), TF._state(b, f), ("chain", voxel))
    finally:
        a.close()
        b.close()


# ---- 3. history independence -----------------------------------------------------------------------------

def test_the_same_bits_after_unrelated_calls_and_on_a_second_context():
    _, pts, k, ratio = R.case_table(3)["rows_4097_k8"]
    f = D.fixture("stretched_3d")
    want = R.expected(3, "rows_4097_k8")
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        R.check(a.sor_points, pts, k, ratio, want, "fresh")
        a.set_sor(*R.CORE_SOR["stretched_3d"])
        a.set_target(f["target"], TF._params(f))
        a.knn_points(K.random_cloud(500, 2, 3), k=5)
        a.sor_points(K.coincident(2), 31, 0.5)
        a.filter_points(f["source"], radius=2.0, min_neighbors=3)
        R.check(a.sor_points, pts, k, ratio, want, "after unrelated calls")
        R.check(b.sor_points, pts, k, ratio, want, "second context")
    finally:
        a.close()
        b.close()


def test_align_does_not_see_one_shot_calls():
    src, tgt, _ = S.scene_pair_3d(4000)
    p = gicp.default_params(3, max_iterations=8, tolerance=1e-9, **P3)
    _, pts, k, ratio = R.case_table(3)["rows_4097_k8"]
    out = []
    for noisy in (False, True):
        e = gicp.Engine(0)
        try:
            if noisy:
                e.sor_points(pts, k, ratio)
            e.set_target(tgt, p)
            if noisy:
                e.sor_points(tgt, 15, 2.0)
            e.set_source(src, p)
            if noisy:
                e.sor_points(K.lattice(3), 6, 1.0)
            T, res = e.align(None, p)
            out.append((T, [res[key] for key in ("iterations", "converged", "correspondences", "pairs_total")],
                        e.covariances("target"), np.array(list(e.pass_info().values()))))
            if noisy:
                R.check(e.sor_points, pts, k, ratio, R.expected(3, "rows_4097_k8"), "after an align")
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


# ---- 4. refusals -----------------------------------------------------------------------------------------

REFUSED = [
    (dict(k=0), "sor: k must be 1..gicp_sor_max_k()"),
    (dict(k=32), "sor: k must be 1..gicp_sor_max_k()"),
    (dict(std_ratio=-0.5), "sor: std_ratio must be finite and >= 0"),
    (dict(std_ratio=np.nan), "sor: std_ratio must be finite and >= 0"),
    (dict(points=np.zeros((1, 3))), "sor: statistical outlier removal needs at least 2 rows"),
    (dict(points=np.array([[0.0, 1.0, np.nan], [0.0, 0.0, 0.0]])), "non-finite"),
    # refused on the host before anything is launched: d2 between the rows overflows
    (dict(points=np.array([[1e200, 0.0, 0.0], [-1e200, 0.0, 0.0], [0.0, 1e200, 0.0]])), "sor: the squared extent of the rows is not finite"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
def test_refusals_carry_the_library_text(kw, text):
    args = dict(points=R.cloud_with_outliers(50, 3, 1), k=4, std_ratio=1.0)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        gicp.sor_points(args["points"], args["k"], args["std_ratio"])
    assert text in str(e.value) and "gicp_sor_points: " in str(e.value)
    e2 = gicp.Engine(0)
    try:
        if "points" not in kw:
            with pytest.raises(ValueError, match="sor: "):
                e2.set_sor(args["k"] if args["k"] else 40, args["std_ratio"])
            assert e2.sor == (0, 0.0)
    finally:
        e2.close()


def test_a_stage_that_leaves_no_row_is_refused_on_the_device():
    """Equal means and a mu that rounds below them (tests/test_sor_cpu.py has the host's side): the device's result
    words say M = 0 and the call is refused."""
    pts = R.empty_stage_cloud()
    with pytest.raises(ValueError, match="sor: statistical outlier removal removed all 3 points"):
        gicp.sor_points(pts, 1, 0.0)


def test_a_too_wide_stage_is_refused_inside_a_build():
    """The extent refusal of a fused build, before the stage launches anything: the cloud is NOT SET."""
    f = D.fixture("stretched_3d")
    wide = np.array(f["target"])
    wide[0, 0], wide[1, 0] = 1e200, -1e200
    e = gicp.Engine(0)
    try:
        e.set_sor(8, 1.0)
        with pytest.raises(ValueError, match="sor: the squared extent of the rows is not finite"):
            e.set_target(wide, TF._params(f))
        assert e.cloud_size("target") == 0
    finally:
        e.close()


@pytest.mark.parametrize("which", ["source", "target"])
def test_a_refused_stage_leaves_the_cloud_not_set(which):
    """A crop that leaves one row, then statistical outlier removal, which needs two: refused after the build began."""
    name = "stretched_3d"
    f = D.fixture(name)
    p = TF._params(f)
    e = gicp.Engine(0)
    try:
        e.set_sor(*R.CORE_SOR[name])
        e.set_target(f["target"], p)
        e.set_source(f["source"], p)
        other = "target" if which == "source" else "source"
        before = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        build = e.set_source if which == "source" else e.set_target
        e.set_filter(center=f[which][5], max_range=1e-9)
        with pytest.raises(ValueError, match="sor: statistical outlier removal needs at least 2 rows"):
            build(f[which], p)
        assert e.cloud_size(which) == 0                       # NOT SET
        with pytest.raises(_lib.GicpError) as ei:
            e.iterate(np.eye(4))
        assert ei.value.code == _lib.GICP_E_STATE
        after = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        assert all(np.array_equal(x, y) for x, y in zip(before, after))   # the other cloud is untouched
        e.set_filter()
        build(f[which], p)                                    # a good rebuild: a fresh context's bits
        TF._assert_same(TF._state(e, f), _unfused(name), which)
        if which == "target":                                 # a staged build that the stage refuses fails the commit
            e.set_filter(center=f[which][5], max_range=1e-9)
            e.stage_target(f["target"], p)
            with pytest.raises(ValueError, match="sor: statistical outlier removal needs at least 2 rows"):
                e.commit_target()
    finally:
        e.close()


# ---- 5. gicp() and Odometry ------------------------------------------------------------------------------

def test_drop_in_with_statistical_outlier_removal():
    f = D.fixture("stretched_3d")
    cs, ct = D.core_only("stretched_3d")
    kw = dict(max_iterations=8, tolerance=1e-9, verbose=False, **D.params_kw(f))
    eng = gicp._engine(0)
    eng.set_sor(3, 7.0)                                 # a setting of the caller's own, to be found again afterwards
    try:
        out = gicp.gicp(f["source"], f["target"], sor_k=8, sor_std_ratio=1.0, **kw)
        assert eng.sor == (3, 7.0)
        eng.set_sor(None)
        ref = gicp.gicp(cs, ct, **kw)
    finally:
        eng.set_sor(None)
    assert out[2].shape == (len(cs), 3, 3) and out[3].shape == (len(ct), 3, 3)
    assert np.array_equal(out[0], ref[0])
    assert len(out[1]) == len(ref[1]) and all(np.array_equal(x, y) for x, y in zip(out[1], ref[1]))
    assert np.array_equal(out[2], ref[2]) and np.array_equal(out[3], ref[3])


@pytest.mark.parametrize("mode", ["scan", "map"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_odometry_with_far_returns_equals_the_clean_stream(mode, how):
    clean, raw = TF._stream()
    for fr, rw in zip(clean, raw):      # the stage removes the 12 appended returns and nothing else
        keep, _, _ = R.sor(rw, 8, 1.0)
        assert np.array_equal(np.nonzero(keep)[0], np.arange(len(fr)))
    kw = dict(map_voxel_size=0.5, map_range=60.0) if mode == "map" else {}
    prm = dict(max_iterations=20, tolerance=1e-9, **P3)
    out = []
    for frames, filt in ((raw, dict(sor_k=8, sor_std_ratio=1.0)), (clean, {})):
        odo = Odometry(3, params=gicp.default_params(3, **prm), **filt, **kw)
        try:
            got = [odo.step(fr)[0] for fr in frames] if how == "step" else [T for T, _ in odo.run(frames, depth=2)]
            assert odo.eng.cloud_size("source") == len(clean[-1 if mode == "map" else -2])
            out.append((got, [P.copy() for P in odo.poses]))
        finally:
            odo.eng.close()
    (ta, pa), (tb, pb) = out
    assert ta[0] is None and tb[0] is None
    assert all(np.array_equal(x, y) for x, y in zip(ta[1:], tb[1:]))
    assert len(pa) == len(pb) == 5 and all(np.array_equal(x, y) for x, y in zip(pa, pb))
