"""Euclidean cluster extraction on the device (gicp_cluster.hip): the one-shot against the NumPy / SciPy
restatement (tests/cluster_ref.py) exactly -- labels, sizes, C, the kept index and rows -- at every size where the
kernels or rocPRIM take another path, on long thin components in every row order, on pairs across every diagonal cell
boundary, at the axis ends and on the widest grid, on coincident and tied inputs, under a permutation of the rows; the
decision; the identity with radius outlier removal's counts; the stage fused into every cloud build against a plain
build of the survivors bit for bit (synchronous, staged, borrowed, sharded, chained with the other filters);
independence of the context's history; refusals; gicp() and Odometry.

On stretched_3d and offset_origin_3d the survivors at radius 3.0, min_size 13 are exactly the core (asserted on the
CPU, tests/test_cluster_cpu.py), so the fused builds must equal the core-only builds of test_gpu_filter.py in every bit."""
import functools

import numpy as np
import pytest

import cluster_ref as R
import density_ref as D
import filter_ref as F
import knn_ref as K
import test_gpu_filter as TF      # the comparison of two engines' states, and the core-only builds it caches

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from gicp.odometry import Odometry  # noqa: E402

pytestmark = pytest.mark.gpu

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)


# ---- 1. the one-shot against the reference ---------------------------------------------------------------

def _cases():
    return [(dim, name) for dim in (2, 3) for name in R.cases(dim)]


@pytest.mark.parametrize("dim,name", _cases())
def test_one_shot_matches_reference(dim, name):
    pts, radius, lo, hi = R.cases(dim)[name]
    R.check(gicp.cluster_points, pts, radius, lo, hi, R.expected(dim, name), name)


@pytest.mark.parametrize("dim", [2, 3])
def test_one_shot_equals_the_host_function(dim):
    for name in ("n257", "n4097", "chain_4097_snake", "diagonal_pairs", "key_runs", "coincident", "widest"):
        pts, radius, lo, hi = R.cases(dim)[name]
        got = gicp.cluster_points(pts, radius, lo, hi, return_index=True, return_labels=True, return_sizes=True)
        want = gicp.cluster_points_host(pts, radius, lo, hi, return_index=True, return_labels=True, return_sizes=True)
        assert all(R.same_bits(x, y) for x, y in zip(got, want)), name


def test_a_long_chain_is_one_pass_like_a_short_one():
    """The device makes one lock-free pass over the edges whatever the diameter (there is no round count to compare):
    the 16 385-row chain in random order comes out as one cluster, as the reference's, within the budget of any test
    here."""
    pts, radius, lo, hi = R.cases(3)["chain_16385"]
    _, labels, sizes = gicp.cluster_points(pts, radius, lo, hi, return_labels=True, return_sizes=True)
    assert list(sizes) == [16385] and not labels.any()


@pytest.mark.parametrize("dim", [2, 3])
def test_the_first_refused_grid(dim):
    """filter_ref.widest: the widest accepted grid is a case above; one more cell on x is refused, naming the axis."""
    with pytest.raises(ValueError, match=r"cluster: radius grid too wide: axis x spans .* cells of edge radius = 1 "):
        gicp.cluster_points(F.widest(dim, extra=1), 1.0)


def test_rounded_difference_two_cells_apart():
    """test_filter_cpu.py's pair whose rounded difference is exactly the radius and whose cells of edge `radius` would
    be two apart: linked, as the definition says."""
    for dim in (2, 3):
        p = np.zeros((3, dim))
        p[0, 0], p[1, 0], p[2, 0] = 1.0 - 2.0 ** -53, 2.0, 50.0
        R.check(gicp.cluster_points, p, 1.0, 1, 0, None, "rounded")
        _, labels = gicp.cluster_points(p, 1.0, return_labels=True)
        assert list(labels) == [0, 0, 1]


@pytest.mark.parametrize("dim", [2, 3])
def test_decision_on_either_side_of_a_size(dim):
    pts, radius, _, _ = R.cases(dim)["n4097"]
    labels, sizes, _ = R.expected(dim, "n4097")
    s = int(np.sort(np.unique(sizes))[len(np.unique(sizes)) // 2])      # an existing size, neither the smallest nor the largest
    for lo, hi in ((s, 0), (s + 1, 0), (1, s), (1, s - 1), (s, s), (2, s), (int(sizes.max()), 0), (1, 1)):
        want = (labels, sizes, R.keeps(sizes, lo, hi)[labels])
        assert want[2].any()
        R.check(gicp.cluster_points, pts, radius, lo, hi, want, (lo, hi))
    with pytest.raises(ValueError, match=r"cluster: none of the \d+ clusters of the 4097 points has a size in"):
        gicp.cluster_points(pts, radius, int(sizes.max()) + 1, 0)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_permutation_permutes_the_partition(dim):
    """Under a row permutation the partition is the permuted one and the numbering follows the new smallest rows."""
    for name in ("n4097", "chain_two", "duplicates"):
        pts, radius, lo, hi = R.cases(dim)[name]
        labels, sizes, _ = R.expected(dim, name)
        perm = np.random.default_rng([7, dim]).permutation(len(pts))
        p2 = np.ascontiguousarray(pts[perm])
        R.check(gicp.cluster_points, p2, radius, lo, hi, None, (name, "permuted"))
        _, l2, s2 = gicp.cluster_points(p2, radius, lo, hi, return_labels=True, return_sizes=True)
        back = np.empty_like(l2)
        back[perm] = l2
        pairs = np.unique(np.stack([labels, back], 1), axis=0)
        assert len(pairs) == len(sizes) == len(s2), name
        assert R.same_bits(s2[pairs[:, 1]], sizes[pairs[:, 0]]), name
        first = np.full(len(s2), len(l2))
        np.minimum.at(first, l2, np.arange(len(l2)))
        assert np.all(np.diff(first) > 0), name


@pytest.mark.parametrize("dim", [2, 3])
def test_singletons_are_the_rows_radius_outlier_removal_counts_zero(dim):
    for name in ("n4097", "n65537", "key_runs", "duplicates", "diagonal_pairs"):
        pts, radius, _, _ = R.cases(dim)[name]
        _, labels, sizes = gicp.cluster_points(pts, radius, return_labels=True, return_sizes=True)
        _, counts = gicp.filter_points(pts, radius=radius, min_neighbors=1, return_counts=True)
        assert np.array_equal(counts == 0, sizes[labels] == 1), name


def test_determinism_across_calls_and_engines():
    e2 = gicp.Engine(0)
    try:
        for dim, name in ((3, "n65537"), (2, "n16385"), (3, "chain_4097_random")):
            pts, radius, lo, hi = R.cases(dim)[name]
            kw = dict(return_index=True, return_labels=True, return_sizes=True)
            first = gicp.cluster_points(pts, radius, lo, hi, **kw)
            for _ in range(2):
                again = e2.cluster_points(pts, radius, lo, hi, **kw)
                assert all(R.same_bits(x, y) for x, y in zip(first, again)), name
            assert all(R.same_bits(x, y) for x, y in zip(first, gicp.cluster_points(pts, radius, lo, hi, **kw))), name
    finally:
        e2.close()


# ---- 2. fused equals unfused, bit for bit ----------------------------------------------------------------

def _fused(name, how, shard=None):
    f = D.fixture(name)
    p = TF._params(f)
    e = gicp.Engine(0)
    try:
        e.set_cluster(*R.CORE_CLUSTER[name])
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


@pytest.mark.parametrize("name", sorted(R.CORE_CLUSTER))
def test_fused_build_equals_the_core_only_build(name):
    """Points, covariances, neighbour counts, graph, eight passes' statistics and pass_info, align."""
    TF._assert_same(_fused(name, "set"), _unfused(name), name)


@pytest.mark.parametrize("how", ["stage", "borrow"])
def test_staged_builds_filter_on_their_own_stream(how):
    TF._assert_same(_fused("stretched_3d", how), _unfused("stretched_3d"), how)


@pytest.mark.parametrize("rank", [0, 1])
def test_two_shards_filter_the_whole_cloud(rank):
    TF._assert_same(_fused("offset_origin_3d", "set", (rank, 2)), _unfused("offset_origin_3d", (rank, 2)), ("shard", rank))


def test_a_staged_build_uses_the_setting_in_force_when_staged_and_off_is_the_plain_build():
    f = D.fixture("stretched_3d")
    p = TF._params(f)
    e = gicp.Engine(0)
    try:
        e.set_cluster(*R.CORE_CLUSTER["stretched_3d"])
        assert e.cluster == R.CORE_CLUSTER["stretched_3d"]
        e.stage_target(f["target"], p)
        e.set_cluster(None)                              # off again before the commit
        assert e.cluster == (0.0, 1, 0)
        e.commit_target()
        assert np.array_equal(e.points("target"), f["target"][f["core_target"]])
        e.set_target(f["target"], p)                     # off: the plain build, every row
        assert e.n_tgt == len(f["target"]) and np.array_equal(e.points("target"), f["target"])
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def _chain():
    """Crop, radius outlier removal, statistical outlier removal, cluster extraction and the voxel filter as five
    one-shots, each fed the one before; every stage removes rows."""
    f = D.fixture("stretched_3d")
    out = {}
    for which in ("source", "target"):
        centre = f[which][f["core_" + which]].mean(axis=0)
        x0 = f[which]
        x1 = gicp.filter_points(x0, center=centre, max_range=22.0)
        x2 = gicp.filter_points(x1, radius=0.8, min_neighbors=4)
        x3 = gicp.sor_points(x2, 8, 1.0)
        x4 = gicp.cluster_points(x3, 1.0, 5, 0)
        x5 = gicp.voxel_downsample(x4, 0.25)
        assert len(x0) > len(x1) > len(x2) > len(x3) > len(x4) > len(x5) > 1000, [len(x) for x in (x0, x1, x2, x3, x4, x5)]
        assert R.same_bits(x4, np.ascontiguousarray(x3[R.cluster(x3, 1.0, 5, 0)[2]]))
        out[which] = (centre, x4, x5)
    return out


@pytest.mark.parametrize("voxel", [False, True])
def test_stage_order_equals_the_one_shots_chained(voxel):
    """After crop + ROR + SOR and before the voxel filter."""
    f = D.fixture("stretched_3d")
    p = TF._params(f)
    ch = _chain()
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        a.set_sor(8, 1.0)
        a.set_cluster(1.0, 5, 0)
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

def test_the_same_result_after_unrelated_calls_and_on_a_second_context():
    pts, radius, lo, hi = R.cases(3)["n4097"]
    want = R.expected(3, "n4097")
    f = D.fixture("stretched_3d")
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        R.check(a.cluster_points, pts, radius, lo, hi, want, "fresh")
        a.set_cluster(*R.CORE_CLUSTER["stretched_3d"])
        a.set_target(f["target"], TF._params(f))
        a.knn_points(K.random_cloud(500, 2, 3), k=5)
        a.cluster_points(R.cases(2)["chain_16385"][0], R.STEP)          # a larger cloud of another dimension
        a.sor_points(K.coincident(2), 31, 0.5)
        a.filter_points(f["source"], radius=2.0, min_neighbors=3)
        R.check(a.cluster_points, pts, radius, lo, hi, want, "after unrelated calls")
        R.check(b.cluster_points, pts, radius, lo, hi, want, "second context")
        assert a.cluster == R.CORE_CLUSTER["stretched_3d"]              # the one-shot leaves the setting alone
    finally:
        a.close()
        b.close()


def test_align_does_not_see_one_shot_calls():
    src, tgt, _ = S.scene_pair_3d(4000)
    p = gicp.default_params(3, max_iterations=8, tolerance=1e-9, **P3)
    pts, radius, lo, hi = R.cases(3)["n4097"]
    out = []
    for noisy in (False, True):
        e = gicp.Engine(0)
        try:
            if noisy:
                e.cluster_points(pts, radius, lo, hi)
            e.set_target(tgt, p)
            if noisy:
                e.cluster_points(tgt, 0.3)
            e.set_source(src, p)
            if noisy:
                e.cluster_points(K.lattice(3), 1.0)
            T, res = e.align(None, p)
            out.append((T, [res[key] for key in ("iterations", "converged", "correspondences", "pairs_total")],
                        e.covariances("target"), np.array(list(e.pass_info().values()))))
            if noisy:
                R.check(e.cluster_points, pts, radius, lo, hi, R.expected(3, "n4097"), "after an align")
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


# ---- 4. refusals -----------------------------------------------------------------------------------------

REFUSED = [
    (dict(radius=0.0), "cluster: radius must be finite and > 0"),
    (dict(radius=-1.0), "cluster: radius must be finite and > 0"),
    (dict(radius=np.nan), "cluster: radius must be finite and > 0"),
    (dict(min_size=0), "cluster: min_size must be >= 1"),
    (dict(min_size=5, max_size=4), "cluster: max_size 4 must be 0 (no upper limit) or at least min_size 5"),
    (dict(points=np.array([[0.0, 1.0, np.nan], [0.0, 0.0, 0.0]])), "cluster: cloud contains non-finite coordinates"),
    (dict(points=np.array([[0.0, 0.0, 0.0], [0.0, 3e6, 0.0]])), "cluster: radius grid too wide: axis y spans"),
    (dict(points=np.array([[1e12, 0.0, 0.0], [1e12, 1.0, 0.0]])), "cluster: axis x lies beyond 2^35 cells of edge radius = 1"),
    (dict(min_size=60), "cluster: none of the"),
]


@pytest.mark.parametrize("kw,text", REFUSED)
def test_refusals_carry_the_library_text(kw, text):
    args = dict(points=R.mix_cloud(50, 3), radius=1.0, min_size=1, max_size=0)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        gicp.cluster_points(args["points"], args["radius"], args["min_size"], args["max_size"])
    assert "gicp_cluster_points: " + text in str(e.value), str(e.value)      # (the entry point's name, then the library's text)
    e2 = gicp.Engine(0)
    try:
        if "points" not in kw and "none of" not in text:      # what the setting alone decides, gicp_set_cluster refuses too
            with pytest.raises(ValueError, match="cluster: "):
                e2.set_cluster(args["radius"] if args["radius"] else -2.0, args["min_size"], args["max_size"])
            assert e2.cluster == (0.0, 1, 0)       # a refused setting changes nothing
    finally:
        e2.close()


def test_a_refused_call_writes_nothing():
    import ctypes as C
    e = gicp.Engine(0)
    try:
        pts = R.mix_cloud(20, 3)
        c = _lib.Cluster(1.0, 21, 0)               # nothing is kept: refused after the device has run
        out = np.full((20, 3), 7.5)
        idx = np.full(20, 77, dtype=np.int64)
        labels = np.full(20, 77, dtype=np.int32)
        sizes = np.full(20, 77, dtype=np.int32)
        m, nc = C.c_int64(5), C.c_int64(5)
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        rc = e._lib.gicp_cluster_points(e._ctx, _lib.dptr(pts), 20, 3, C.byref(c), labels.ctypes.data_as(i32),
                                        sizes.ctypes.data_as(i32), C.byref(nc), _lib.dptr(out), idx.ctypes.data_as(i64), C.byref(m))
        assert rc == _lib.GICP_E_INVALID
        assert np.all(out == 7.5) and np.all(idx == 77) and np.all(labels == 77) and np.all(sizes == 77)
        assert m.value == 5 and nc.value == 5
    finally:
        e.close()


@pytest.mark.parametrize("which", ["source", "target"])
def test_a_refused_stage_leaves_the_cloud_not_set(which):
    """A min_size no cluster reaches: refused after the build began."""
    name = "stretched_3d"
    f = D.fixture(name)
    p = TF._params(f)
    e = gicp.Engine(0)
    try:
        e.set_cluster(*R.CORE_CLUSTER[name])
        e.set_target(f["target"], p)
        e.set_source(f["source"], p)
        other = "target" if which == "source" else "source"
        before = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        build = e.set_source if which == "source" else e.set_target
        e.set_cluster(3.0, 9000)
        with pytest.raises(ValueError, match="cluster: none of the 13 clusters of the 8012 points has a size in"):
            build(f[which], p)
        assert e.cloud_size(which) == 0                       # NOT SET
        with pytest.raises(_lib.GicpError) as ei:
            e.iterate(np.eye(4))
        assert ei.value.code == _lib.GICP_E_STATE
        after = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        assert all(np.array_equal(x, y) for x, y in zip(before, after))   # the other cloud is untouched
        if which == "target":                                 # a staged build that the stage refuses fails the commit
            e.stage_target(f["target"], p)
            with pytest.raises(ValueError, match="cluster: none of the 13 clusters"):
                e.commit_target()
        e.set_cluster(*R.CORE_CLUSTER[name])
        build(f[which], p)                                    # a good rebuild: a fresh context's bits
        TF._assert_same(TF._state(e, f), _unfused(name), which)
    finally:
        e.close()


# ---- 5. gicp() and Odometry ------------------------------------------------------------------------------

def test_drop_in_with_cluster_extraction():
    f = D.fixture("offset_origin_3d")
    cs, ct = D.core_only("offset_origin_3d")
    kw = dict(max_iterations=8, tolerance=1e-9, verbose=False, **D.params_kw(f))
    eng = gicp._engine(0)
    eng.set_cluster(0.7, 3, 50)                         # a setting of the caller's own, to be found again afterwards
    try:
        out = gicp.gicp(f["source"], f["target"], cluster_radius=3.0, cluster_min_size=13, **kw)
        assert eng.cluster == (0.7, 3, 50)
        eng.set_cluster(None)
        ref = gicp.gicp(cs, ct, **kw)
    finally:
        eng.set_cluster(None)
    assert out[2].shape == (len(cs), 3, 3) and out[3].shape == (len(ct), 3, 3)
    assert np.array_equal(out[0], ref[0])
    assert len(out[1]) == len(ref[1]) and all(np.array_equal(x, y) for x, y in zip(out[1], ref[1]))
    assert np.array_equal(out[2], ref[2]) and np.array_equal(out[3], ref[3])


@functools.lru_cache(maxsize=None)
def _filtered_stream():
    """test_gpu_filter.py's raw stream (12 far returns appended to every frame) and what cluster extraction at
    radius 2.0, min_size 13 leaves of each frame, by the reference."""
    _, raw = TF._stream()
    kept = []
    for rw in raw:
        _, sizes, keep = R.cluster(rw, 2.0, 13, 0)
        assert not keep[-12:].any() and keep.sum() > 0.9 * len(rw)      # the far returns go, nearly all else stays
        kept.append(np.ascontiguousarray(rw[keep]))
    return raw, kept


@pytest.mark.parametrize("mode", ["scan", "map"])
def test_odometry_with_cluster_extraction_equals_the_prefiltered_stream(mode):
    raw, kept = _filtered_stream()
    kw = dict(map_voxel_size=0.5, map_range=60.0) if mode == "map" else {}
    prm = dict(max_iterations=20, tolerance=1e-9, **P3)
    out = []
    for frames, filt in ((raw, dict(cluster_radius=2.0, cluster_min_size=13)), (kept, {})):
        odo = Odometry(3, params=gicp.default_params(3, **prm), **filt, **kw)
        try:
            got = [odo.step(fr)[0] for fr in frames]
            assert odo.eng.cloud_size("source") == len(kept[-1 if mode == "map" else -2])
            out.append((got, [P.copy() for P in odo.poses]))
        finally:
            odo.eng.close()
    (ta, pa), (tb, pb) = out
    assert ta[0] is None and tb[0] is None
    assert all(np.array_equal(x, y) for x, y in zip(ta[1:], tb[1:]))
    assert len(pa) == len(pb) == 5 and all(np.array_equal(x, y) for x, y in zip(pa, pb))
