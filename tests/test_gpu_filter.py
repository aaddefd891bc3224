"""Input filters on the device (gicp_filter.hip): the one-shot against the NumPy reference
(tests/filter_ref.py) bit for bit, determinism, the filters fused into every cloud build against a plain build of the
reference's survivors bit for bit, errors and recovery, gicp() and Odometry.

On the clouds of uneven density (tests/density_ref.py) the survivors are exactly the core (asserted on the CPU,
tests/test_filter_cpu.py), so the fused builds must equal the core-only builds in every bit, the pairs pass 0
screens included: the collapsed grid's cost is shown to be gone by equality, not by a ratio."""
import functools

import numpy as np
import pytest

import density_ref as D
import filter_ref as F

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402
from gicp.odometry import Odometry  # noqa: E402

pytestmark = pytest.mark.gpu

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)


# ---- 1. the one-shot against the reference ---------------------------------------------------------------

@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", sorted(F.cases(3)))
def test_one_shot_matches_reference(dim, name):
    F.check_against_reference(gicp.filter_points, dim, name)


@pytest.mark.parametrize("dim", [2, 3])
def test_one_shot_equals_the_host_function(dim):
    for name in ("key_runs", "n257", "lattice_345_ror"):
        pts, kw, _, _ = F.reference(dim, name)
        got = gicp.filter_points(pts, return_index=True, return_counts=True, **kw)
        want = gicp.filter_points_host(pts, return_index=True, return_counts=True, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), name


def test_identity_and_rounded_difference():
    pts = np.random.default_rng(2).normal(size=(300, 3))
    rows, idx, cnt = gicp.filter_points(pts, return_index=True, return_counts=True)
    assert rows.tobytes() == pts.tobytes() and np.array_equal(idx, np.arange(300)) and np.all(cnt == 0)
    # test_filter_cpu.py test_rounded_difference_two_cells_apart, on the device
    for dim in (2, 3):
        p = np.zeros((3, dim))
        p[0, 0], p[1, 0], p[2, 0] = 1.0 - 2.0 ** -53, 2.0, 50.0
        _, idx, cnt = gicp.filter_points(p, radius=1.0, min_neighbors=1, return_index=True, return_counts=True)
        assert list(idx) == [0, 1] and list(cnt) == [1, 1, 0]


@pytest.mark.parametrize("dim", [2, 3])
def test_widest_span_is_taken_and_the_next_refused(dim):
    pts = F.widest(dim, extra=1)
    with pytest.raises(ValueError, match=r"axis x spans .* cells of edge radius = 1 .*max_range"):
        gicp.filter_points(pts, radius=1.0, min_neighbors=1)
    far = pts[np.argmax(pts[:, 0])]
    keep, _ = F.filter_ref(pts, center=far, min_range=0.5, radius=1.0, min_neighbors=1)
    rows = gicp.filter_points(pts, center=far, min_range=0.5, radius=1.0, min_neighbors=1)
    assert rows.tobytes() == pts[keep].tobytes()


def test_refusals_carry_the_library_text():
    pts = np.random.default_rng(4).uniform(-2.0, 2.0, (50, 3))
    with pytest.raises(ValueError, match="the range crop removed all 50 points"):
        gicp.filter_points(pts, min_range=100.0)
    with pytest.raises(ValueError, match="radius outlier removal removed all"):
        gicp.filter_points(pts, max_range=2.0, radius=0.01)
    bad = pts.copy()
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        gicp.filter_points(bad, max_range=1.0)
    e = gicp.Engine(0)
    try:
        for kw, text in (((dict(min_range=-1.0)), "must be >= 0"), (dict(min_range=3.0, max_range=2.0), "exceeds max_range"),
                         (dict(radius=1.0, min_neighbors=0), "min_neighbors must be >= 1"),
                         (dict(max_range=float("nan")), "must be finite")):
            with pytest.raises(ValueError, match=text):
                e.set_filter(**kw)
            assert e.filter == gicp._NO_FILTER       # a refused setting changes nothing
    finally:
        e.close()


# ---- 2. determinism --------------------------------------------------------------------------------------

def test_determinism_across_calls_and_engines():
    e2 = gicp.Engine(0)
    try:
        for dim in (2, 3):
            for name in ("dense_cell", "n4097"):
                pts, kw, _, _ = F.reference(dim, name)
                a = gicp.filter_points(pts, return_index=True, return_counts=True, **kw)
                b = gicp.filter_points(pts, return_index=True, return_counts=True, **kw)
                c = e2.filter_points(pts, return_index=True, return_counts=True, **kw)
                assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(a, b, c))
    finally:
        e2.close()


# ---- 3. fused equals unfused, bit for bit ----------------------------------------------------------------

# the filter that keeps exactly core_only(name) (tests/test_filter_cpu.py asserts it)
CORE_FILTER = {"stretched_3d": dict(radius=2.0, min_neighbors=3), "halo_3d": dict(radius=2.0, min_neighbors=3),
               "stretched_2d": dict(radius=20.0, min_neighbors=2), "offset_origin_3d": dict(min_range=10.0)}


def _params(f, **kw):
    return gicp.default_params(f["dim"], **D.params_kw(f), **kw)


def _state(e, f, shard=False):
    """Everything the comparison covers, read from an engine with both clouds set: the clouds, the graph, eight
    passes along the moving poses (statistics, per-point outputs of the first, pass_info), one align."""
    out = {}
    for which in ("target", "source"):
        out[which] = (e.points(which), e.covariances(which), e.neighbor_counts(which))
    out["graph"] = e.graph()
    out["passes"] = []
    for k, T in enumerate(D.moving_poses(f)):
        st, dbg = e.iterate(T, debug=True)
        out["passes"].append((st, dbg if k == 0 else None, np.array(list(e.pass_info().values()))))
    if not shard:      # (a sharded source reduces its shard only: the align is the whole source's)
        T, res = e.align(None, _params(f, max_iterations=6, tolerance=1e-9))
        out["align"] = (T, [res[k] for k in ("iterations", "converged", "correspondences", "ambiguous", "pairs_total")])
    return out


def _assert_same(a, b, what):
    for which in ("target", "source"):
        for x, y, part in zip(a[which], b[which], ("points", "covariances", "neighbor_counts")):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (what, which, part)
    assert np.array_equal(a["graph"][0], b["graph"][0]) and np.array_equal(a["graph"][1], b["graph"][1]), (what, "graph")
    assert a["passes"][0][0][-1] > 0, (what, "no correspondences")
    for k, ((sa, da, ia), (sb, db, ib)) in enumerate(zip(a["passes"], b["passes"])):
        assert np.array_equal(sa, sb), (what, k, "statistics")
        assert np.array_equal(ia, ib), (what, k, "pass_info", ia, ib)      # [1]: the pairs screened
        if da is not None:
            own = ~np.isnan(a["source"][1][:, 0, 0])      # (a sharded source writes its own tiles' rows only)
            for key in da:
                assert np.array_equal(da[key][own], db[key][own]), (what, key)
    if "align" in a:
        assert np.array_equal(a["align"][0], b["align"][0]) and a["align"][1] == b["align"][1], (what, a["align"][1], b["align"][1])


@functools.lru_cache(maxsize=None)
def _survivors(name, which):
    """filter_ref's survivors of the fixture's cloud under CORE_FILTER: the core, rows in their order."""
    f = D.fixture(name)
    keep, _ = F.filter_ref(f[which], **CORE_FILTER[name])
    assert np.array_equal(keep, f["core_" + which])
    out = np.ascontiguousarray(f[which][keep])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _unfused(name, shard=None):
    """The reference: a plain engine given the survivors."""
    f = D.fixture(name)
    p = _params(f)
    e = gicp.Engine(0)
    try:
        e.set_target(_survivors(name, "target"), p)
        e.set_source(_survivors(name, "source"), p, *(shard or ()))
        return _state(e, f, shard is not None)
    finally:
        e.close()


def _fused(name, how, shard=None):
    f = D.fixture(name)
    p = _params(f)
    e = gicp.Engine(0)
    try:
        e.set_filter(**CORE_FILTER[name])
        if how == "set":
            e.set_target(f["target"], p)
        else:
            e.stage_target(f["target"], p, borrow=how == "borrow")
            e.commit_target()
        e.set_source(f["source"], p, *(shard or ()))
        assert e.n_tgt == len(_survivors(name, "target")) and e.n_src == len(_survivors(name, "source"))
        return _state(e, f, shard is not None)
    finally:
        e.close()


@pytest.mark.parametrize("name", sorted(CORE_FILTER))
def test_fused_build_equals_the_core_only_build(name):
    _assert_same(_fused(name, "set"), _unfused(name), name)


@pytest.mark.parametrize("how", ["stage", "borrow"])
def test_staged_builds_filter_on_their_own_stream(how):
    _assert_same(_fused("stretched_3d", how), _unfused("stretched_3d"), how)


def test_a_staged_build_uses_the_setting_in_force_when_staged():
    f = D.fixture("stretched_3d")
    p = _params(f)
    e = gicp.Engine(0)
    try:
        e.set_filter(**CORE_FILTER["stretched_3d"])
        e.stage_target(f["target"], p)
        e.set_filter()                                   # off again before the commit
        e.commit_target()
        assert e.n_tgt == len(_survivors("stretched_3d", "target"))
        assert np.array_equal(e.points("target"), _survivors("stretched_3d", "target"))
        e.set_target(f["target"], p)
        assert e.n_tgt == len(f["target"])
    finally:
        e.close()


def test_pass_info_of_a_fresh_engine_does_not_depend_on_earlier_engines():
    """The comparisons above need it: the first pass after a cloud change reads slot 0 of the pose ring as the last
    pass's pose, and until k_reset_tiles zeroed that slot the lists' first skin, and with it the rebuilds and pairs
    of later passes, came from whatever an earlier engine had left in the memory."""
    f = D.fixture("halo_3d")
    p = _params(f)
    seen = []
    for k in range(3):
        e = gicp.Engine(0)
        try:
            e.set_target(_survivors("halo_3d", "target"), p)
            e.set_source(_survivors("halo_3d", "source"), p)
            if k == 1:      # a long registration: pass 64 writes slot 0 of the ring, the next cloud change resets it
                e.align(None, _params(f, max_iterations=70, tolerance=0.0))
                e.set_source(_survivors("halo_3d", "source"), p)
            info = []
            for T in D.moving_poses(f):
                e.iterate(T)
                info.append(list(e.pass_info().values()))
            seen.append(np.array(info))
        finally:
            e.close()
    assert np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])


@pytest.mark.parametrize("rank", [0, 1])
def test_two_shards_filter_the_whole_cloud(rank):
    _assert_same(_fused("stretched_3d", "set", (rank, 2)), _unfused("stretched_3d", (rank, 2)), ("shard", rank))


def test_fused_with_the_voxel_filter():
    """Crop, then radius outlier removal, then the voxel filter: the reference is the voxel filter of the
    survivors, compared as test_gpu_voxel.py compares fused to unfused."""
    name, leaf = "stretched_3d", 0.25
    f = D.fixture(name)
    p = _params(f)
    vs, vt = gicp.voxel_downsample(_survivors(name, "source"), leaf), gicp.voxel_downsample(_survivors(name, "target"), leaf)
    assert len(vs) < len(_survivors(name, "source"))
    with pytest.raises(ValueError, match="voxel grid too wide"):       # what the caller got without the input filter
        gicp.voxel_downsample(f["source"], 0.01)
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        a.set_filter(**CORE_FILTER[name])
        a.set_voxel(leaf)
        a.set_target(f["target"], p)
        a.set_source(f["source"], p)
        b.set_target(vt, p)
        b.set_source(vs, p)
        assert np.array_equal(a.points("source"), vs) and np.array_equal(a.points("target"), vt)
        _assert_same(_state(a, f), _state(b, f), "voxel")
    finally:
        a.close()
        b.close()


def test_sweep_builds_filter_the_deskewed_rows():
    """The crop centre and the radius act on the de-skewed rows: the reference filters the host-de-skewed rows (the
    device's de-skew decides the same mask: no decision is within rounding of its bound) and a plain engine gets
    the device-de-skewed survivors."""
    name = "stretched_3d"
    f = D.fixture(name)
    p = _params(f)
    # a typical sweep: 0.5 m and 2 degrees over the stamp unit, 360 distinct stamps in [0, 1)
    M, ref = S.se3_exp(np.array([0.007, -0.0035, 0.034, 0.3, -0.2, 0.35])), 0.5
    filt = dict(max_range=200.0, center=f["source"][f["core_source"]].mean(axis=0), **CORE_FILTER[name])
    clouds = {}
    for k, which in enumerate(("source", "target")):
        st = np.random.default_rng(1 + k).integers(0, 360, len(f[which])) / 360.0
        host = gicp.deskew_host(f[which], st, M, ref)
        dev = gicp.deskew(f[which], st, M, ref)
        keep, _ = F.filter_ref(host, **filt)
        assert np.array_equal(keep, F.filter_ref(dev, **filt)[0])
        assert keep.sum() > 0 and not keep[~f["core_" + which]].any()
        clouds[which] = (st, np.ascontiguousarray(dev[keep]))
    b = gicp.Engine(0)
    try:
        b.set_target(clouds["target"][1], p)
        b.set_source(clouds["source"][1], p)
        want = _state(b, f)
    finally:
        b.close()
    for how in ("set", "stage", "borrow"):
        a = gicp.Engine(0)
        try:
            a.set_filter(**filt)
            kw = dict(stamps=clouds["target"][0], motion=M, ref=ref)
            if how == "set":
                a.set_target(f["target"], p, **kw)
            else:
                a.stage_target(f["target"], p, borrow=how == "borrow", **kw)
                a.commit_target()
            a.set_source(f["source"], p, stamps=clouds["source"][0], motion=M, ref=ref)
            _assert_same(_state(a, f), want, ("sweep", how))
        finally:
            a.close()


# ---- 4. errors and recovery ------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["source", "target"])
@pytest.mark.parametrize("fault", ["crop_empty", "ror_empty", "too_wide"])
def test_a_refused_filter_leaves_the_cloud_not_set(which, fault):
    name = "stretched_3d"
    f = D.fixture(name)
    p = _params(f)
    bad, text = {"crop_empty": (dict(min_range=1e7), "the range crop removed all"),
                 "ror_empty": (dict(radius=1e-3, max_range=30.0, center=f[which][f["core_" + which]].mean(axis=0)),
                               "radius outlier removal removed all"),
                 "too_wide": (dict(radius=0.05), "radius grid too wide: axis x")}[fault]
    e = gicp.Engine(0)
    try:
        e.set_filter(**CORE_FILTER[name])
        e.set_target(f["target"], p)
        e.set_source(f["source"], p)
        other = "target" if which == "source" else "source"
        before = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        build = e.set_source if which == "source" else e.set_target
        e.set_filter(**bad)
        with pytest.raises(ValueError, match=text):
            build(f[which], p)
        assert e.cloud_size(which) == 0                       # NOT SET
        with pytest.raises(_lib.GicpError) as ei:
            e.iterate(np.eye(4))
        assert ei.value.code == _lib.GICP_E_STATE
        after = (e.points(other), e.covariances(other), e.neighbor_counts(other))
        assert all(np.array_equal(x, y) for x, y in zip(before, after))   # the other cloud is untouched
        e.set_filter(**CORE_FILTER[name])
        build(f[which], p)                                    # a good rebuild: a fresh context's bits
        _assert_same(_state(e, f), _unfused(name), (which, fault))
        if which == "target":                                 # a staged build that its filter refuses fails the commit
            e.set_filter(**bad)
            e.stage_target(f["target"], p)
            with pytest.raises(ValueError, match=text):
                e.commit_target()
    finally:
        e.close()


# ---- 5. gicp() and Odometry ------------------------------------------------------------------------------

def test_drop_in_with_the_outlier_filter():
    f = D.fixture("stretched_3d")
    cs, ct = D.core_only("stretched_3d")
    kw = dict(max_iterations=8, tolerance=1e-9, verbose=False, **D.params_kw(f))
    eng = gicp._engine(0)
    eng.set_filter(max_range=1e6)                       # a setting of the caller's own, to be found again afterwards
    mine = dict(eng.filter)
    try:
        out = gicp.gicp(f["source"], f["target"], outlier_radius=2.0, outlier_min_neighbors=3, **kw)
        assert eng.filter == mine
        eng.set_filter()
        ref = gicp.gicp(cs, ct, **kw)
    finally:
        eng.set_filter()
    assert out[2].shape == (len(cs), 3, 3) and out[3].shape == (len(ct), 3, 3)
    assert np.array_equal(out[0], ref[0])
    assert len(out[1]) == len(ref[1]) and all(np.array_equal(x, y) for x, y in zip(out[1], ref[1]))
    assert np.array_equal(out[2], ref[2]) and np.array_equal(out[3], ref[3])
    for k in (4, 5):
        assert len(out[k]) == len(ref[k]) and all(np.array_equal(x, y) for x, y in zip(out[k], ref[k]))
    assert len(out[6]) == len(ref[6]) and all(np.array_equal(out[6][k], ref[6][k]) for k in range(len(ref[6])))


@functools.lru_cache(maxsize=None)
def _stream():
    """Five 32 x 250 frames, and the same frames with 12 max-range returns appended to each."""
    clean = [np.ascontiguousarray(fr) for fr, _ in S.lidar_stream(5, beams=32, azimuths=250)]
    rng = np.random.default_rng(23)
    raw = []
    for fr in clean:
        d = rng.normal(size=(12, 3))
        raw.append(np.concatenate([fr, 1e5 * d / np.linalg.norm(d, axis=1, keepdims=True)]))
        assert np.linalg.norm(fr, axis=1).max() < 100.0
    return clean, raw


@pytest.mark.parametrize("mode", ["scan", "map"])
@pytest.mark.parametrize("how", ["step", "run"])
def test_odometry_with_max_range_equals_the_clean_stream(mode, how):
    clean, raw = _stream()
    kw = dict(map_voxel_size=0.5, map_range=60.0) if mode == "map" else {}
    prm = dict(max_iterations=20, tolerance=1e-9, **P3)
    out = []
    for frames, filt in ((raw, dict(max_range=100.0)), (clean, {})):
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
