"""GPU parity on clouds of uneven density and outlier-stretched extent (tests/density_ref.py, whose CPU
preconditions test_density_ref_cpu.py holds): a Morton grid collapsed onto one cell by a dozen far points, a
screen margin dominated by the largest tile radius of a sparse halo, and the range-dependent density of a
spinning-LiDAR frame.  Builds, passes along a moving pose, every acceleration switched off, shards, the whole
loop and the fused voxel filter, each against the oracle (cKDTree, fp64) or bit for bit against the plain path."""
import numpy as np
import pytest

import density_ref as D
import gpu_helpers as G
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402


def params(f, **kw):
    return gicp.default_params(f["dim"], **{**D.params_kw(f), **kw})


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


# ============================================================================= builds
@pytest.mark.parametrize("which", ["target", "source"])
@pytest.mark.parametrize("name", D.FIXTURES)
def test_builds(eng, name, which):
    """Each fixture cloud through both builds: as the target (with the neighbour graph) and as the source.
    Counts exactly the oracle's, covariances by the criteria of G.check_covariances with the cloud's own
    left-out count (density_ref.LEFT_OUT), graph rows that cover their radius on every row (brute force), and
    points with fewer than min_neighbors neighbours -- every far point of the stretched clouds -- the identity
    exactly."""
    f = D.fixture(name)
    pts, p = f[which], params(f)
    left = D.max_left_out(name, which)
    eng.set_target(pts, p)
    rep = G.check_covariances(eng, pts, f["d_n"], "target", max_left_out=left)
    idx, rad = eng.graph()
    G.graph_rows_cover_their_radius(pts, idx, rad)
    eng.set_source(pts, p)
    G.check_covariances(eng, pts, f["d_n"], "source", max_left_out=left)
    assert rep["surface"].mean() >= 0.30
    if name in ("stretched_3d", "stretched_2d"):
        extra = ~f["core_" + which]
        for cloud in ("target", "source"):
            assert np.all(eng.neighbor_counts(cloud)[extra] == 1)
            assert np.all(eng.covariances(cloud)[extra] == np.eye(f["dim"]))


# ============================================================================= passes along the moving sequence
# The distance of check_pass is compared with coord_atol, its allowance for the rounding of R s + t itself: every
# pose of the sequence but the first turns the cloud, and the moved point is then known to an ulp of its
# coordinate to the oracle as to the kernel -- 9e-10 m at 5.4e6 m from the origin (offset_origin_3d), 1e-13 px at
# 1000 px (stretched_2d), 7e-15 m at the 34 m of a LiDAR range -- which rtol 1e-12 of a distance of millimetres
# does not allow.  Measured on an MI355X with rtol alone: lidar_small at pose 7, 6 of 6796 distances differ by at
# most 5.9e-15 m (0.8 ulp of a 32 m coordinate, 1.5e-12 of the distance), every index equal; the allowance there
# is 6 sqrt(3) 2^-53 max(|R||s| + |t|), about 4e-14 m.
PASS_CASES = [(name, "plane_to_plane") for name in D.FIXTURES] + [("stretched_3d", "point_to_point"),
                                                                  ("stretched_3d", "point_to_plane")]


@pytest.mark.parametrize("name,model", PASS_CASES, ids=[f"{n}-{m}" for n, m in PASS_CASES])
def test_passes_along_the_moving_sequence(monkeypatch, name, model):
    """G.check_pass at each of the 8 poses of density_ref.moving_poses on ONE warm engine under the library's
    own defaults: certificates, lists and the graph descent carry over from pose to pose.  Indices bit-exact
    against cKDTree, W and statistics to 1e-9, at every pose the share of accepted points the CPU preconditions
    found."""
    f = D.fixture(name)
    src, tgt = f["source"], f["target"]
    p = params(f, cov_model=_lib.COV_MODELS[model])
    e = G.make_engine(monkeypatch, **{G.LIBRARY: "1"})
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        for k, T in enumerate(D.moving_poses(f)):
            _, idx = G.check_pass(e, src, tgt, T, f["d_c"], model=model, what=f"{name} {model} pose {k}",
                                  coord_atol=True)
            assert 0.25 <= np.mean(idx >= 0) <= 0.95, (k, np.mean(idx >= 0))
            info = e.pass_info()
            print(f"{name} {model} pose {k}: accepted {np.mean(idx >= 0):.3f} pairs {info['pairs']:.0f} ambiguous "
                  f"{info['ambiguous']:.0f} graph-proved {info['graph_proved']:.0f} walked tiles {info['walked_tiles']:.0f}")
    finally:
        e.close()


# ============================================================================= accelerations change nothing
SWITCHED = ("plain", "no_lists", "no_graph", "sparse_walk_64", "sparse_amb_0")
ACCEL_FIXTURES = ("stretched_3d", "halo_3d", "stretched_2d")


def _sequence(monkeypatch, f, variant):
    e = G.make_engine(monkeypatch, **G.VARIANTS[variant])
    try:
        p = params(f)
        e.set_target(f["target"], p)
        e.set_source(f["source"], p)
        out = []
        for T in D.moving_poses(f):
            st, dbg = e.iterate(T, debug=True)
            out.append((st, dbg["index"]))
        return out
    finally:
        e.close()


@pytest.fixture(scope="module")
def default_sequences():
    return {}


@pytest.mark.parametrize("variant", SWITCHED)
@pytest.mark.parametrize("name", ACCEL_FIXTURES)
def test_accelerations_change_nothing(monkeypatch, default_sequences, name, variant):
    """The moving sequence without certificates and lists, without lists, without the graph, with every walking
    wave searched lane-parallel and with every ambiguous lane re-resolved wave-wide: statistics and indices
    bit-equal to the default engine's at every pose."""
    f = D.fixture(name)
    if name not in default_sequences:
        default_sequences[name] = _sequence(monkeypatch, f, "default")
    ref = default_sequences[name]
    got = _sequence(monkeypatch, f, variant)
    for k, ((a, ia), (b, ib)) in enumerate(zip(ref, got)):
        assert np.array_equal(ia, ib), (name, variant, k, int(np.sum(ia != ib)))
        assert np.array_equal(a, b), (name, variant, k, np.max(np.abs(a - b)))
    assert ref[0][0][-1] >= 0.25 * len(f["source"])


# ============================================================================= shards
@pytest.mark.parametrize("tile", ["64", "16"])
@pytest.mark.parametrize("name", ["stretched_3d", "halo_3d"])
def test_shards_sum_to_the_full_pass(monkeypatch, name, tile):
    """The source in 3 shards, summed in rank order, against the unsharded pass: the criterion of
    test_sharded_statistics_sum_to_full (1e-12 of each entry, and of the largest), the counts exactly; with
    64-point source tiles and with GICP_SRC_TILE=16."""
    f = D.fixture(name)
    p = params(f)
    T = D.moving_poses(f)[3]
    e = G.make_engine(monkeypatch, GICP_SRC_TILE=tile)
    try:
        e.set_target(f["target"], p)
        e.set_source(f["source"], p)
        full = e.iterate(T)
        assert full[-1] >= 0.25 * len(f["source"])
        parts = []
        for s in range(3):
            e.set_source(f["source"], p, shard=s, nshards=3)
            parts.append(e.iterate(T))
        total = parts[0] + parts[1] + parts[2]
        assert total[-1] == full[-1] and sum(part[-1] > 0 for part in parts) >= 2     # (shards are chunks of 64 tiles)
        np.testing.assert_allclose(total, full, rtol=1e-12, atol=1e-12 * np.max(np.abs(full)))
    finally:
        e.close()


# ============================================================================= end to end
@pytest.mark.parametrize("name", ["stretched_3d", "lidar_small"])
def test_whole_loop_vs_oracle(name):
    """gicp.gicp against the oracle's loop, 12 iterations at most: 1e-7 rad and 1e-6 m (the bounds of
    test_align_100k_vs_oracle)."""
    f = D.fixture(name)
    kw = dict(max_iterations=12, tolerance=1e-9, **D.params_kw(f))
    T, *_ = gicp.gicp(f["source"], f["target"], full_output=False, verbose=False, **kw)
    To, *_ = O.gicp(f["source"], f["target"], **kw)
    a, t = S.rotation_angle_error(T, To), S.translation_error(T, To)
    print(f"{name}: GPU vs oracle {a:.3e} rad {t:.3e} m; the motion found {S.rotation_angle_error(To, np.eye(4)):.4f} rad "
          f"{np.linalg.norm(To[:3, 3]):.3f} m")
    assert a < 1e-7 and t < 1e-6, (a, t)
    assert S.rotation_angle_error(To, np.eye(4)) > 1e-3          # (a registration took place)


def test_whole_loop_at_the_offset_origin_vs_oracle():
    """offset_origin_3d: the pose is judged where it acts, on the cloud (largest displacement of a core point
    between the GPU's pose and the oracle's), as test_large_coordinate_offsets judges it, not by its lever-arm
    translation.

    The bound.  The statistics are sums about the far-away origin: with the core's centroid |c| = 5.42e6 m away
    and the core r = 28.5 m in radius (half the room's diagonal), the normal equations' rotation block holds
    |c|^2 where the part that determines the rotation holds r^2, so the reduced system is known to
    u_eff = 2^-53 (|c| / r)^2 = 4e-6 relative to either side, a factor 10 allowed for the growth of rounding
    over the 8000-term sums.  Every Gauss-Newton step is wrong by that share of itself, later steps contract
    earlier errors, and the steps sum to the motion found (rotation w, and w r + |t| on the cloud): the poses
    may differ by 10 u_eff w in angle and 10 u_eff (w r + |t|) in displacement -- about 1.4e-6 rad and
    5e-5 m here, a hundredth of the 5e-3 m test_large_coordinate_offsets allows against the ground truth."""
    f = D.fixture("offset_origin_3d")
    core = f["source"][f["core_source"]]
    kw = dict(max_iterations=12, tolerance=1e-9, **D.params_kw(f))
    T, *_ = gicp.gicp(f["source"], f["target"], full_output=False, verbose=False, **kw)
    To, *_ = O.gicp(f["source"], f["target"], **kw)
    c = core.mean(axis=0)
    r = np.max(np.linalg.norm(core - c, axis=1))
    u_eff = 2.0 ** -53 * (np.linalg.norm(c) / r) ** 2
    w = S.rotation_angle_error(To, np.eye(4))
    moved = np.max(np.linalg.norm(O.apply_transformation(core, To) - core, axis=1))
    disp = np.max(np.linalg.norm(O.apply_transformation(core, T) - O.apply_transformation(core, To), axis=1))
    a = S.rotation_angle_error(T, To)
    print(f"offset_origin_3d: |c| {np.linalg.norm(c):.4e} r {r:.2f} u_eff {u_eff:.2e}; motion {w:.4f} rad, {moved:.3f} m on "
          f"the cloud; GPU vs oracle {a:.3e} rad (bound {10 * u_eff * w:.2e}), {disp:.3e} m (bound {10 * u_eff * moved:.2e})")
    assert w > 1e-3
    assert a <= 10 * u_eff * w and disp <= 10 * u_eff * moved, (a, disp)


# ============================================================================= the fixtures reach their regime
def _first_passes(monkeypatch, f, src, tgt, n_passes, **env):
    e = G.make_engine(monkeypatch, **env)
    try:
        p = params(f)
        e.set_target(tgt, p)
        e.set_source(src, p)
        out = []
        for T in D.moving_poses(f)[:n_passes]:
            e.iterate(T)
            out.append(e.pass_info())
        return out
    finally:
        e.close()


def test_the_fixtures_reach_their_regime(monkeypatch):
    """Conditions on the fixtures, not on correctness; the comparison cloud is the fixture's own core
    (density_ref.core_only), built here.

    1. Collapsed grid: pass 0 of stretched_3d without certificates and lists screens at least 5 times the
       pairs of the same room without its 12 far points.
    2. rho-dominated margin: the first moving pass (pose 1) of halo_3d re-resolves at least 5 times the
       ambiguous lanes of its core alone.

    Measured on an MI355X: (1) 65,702,528 pairs against 1,737,728, a factor 37.8 -- 8012^2 = 64.2 million is
    every source against every target, and the default engine screens as many at every pose of the sequence
    (all 140 source tiles walk, no list is kept); (2) 132 lanes against 2, a factor 66 (pass 0: 345)."""
    f = D.fixture("stretched_3d")
    core_s, core_t = D.core_only("stretched_3d")
    with_far = _first_passes(monkeypatch, f, f["source"], f["target"], 1, **G.VARIANTS["plain"])[0]["pairs"]
    without = _first_passes(monkeypatch, f, core_s, core_t, 1, **G.VARIANTS["plain"])[0]["pairs"]
    print(f"stretched_3d pass 0 (plain): {with_far:.0f} pairs screened, the room alone {without:.0f}: "
          f"ratio {with_far / max(without, 1):.2f}")
    assert without > 0 and with_far >= 5 * without
    h = D.fixture("halo_3d")
    core_s, core_t = D.core_only("halo_3d")
    halo = _first_passes(monkeypatch, h, h["source"], h["target"], 2, **{G.LIBRARY: "1"})[1]["ambiguous"]
    core = _first_passes(monkeypatch, h, core_s, core_t, 2, **{G.LIBRARY: "1"})[1]["ambiguous"]
    print(f"halo_3d pass 1: {halo:.0f} ambiguous lanes re-resolved, the core alone {core:.0f}")
    assert halo > 0 and halo >= 5 * core


# ============================================================================= the fused voxel filter
def _state_error(fn):
    with pytest.raises(_lib.GicpError) as ei:
        fn()
    assert ei.value.code == _lib.GICP_E_STATE, ei.value


def _same_clouds_and_pass(a, b, T, what):
    """The criterion of test_fused_equals_unfused_bit_for_bit: sizes, points, covariances and neighbour counts
    of both clouds, then one pass's statistics and indices, bit for bit."""
    for which in ("target", "source"):
        assert a.cloud_size(which) == b.cloud_size(which), (what, which)
        assert np.array_equal(a.points(which), b.points(which)), (what, which)
        assert np.array_equal(a.covariances(which), b.covariances(which)), (what, which)
        assert np.array_equal(a.neighbor_counts(which), b.neighbor_counts(which)), (what, which)
    sa, da = a.iterate(T, debug=True)
    sb, db = b.iterate(T, debug=True)
    assert sa[-1] > 0, what
    assert np.array_equal(sa, sb) and np.array_equal(da["index"], db["index"]), what
    return sa


def test_fused_voxel_filter_on_a_stretched_cloud():
    """stretched_3d through the fused filter.  Leaf 0.25: 8 10^5 cells per axis, inside the 2^21 of a 63-bit
    key; the fused build equals the unfused path (voxel_downsample, then a plain build) bit for bit.  Leaf
    0.05: 4 10^6 cells, refused with "voxel grid too wide".  The filter runs after the build has begun
    (build_cloud: begin_build, then voxel_filter), so the header's rule for a failed build applies: that cloud
    is NOT SET -- size 0, GICP_E_STATE from a pass and the getters -- the other cloud is untouched, and a later
    good build gives a fresh context's results."""
    f = D.fixture("stretched_3d")
    src, tgt, p = f["source"], f["target"], params(f)
    T = D.moving_poses(f)[2]
    fsrc, ftgt = gicp.voxel_downsample(src, 0.25), gicp.voxel_downsample(tgt, 0.25)
    assert 4000 < len(ftgt) < len(tgt)
    a, b = gicp.Engine(0), gicp.Engine(0)
    try:
        a.set_voxel(0.25)
        a.set_target(tgt, p)
        a.set_source(src, p)
        b.set_target(ftgt, p)
        b.set_source(fsrc, p)
        assert np.array_equal(a.points("target"), ftgt) and np.array_equal(a.points("source"), fsrc)
        before = _same_clouds_and_pass(a, b, T, "leaf 0.25")
        a.iterate(D.moving_poses(f)[3])                                   # warm state to go stale
        src_before = (a.covariances("source"), a.neighbor_counts("source"), a.cloud_size("source"))
        a.set_voxel(0.05)
        with pytest.raises(ValueError, match="voxel grid too wide"):
            a.set_target(tgt, p)
        assert a.cloud_size("target") == 0 and a.cloud_size("source") == src_before[2]
        _state_error(lambda: a.iterate(T))
        _state_error(lambda: a.align(T, params(f, max_iterations=2)))
        _state_error(lambda: a.covariances("target"))
        _state_error(lambda: a.neighbor_counts("target"))
        _state_error(a.graph)
        assert np.array_equal(a.covariances("source"), src_before[0])
        assert np.array_equal(a.neighbor_counts("source"), src_before[1])
        with pytest.raises(ValueError, match="voxel grid too wide"):     # ... and the source alike
            a.set_source(src, p)
        assert a.cloud_size("source") == 0
        _state_error(lambda: a.covariances("source"))
        with pytest.raises(ValueError, match="voxel grid too wide"):
            gicp.voxel_downsample(tgt, 0.05)
        a.set_voxel(0.25)
        a.set_target(tgt, p)
        _state_error(lambda: a.iterate(T))                                # the source is still not set
        a.set_source(src, p)
        after = _same_clouds_and_pass(a, b, T, "after the refused builds")
        assert np.array_equal(after, before)
    finally:
        a.close()
        b.close()
