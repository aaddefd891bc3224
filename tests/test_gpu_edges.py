"""GPU parity away from the one 20k scene: k_corr at large poses, jumps, a wrapping pose ring and other
scales; exact ties and exact boundaries in 3-D; k_knn_cov off its defaults and on analytic clouds; a ladder
of cloud sizes around the tile, sub-tile and unit edges, empty shards and the reduction's level switch.
References: the oracle (cKDTree, fp64) and tests/edge_ref.py (checked by test_edge_ref_cpu.py)."""
import numpy as np
import pytest

import edge_ref as E
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gicp import synthetic as S  # noqa: E402
from gpu_helpers import (P2, P3, RESIDUAL_BOUND, VARIANTS, check_covariances, check_pass,  # noqa: E402
                         make_engine)
from gpu_helpers import ladder_params as _ladder_params  # noqa: E402
from gpu_helpers import ladder_pose as _ladder_pose  # noqa: E402
from gpu_helpers import planar_lattice as _planar_lattice  # noqa: E402

@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scene3d():
    return S.scene_pair_3d(4000)


@pytest.fixture(scope="module")
def scene2d():
    return S.segment_scene_2d(4000)


def _axis(seed):
    a = np.random.default_rng(seed).normal(size=3)
    return a / np.linalg.norm(a)


POSES_3D = {
    "30deg": E.rigid(3, S.axis_angle(_axis(1), np.deg2rad(30.0)), [1.5, -0.7, 0.4]),
    "90deg": E.rigid(3, S.axis_angle(_axis(2), np.deg2rad(90.0)), [-2.0, 1.0, 0.5]),
    "179deg": E.rigid(3, S.axis_angle(_axis(3), np.deg2rad(179.0)), [0.5, 2.5, -1.0]),
    "z90": E.rigid(3, E.rot_z90()),
}
POSES_2D = {"45deg": E.rigid(2, O.rot2(np.deg2rad(45.0)), [30.0, -12.0]),
            "180deg": E.rigid(2, O.rot2(np.deg2rad(180.0)), [5.0, 8.0])}


# ============================================================================= B: poses
@pytest.mark.parametrize("pose", list(POSES_3D))
def test_corr_3d_at_large_rotations(eng, scene3d, pose):
    """k_corr at rotations of 30, 90 and 179 degrees about random axes and the exact quarter turn about z
    (the prologue's fp32 R.rel, the wave box |R|.h): the source is T^-1 of the scene's registered source, so the
    moved cloud lies on the target and a large part of it is accepted."""
    src0, tgt, Tgt = scene3d
    T = POSES_3D[pose]
    src = E.inverse_moved(O.apply_transformation(src0, Tgt), T)
    p = gicp.default_params(3, **P3)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    _, idx = check_pass(eng, src, tgt, T, P3["max_distance_correspondence"], what=pose)
    assert np.mean(idx >= 0) > 0.4


@pytest.mark.parametrize("model", ["point_to_point", "point_to_plane"])
def test_corr_3d_cov_models_at_a_large_rotation(eng, scene3d, model):
    src0, tgt, Tgt = scene3d
    T = POSES_3D["90deg"]
    src = E.inverse_moved(O.apply_transformation(src0, Tgt), T)
    p = gicp.default_params(3, cov_model=gicp._lib.COV_MODELS[model], **P3)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    check_pass(eng, src, tgt, T, P3["max_distance_correspondence"], model=model, what=model)


@pytest.mark.parametrize("pose", list(POSES_2D))
def test_corr_2d_at_large_rotations(eng, scene2d, pose):
    src0, tgt, Tgt = scene2d
    T = POSES_2D[pose]
    src = E.inverse_moved(O.apply_transformation(src0, Tgt), T)
    p = gicp.default_params(2, **P2)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    _, idx = check_pass(eng, src, tgt, T, P2["max_distance_correspondence"], what=pose, coord_atol=True)
    assert np.mean(idx >= 0) > 0.4


def test_corr_jumps_between_distant_poses(scene3d, monkeypatch):
    """Successive passes on one engine at identity, a 90 degree pose, identity + 1e-4, a 179 degree pose and
    identity again: state left by a distant pose (lists, certificates, last matches, the pose ring) must
    never be trusted.  Indices against the oracle after every pass."""
    src, tgt, _ = scene3d
    near = E.rigid(3, t=[1e-4, 0.0, 0.0])
    seq = [("identity", np.eye(4)), ("90deg", POSES_3D["90deg"]), ("identity+1e-4", near),
           ("179deg", POSES_3D["179deg"]), ("identity", np.eye(4))]
    p = gicp.default_params(3, **P3)
    e = make_engine(monkeypatch)
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        for name, T in seq:
            _, dbg = e.iterate(T, debug=True)
            idx, _ = O.correspondences(O.apply_transformation(src, T), tgt, P3["max_distance_correspondence"])
            assert np.array_equal(dbg["index"], idx), name
    finally:
        e.close()


def test_pose_ring_wraps_under_live_certificates(scene3d, monkeypatch):
    """140 passes on one engine (the pose ring holds 64) along a pose creeping by 2e-5 m and 1e-6 rad per
    pass, so most certificates survive, with a 0.1 m jump at pass 70.  Indices against the oracle at every
    pass, statistics against it at passes 0, 63, 64, 65, 128 and 139, and every pass's statistics
    bit-identical to an engine without certificates."""
    from scipy.spatial import cKDTree
    src, tgt, Tgt = scene3d
    tree = cKDTree(tgt)
    p = gicp.default_params(3, **P3)
    d_c = P3["max_distance_correspondence"]
    ax = _axis(7)
    along = np.array([1.0, -0.5, 0.25]) / np.linalg.norm([1.0, -0.5, 0.25])
    poses = []
    for k in range(140):
        T = E.rigid(3, S.axis_angle(ax, k * 1e-6), along * 2e-5 * k)
        if k >= 70:
            T[:3, 3] += [0.1, 0.0, 0.0]
        poses.append(T @ Tgt)      # around the registered pose: most points have a correspondence
    out = {}
    for certs in ("0", "1"):
        e = make_engine(monkeypatch, GICP_NO_CERTS=certs)
        try:
            e.set_target(tgt, p)
            e.set_source(src, p)
            C_s, C_t = e.covariances("source"), e.covariances("target")
            sts, pairs = [], []
            for k, T in enumerate(poses):
                st, dbg = e.iterate(T, debug=True)
                pairs.append(e.pass_info()["pairs"])
                idx, _ = O.correspondences(O.apply_transformation(src, T), tgt, d_c, tree)
                assert np.array_equal(dbg["index"], idx), (certs, k)
                if k in (0, 63, 64, 65, 128, 139):
                    _, _, _, ref = E.pass_reference(src, tgt, T, d_c, C_s, C_t)
                    np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * np.max(np.abs(ref)), err_msg=str(k))
                sts.append(st)
            out[certs] = (sts, pairs)
        finally:
            e.close()
    for k in range(140):
        assert np.array_equal(out["0"][0][k], out["1"][0][k]), k
    # the certificates were live: the creeping passes screened far fewer pairs with them
    assert sum(out["0"][1][1:]) < 0.5 * sum(out["1"][1][1:])


@pytest.mark.parametrize("exp", [-10, 10])
def test_corr_and_covariances_at_other_scales(eng, scene3d, exp):
    """The scene with coordinates, d_c and d_n multiplied by 2^-10 and 2^10 (an exact scaling in fp64):
    indices and neighbour counts exactly the oracle's at that scale, statistics to 1e-9."""
    src0, tgt0, Tgt = scene3d
    f = 2.0 ** exp
    src, tgt = src0 * f, tgt0 * f
    d_c, d_n = 0.5 * f, 1.0 * f
    p = gicp.default_params(3, max_distance_correspondence=d_c, max_distance_nearest_neighbors=d_n)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    _, cnt = O.covariances(tgt, d_n)
    assert np.array_equal(eng.neighbor_counts("target"), cnt)
    _, cnt0 = O.covariances(tgt0, 1.0)
    assert np.array_equal(cnt, cnt0)
    _, cnt_s = O.covariances(src, d_n)
    assert np.array_equal(eng.neighbor_counts("source"), cnt_s)
    T = Tgt.copy()
    T[:3, 3] *= f
    _, idx = check_pass(eng, src, tgt, T, d_c, what=f"2^{exp}")
    assert np.mean(idx >= 0) > 0.4


# ============================================================================= C: exact ties and boundaries
@pytest.fixture(scope="module")
def lattice():
    tgt = E.lattice_target()
    src = E.lattice_sources()
    poses = E.lattice_poses()
    ref = {}
    for kind, s in src.items():
        for name, T in poses.items():
            # the source is T^-1 of the tie points: exact for these dyadic poses
            s_in = E.inverse_moved(s, T)
            assert np.array_equal(O.apply_transformation(s_in, T), s)
            ref[kind, name] = (s_in, T) + E.nearest_lowest_index(s, tgt, 0.5)
    return tgt, ref


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_exact_ties_go_to_the_lowest_index(lattice, monkeypatch, variant):
    """Distinct targets at exactly equal fp64 distances (equal distances go to the smaller
    original index): sources at the cell centres (8-way ties), face centres (4-way) and edge midpoints
    (2-way) of a shuffled dyadic lattice with 40 duplicated points, at the identity, a one-cell shift and the
    exact quarter turn that maps the lattice onto itself.  Index equals the brute-force lowest-index
    reference (duplicates go to the smaller index too), distance to 1 ulp, and a second and third pass at
    the same pose give the same indices (a zero gap must never become a certificate) -- under every search
    variant."""
    tgt, ref = lattice
    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
    e = make_engine(monkeypatch, **VARIANTS[variant])
    try:
        e.set_target(tgt, p)
        for (kind, name), (src, T, idx, dist) in ref.items():
            e.set_source(src, p)
            assert np.all(idx >= 0)
            for rep in range(3):
                st, dbg = e.iterate(T, debug=True)
                bad = np.nonzero(dbg["index"] != idx)[0]
                assert len(bad) == 0, (kind, name, rep, len(bad), dbg["index"][bad[:5]], idx[bad[:5]])
                assert np.all(np.abs(dbg["distance"] - dist) <= np.spacing(dist)), (kind, name, rep)
                assert st[-1] == len(src)
    finally:
        e.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_correspondence_exactly_at_d_c(lattice, monkeypatch, variant):
    """Edge-midpoint sources lie at exactly 0.25 from their two nearest targets: d_c = 0.25 accepts all of
    them (gicp.py:136, inclusive), the next fp64 below 0.25 rejects all of them and the statistics' count
    is 0.  The kernel compares squared distances with the largest d2 whose square root is <= d_c; for
    d_c = 0.25 that is the double above 0.0625, so the second half of the test puts every source at a dyadic
    offset from a lattice point whose squared length is exactly that largest d2 for d_c = |offset|
    (edge_ref.last_accepted_offset): accepted at d_c, rejected at the next fp64 below."""
    tgt, ref = lattice
    n_unique = int(np.prod(E.LATTICE))
    off, d2, d_off = E.last_accepted_offset()
    cases = [("edges", name, 0.25) + ref["edges", name] for name in ("identity", "turn")]
    for name in ("identity", "turn"):
        T = E.lattice_poses()[name]
        s = tgt[:n_unique] + off
        s_in = E.inverse_moved(s, T)
        assert np.array_equal(O.apply_transformation(s_in, T), s)
        cases.append(("offset", name, d_off, s_in, T) + E.nearest_lowest_index(s, tgt, d_off))
    e = make_engine(monkeypatch, **VARIANTS[variant])
    try:
        for kind, name, d_c, src, T, idx, dist in cases:
            assert np.all(dist == d_c) and np.all(idx >= 0)
            p = gicp.default_params(3, max_distance_correspondence=d_c, max_distance_nearest_neighbors=1.0)
            e.set_target(tgt, p)
            e.set_source(src, p)
            for rep in range(2):
                st, dbg = e.iterate(T, debug=True)
                assert np.array_equal(dbg["index"], idx) and st[-1] == len(src), (kind, name, rep, st[-1])
                assert np.all(dbg["distance"] == d_c)
            p = gicp.default_params(3, max_distance_correspondence=float(np.nextafter(d_c, 0)),
                                    max_distance_nearest_neighbors=1.0)
            e.set_source(src, p)
            for rep in range(2):
                st, dbg = e.iterate(T, debug=True)
                assert np.all(dbg["index"] == -1), (kind, name, rep, int(np.sum(dbg["index"] >= 0)))
                assert st[-1] == 0 and np.all(st[:gicp.stats_size(3)] == 0)
    finally:
        e.close()


def test_graph_rows_on_the_lattice(eng, lattice):
    """The property of test_target_graph_rows_cover_their_radius for every point of the lattice target,
    whose neighbour shells are exact ties (6 at 0.5, 12 at 0.5 sqrt 2, 8 at 0.5 sqrt 3 around an interior
    point: the 20-entry row ends inside a tied shell): every other target strictly inside radius[i] is in
    row i (the duplicates at distance 0 included), rows hold distinct other points nearest first, and the
    radius never exceeds the 21st other neighbour's distance.

    A row whose ties overflowed certifies nothing (radius 0).  k_knn_cov ranks the candidates by a key that
    is the fp32 squared distance with its low 6 bits replaced by the point's slot in its tile, so points of
    one shell tie only where their slots collide too: a row overflows when more than 20 others have a key
    at or below the 21st, which the geometry allows only where more than 20 others lie at or below the 20th
    other neighbour's distance, and then happens or not with the tile layout (measured on an MI355X: 791 of
    the 904 rows have such a tie, 39 overflow).  So: rows with radius 0 exist, each of them has the
    geometric tie, every row without it has a positive radius, and the coverage property above holds for
    every row -- which is what fails when an overflowed row keeps a radius, since such a row was filled in
    scan order and lacks nearer points than the ones it holds.
    (d_n = 2 here, so that every point's 21st other neighbour lies well inside the search radius.)"""
    tgt, _ = lattice
    d_n = 2.0
    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=d_n)
    eng.set_target(tgt, p)
    idx, rad = eng.graph()
    assert idx.shape == (len(tgt), 20) and np.all(rad >= 0) and np.all(np.isfinite(rad))
    d2 = ((tgt[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    srt = np.sort(d2, axis=1)
    d20, d21 = srt[:, 19], srt[:, 20]
    assert np.all(d21 < (0.9 * d_n) ** 2)
    assert np.all(rad <= np.sqrt(d21) * (1 + 1e-5))
    uncovered = []
    for i in range(len(tgt)):
        row = idx[i][idx[i] >= 0]
        assert i not in row and len(set(row)) == len(row), i
        assert np.all(idx[i][len(row):] < 0)
        inside = np.nonzero(d2[i] < rad[i] * rad[i])[0]
        if not set(inside) <= set(row):
            uncovered.append(i)
            continue
        d = np.sqrt(d2[i][row])
        assert np.all(np.diff(d) >= -1e-6 * (1.0 + d[1:])), (i, d)
    tie = (d2 <= d20[:, None]).sum(axis=1) > 20
    print(f"lattice graph: {int(tie.sum())} of {len(tgt)} rows end in a tie; radius 0 on {int(np.sum(rad == 0))}; "
          f"{len(uncovered)} rows do not cover their radius")
    assert not uncovered, uncovered[:10]
    assert tie.sum() > 100 and (~tie).sum() > 100
    assert np.any(rad == 0)
    assert np.all(tie[rad == 0]), np.nonzero(~tie & (rad == 0))[0][:10]


# ============================================================================= D: k_knn_cov off its defaults
COV_CASES = {"k10": dict(k_neighbors=10), "eps_ratio": dict(epsilon=1.0, ratio=0.01),
             "min5": dict(min_neighbors=5), "all": dict(k_neighbors=10, epsilon=1.0, ratio=0.01, min_neighbors=5)}


@pytest.mark.parametrize("case", list(COV_CASES))
@pytest.mark.parametrize("dim", [2, 3])
def test_covariances_off_defaults(eng, scene3d, scene2d, dim, case):
    """k_knn_cov<3,10> / <2,10> and non-default epsilon, ratio, min_neighbors on random clouds (d_n = 3 m on
    the 4000-point room, so most points have more than k neighbours within it and the k-th one decides)."""
    kw = COV_CASES[case]
    pts, d_n = (scene3d[1], 3.0) if dim == 3 else (scene2d[1], 25.0)
    p = gicp.default_params(dim, max_distance_correspondence=0.5 if dim == 3 else 20.0,
                            max_distance_nearest_neighbors=d_n, **kw)
    eng.set_target(pts, p)
    rep = check_covariances(eng, pts, d_n, **kw)
    assert rep["surface"].mean() > 0.5
    if "k_neighbors" in kw:
        assert rep["counts"].max() == 10 and np.mean(rep["counts"] == 10) > 0.3


def test_point_to_plane_weights_with_other_epsilon_and_ratio(eng, scene3d):
    """pl_inv of corr_args depends on epsilon: W = n n^T of the point-to-plane model from covariances built
    with epsilon = 1, ratio = 0.01, min_neighbors = 5 (no surface: W = 0)."""
    src, tgt, Tgt = scene3d
    kw = dict(epsilon=1.0, ratio=0.01, min_neighbors=5)
    p = gicp.default_params(3, cov_model=2, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0, **kw)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    _, idx = check_pass(eng, src, tgt, Tgt, 0.5, model="point_to_plane", min_neighbors=5, what="ptp eps=1")
    cnt = eng.neighbor_counts("target")
    ok = idx >= 0
    assert np.any(cnt[idx[ok]] < 5) and np.any(cnt[idx[ok]] >= 5)


@pytest.mark.parametrize("d_n,interior,counts", [(1.0, 9, None), (float(np.nextafter(1.0, 2)), 13, None),
                                                 (1.05, 13, {6, 8, 9, 11, 12, 13})])
def test_planar_lattice_neighbourhoods(eng, d_n, interior, counts):
    """A shuffled planar 12 x 12 lattice of spacing 0.5 at z = 0: neighbours at exactly d_n = 1.0 are
    excluded (strict), with the next fp64 above 1.0 they are included; counts equal the oracle's (interior
    points 9 and 13), and C = diag(eps, eps, eps ratio) to 1e-12 wherever a surface exists."""
    pts = _planar_lattice()
    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=d_n)
    eng.set_target(pts, p)
    cnt = eng.neighbor_counts("target")
    _, cnt_or = O.covariances(pts, d_n)
    assert np.array_equal(cnt, cnt_or)
    inner = np.all((pts[:, :2] >= 1.0) & (pts[:, :2] <= 4.5), axis=1)
    assert np.all(cnt[inner] == interior)
    if counts is not None:
        assert set(cnt.tolist()) == counts
    C = eng.covariances("target")
    want = np.diag([O.EPSILON, O.EPSILON, O.EPSILON * O.RATIO])
    assert np.all(cnt >= 3)
    assert np.max(np.abs(C - want)) <= 1e-12 * O.EPSILON, np.max(np.abs(C - want))


def test_collinear_and_coincident_clouds(eng):
    """200 collinear points (two zero eigenvalues: any normal across the line will do): eigenvalues
    {eps ratio, eps, eps} and the normal perpendicular to the line to 1e-12; 30 copies of one point (zero
    sample covariance): finite C with those eigenvalues."""
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    line = np.array([3.0, -1.0, 2.0]) + np.arange(200)[:, None] * 0.05 * u
    p = gicp.default_params(3, **P3)
    eng.set_target(line, p)
    C = eng.covariances("target")
    cnt = eng.neighbor_counts("target")
    _, cnt_or = O.covariances(line, 1.0)
    assert np.array_equal(cnt, cnt_or) and np.all(np.isfinite(C))
    assert E.cov_structure_error(C, O.EPSILON, O.RATIO).max() <= 1e-12
    n = E.normal_of(C, O.EPSILON, O.RATIO)
    assert np.max(np.abs(n @ u)) <= 1e-12, np.max(np.abs(n @ u))
    same = np.tile(np.array([[0.375, -1.25, 2.5]]), (30, 1))
    eng.set_target(same, p)
    C = eng.covariances("target")
    assert np.array_equal(eng.neighbor_counts("target"), np.full(30, 20)) and np.all(np.isfinite(C))
    assert E.cov_structure_error(C, O.EPSILON, O.RATIO).max() <= 1e-12


def test_tied_kth_neighbour(eng):
    """Point 0's 24 nearest neighbours are all at exactly the same distance and k = 20 takes 19 of them:
    whichever the kernel takes (the fp64 ambiguity path decides), the count is exact and its normal is an
    eigenvector, to 1e-13, of the sample covariance of one of the 19-subsets."""
    pts, tied = E.tied_kth_cloud()
    p = gicp.default_params(3, **P3)
    eng.set_target(pts, p)
    cnt = eng.neighbor_counts("target")
    _, cnt_or = O.covariances(pts, 1.0)
    assert np.array_equal(cnt, cnt_or) and cnt[0] == 20
    C = eng.covariances("target")
    assert np.all(np.isfinite(C))
    surf = cnt >= 3
    assert E.cov_structure_error(C[surf], O.EPSILON, O.RATIO).max() <= 1e-12
    n0 = E.normal_of(C[:1], O.EPSILON, O.RATIO)[0]
    res = E.tied_subset_residuals(pts, tied, 19, n0)
    print(f"tied k-th neighbour: best eigen-residual over the 19-subsets {res:.2e}")
    assert res <= RESIDUAL_BOUND, res
    # the points whose neighbourhood has no tie at its edge meet the usual criterion
    far = np.arange(25, len(pts))
    rep = E.covariance_report(pts, 1.0, 20, O.EPSILON, O.RATIO, 3, C, cnt)
    assert rep["residual"][far].max() <= RESIDUAL_BOUND, rep["residual"][far].max()


# ============================================================================= E: size ladder
def _affine_rank(x):
    """Dimension of the affine hull of the points x (0 for none or one point): singular values of the
    centred points above 1e-6 of the largest."""
    if len(x) < 2:
        return 0
    sv = np.linalg.svd(x - x.mean(axis=0), compute_uv=False)
    return int(np.sum(sv > 1e-6 * max(sv[0], 1e-300))) if sv[0] > 0 else 0


@pytest.mark.parametrize("n,m", E.LADDER_PAIRS, ids=[f"{n}x{m}" for n, m in E.LADDER_PAIRS])
@pytest.mark.parametrize("dim", [2, 3])
def test_size_ladder(eng, dim, n, m):
    """Source / target sizes at the sub-tile (16), tile (64) and unit (4 x 64) edges and either side of
    them, 1, 2, 3 points, and very unequal pairs, on a dense patch: counts and covariances of both clouds
    (the criteria of the covariance tests), one pass at a 1.5 degree pose (index exact, W and statistics
    to 1e-9; at least 50 % accepted where both clouds have >= 64 points -- a 3- or 1-point target cannot
    accept half of 65 or 1025 sources) and a 3-iteration align against the host loop over the same passes,
    poses to 1e-10.

    The poses are compared where the first pass determines one: at least d + 1 affinely independent
    accepted sources and as many affinely independent matched targets (_affine_rank == d of both).  With
    fewer -- one to three correspondences, or every source matched to the same one or two targets -- all
    points lie on a line or plane, the plane-to-plane weights all constrain along (nearly) one normal and
    the rotation is free or nearly so: measured on the GPU, device and host poses then differ by 8e-10
    (3 x 65 in 3-D) up to 1 (1 x 1), both minimisers.  What is determined there is the minimum: after one
    iteration the device's pose must be as good a minimiser of the pass's quadratic as the host's and
    report its loss, to 1e-10 of the starting loss (or of 1), and three iterations must end finite and
    orthonormal to 1e-12."""
    src, tgt = E.dense_patch(dim, n, m)
    p = _ladder_params(dim)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    check_covariances(eng, tgt, 1.0, "target")
    check_covariances(eng, src, 1.0, "source")
    T = _ladder_pose(src)
    _, idx = check_pass(eng, src, tgt, T, 0.5, what=f"{dim}-D {n}x{m}")
    if n >= 64 and m >= 64:
        assert np.mean(idx >= 0) >= 0.5
    pa = _ladder_params(dim, fixed_iterations=1, max_iterations=3, tolerance=0.0)
    T0 = np.eye(dim + 1)
    idx0, _ = O.correspondences(src, tgt, 0.5)
    ok = idx0 >= 0
    determined = _affine_rank(src[ok]) == dim and _affine_rank(tgt[idx0[ok]]) == dim
    assert determined or min(n, m) <= 3        # every pair of the ladder beyond the 1-, 2-, 3-point ones
    if determined:
        Th = T0
        for _ in range(3):
            Th, _ = gicp.solve_pose(eng.iterate(Th), Th)
        Tdev, res = eng.align(None, pa)
        assert res["iterations"] == 3
        np.testing.assert_allclose(Tdev, Th, rtol=0, atol=1e-10)
        return
    st = eng.iterate(T0)
    H, g, c0, cnt = O.expand_stats(st, dim)
    assert cnt == ok.sum()
    pa.max_iterations = 1
    _, fh = gicp.solve_pose(st, T0)
    T1, res, tr = eng.align(None, pa, trace=True)
    tol = 1e-10 * max(1.0, c0)
    print(f"ladder {dim}-D {n}x{m}: count {cnt:.0f} c0 {c0:.3e} host loss {fh:.3e} device loss {tr['losses'][0]:.3e} "
          f"quadratic at the device pose {O.quad_loss(T1, H, g, c0, T0):.3e}")
    assert abs(O.quad_loss(T1, H, g, c0, T0) - fh) <= tol
    assert abs(tr["losses"][0] - fh) <= tol
    pa.max_iterations = 3
    T3, res = eng.align(None, pa)
    R = T3[:dim, :dim]
    assert res["iterations"] == 3 and np.all(np.isfinite(T3))
    assert np.max(np.abs(R @ R.T - np.eye(dim))) <= 1e-12


@pytest.mark.parametrize("n,tile", [(257, "64"), (1025, "64"), (1025, "16")])
@pytest.mark.parametrize("nshards", [3, 7])
def test_shards_of_small_clouds(monkeypatch, n, tile, nshards):
    """Shards are chunks of 16 units of 4 tiles: a small cloud has fewer chunks than shards.  The shard
    statistics sum to the full statistics (1e-12), and a shard that owns no tile returns exact zeros (the
    one-process path that clears the statistics without a launch).  257 and 1025 points in 64-point tiles
    are one chunk; 1025 points in 16-point tiles are two."""
    src, tgt = E.dense_patch(3, n, n)
    p = _ladder_params(3)
    T = _ladder_pose(src)
    e = make_engine(monkeypatch, GICP_SRC_TILE=tile)
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        full = e.iterate(T)
        assert full[-1] >= 0.5 * n
        parts = []
        for s in range(nshards):
            e.set_source(src, p, shard=s, nshards=nshards)
            parts.append(e.iterate(T))
            assert np.array_equal(parts[-1], e.iterate(T))
        np.testing.assert_allclose(np.sum(parts, axis=0), full, rtol=1e-12, atol=1e-12 * np.max(np.abs(full)))
        owners = [s for s in range(nshards) if parts[s][-1] > 0]
        assert owners == ([0] if tile == "64" else [0, 1]), owners
        for s in range(nshards):
            if s not in owners:
                assert np.all(parts[s] == 0), s
        # ... and the align of an empty shard (no exchange set) leaves the pose where it was
        e.set_source(src, p, shard=nshards - 1, nshards=nshards)
        Tal, res = e.align(T, _ladder_params(3, fixed_iterations=1, max_iterations=2, tolerance=0.0))
        assert np.array_equal(Tal, T) and res["correspondences"] == 0
    finally:
        e.close()


@pytest.fixture(scope="module")
def patch12400():
    """(source, target): the sizes below are prefixes of the source (uniform subsamples of the patch)."""
    src, tgt = E.dense_patch(3, 12400, 8400)
    return src, tgt


def _tiles(e_plain, src, p, T):
    """Source tiles of `src`: the waves that walk on a cold pass of an engine without certificates,
    lists or graph (every tile holds at least one point, and every lane without a certificate walks)."""
    e_plain.set_source(src, p)
    e_plain.iterate(T)
    return int(e_plain.pass_info()["walked_tiles"])


def test_reduction_levels(patch12400, monkeypatch):
    """With 16-point source tiles, 6000 ... 8400 points are 100 ... 180 units of 4 tiles: the in-launch
    reduction switches from one level to two (kFlatUnits = 128) inside the range, and to a second and
    third group of 64 units.  For each size the statistics against the oracle (1e-9) and two successive
    passes bit-identical; then the same at sizes found to give exactly 127, 128, 129, 192 and 193 units."""
    src, tgt = patch12400
    p = _ladder_params(3)
    T = _ladder_pose(src)
    plain = make_engine(monkeypatch, GICP_SRC_TILE="16", GICP_NO_CERTS="1", GICP_NO_LISTS="1", GICP_NO_GRAPH="1")
    e = make_engine(monkeypatch, GICP_SRC_TILE="16")
    try:
        for x in (plain, e):
            x.set_target(tgt, p)

        def check(n):
            s = src[:n]
            e.set_source(s, p)
            st, _ = check_pass(e, s, tgt, T, 0.5, what=f"n={n}")
            assert np.array_equal(st, e.iterate(T)) and np.array_equal(st, e.iterate(T)), n

        units = {}
        for n in range(6000, 8401, 200):
            tiles = _tiles(plain, src[:n], p, T)
            assert n / 16 <= tiles <= 1.35 * n / 16 + 1, (n, tiles)
            units[n] = -(-tiles // 4)
            check(n)
        print(f"units per size: {units}")
        assert min(units.values()) <= 128 < max(units.values())
        def units_of(n):
            return -(-_tiles(plain, src[:n], p, T) // 4)

        for want in (127, 128, 129, 192, 193):
            lo, hi = 64, len(src)            # units_of(lo) < want <= units_of(hi): the first prefix that reaches it
            assert units_of(lo) < want <= units_of(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if units_of(mid) >= want:
                    hi = mid
                else:
                    lo = mid
            assert units_of(hi) == want, (want, hi, units_of(hi))
            print(f"{want} units at n = {hi}")
            check(hi)
    finally:
        plain.close()
        e.close()
