"""CPU checks of tests/edge_ref.py, the references and input builders of the edge-case GPU tests: the
references are right on their own terms (in 50-digit arithmetic where they claim it), and the inputs have
the properties the GPU tests rely on.  No GPU is used."""
import mpmath as mp
import numpy as np
import pytest

import edge_ref as E
from oracle import gicp_oracle as O

gicp = pytest.importorskip("gicp")


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("dim", [2, 3])
def test_solve_reference_is_a_minimiser_and_pins_the_host_solver(dim):
    """For every case of section A the polished reference is a strict local minimiser of the closed-form
    quadratic in 50-digit arithmetic (tangent gradient < 1e-30, tangent Hessian positive definite), its
    loss agrees with O.inner_gn's per-point loss to 1e-9, and inner_gn's pose lies within 1e-9 of it (so
    the reference is the minimiser inner_gn found, not another one).  The host solver stays within the
    figures the device bounds are derived from (edge_ref.HOST_*)."""
    worst = dict(pose=0.0, loss=0.0, orth=0.0)
    for angle, ident in E.solve_cases(dim):
        s, q, W, idx, Tk, st = E.solve_case(dim, angle, ident)
        ref = E.solve_reference(s, q, W, idx, Tk, st)
        with mp.workdps(E.MP_DIGITS):
            assert ref["grad_norm"] < mp.mpf("1e-30"), (angle, ident)
            assert ref["hess_min_eig"] > 0, (angle, ident)
        assert abs(ref["loss"] - ref["gn_loss"]) <= 1e-9 * ref["gn_loss"], (angle, ident)
        assert np.max(np.abs(ref["T"] - ref["gn_T"])) < 1e-9, (angle, ident)
        R = ref["T"][:dim, :dim]
        assert np.max(np.abs(R @ R.T - np.eye(dim))) < 1e-15
        # the true motion is recovered: the reference turns by the case's angle to the noise level
        ang = np.arctan2(R[1, 0], R[0, 0]) if dim == 2 else np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
        assert abs(ang - (angle if dim == 2 else abs(angle))) < 2e-3, (angle, ident, ang)
        Th, fh = gicp.solve_pose(st, Tk)
        worst["pose"] = max(worst["pose"], np.max(np.abs(Th - ref["T"])))
        worst["loss"] = max(worst["loss"], abs(fh - E.mp_quad_loss(st, Tk, Th)) / ref["loss"])
        worst["orth"] = max(worst["orth"], np.max(np.abs(Th[:dim, :dim] @ Th[:dim, :dim].T - np.eye(dim))))
    print(f"host solver, {dim}-D, worst over the cases: {worst}")
    assert worst["pose"] <= E.HOST_POSE_ERR[dim]
    assert worst["loss"] <= E.HOST_LOSS_ERR[dim]
    assert worst["orth"] <= E.HOST_ORTH_ERR[dim]


def test_mp_quad_loss_matches_the_per_point_loss():
    s, q, W, idx, Tk, st = E.solve_case(3, 0.5, False)
    ok = idx >= 0
    for T in (Tk, E.solve_reference(s, q, W, idx, Tk, st)["T"]):
        r = q[ok] - s[ok] @ T[:3, :3].T - T[:3, 3]
        direct = float(np.einsum("na,nab,nb->", r, W[ok], r))
        assert abs(E.mp_quad_loss(st, Tk, T) - direct) <= 1e-9 * direct


def test_degenerate_statistics_are_degenerate():
    for d in (2, 3):
        H = O.expand_stats(E.parallel_normal_stats(d), d)[0]
        assert np.linalg.matrix_rank(H[d * d:, d * d:]) == 1          # translation block: rank one
        with pytest.raises(ValueError):                                # ... which the host solver refuses
            gicp.solve_pose(E.parallel_normal_stats(d), np.eye(d + 1))
    st = E.collinear_stats()
    H, g, c0, cnt = O.expand_stats(st, 3)
    assert cnt == 200 and np.linalg.eigvalsh(H[9:, 9:])[0] > 0       # translation block SPD ...
    Th, fh = gicp.solve_pose(st, np.eye(4))                           # ... and the host solves it
    assert np.all(np.isfinite(Th)) and fh <= c0


# ----------------------------------------------------------------------------- C
def test_nearest_lowest_index_matches_the_kdtree_where_unique():
    rng = np.random.default_rng(0)
    tgt = rng.uniform(0, 10, (500, 3))
    pts = rng.uniform(0, 10, (700, 3))
    idx, dist = E.nearest_lowest_index(pts, tgt, 0.8)
    io, do = O.correspondences(pts, tgt, 0.8)
    assert np.array_equal(idx, io) and (idx >= 0).any() and (idx < 0).any()
    np.testing.assert_allclose(dist, do, rtol=1e-15)
    # on the lattice: equal wherever the minimum is unique, and the lowest index where it is not
    tgt = E.lattice_target()
    mult = dict(cells=8, faces=4, edges=2)
    for name, src in E.lattice_sources().items():
        src = np.concatenate([src, src + np.array([0.125, 0.0625, -0.03125])])     # second half: unique minima
        idx, dist = E.nearest_lowest_index(src, tgt, 0.5)
        io, do = O.correspondences(src, tgt, 0.5)
        d2 = ((src[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
        ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
        uniq = ties == 1
        assert uniq[len(src) // 2:].mean() > 0.9
        assert np.array_equal(idx[uniq], io[uniq])
        assert np.array_equal(dist, do)
        first = np.array([np.nonzero(d2[i] == d2[i].min())[0][0] for i in range(len(src))])
        assert np.array_equal(idx, first)
        assert np.all(ties[:len(src) // 2] >= mult[name])           # (more where a duplicate takes part)


def test_lattice_inputs_are_exact():
    tgt = E.lattice_target()
    n = int(np.prod(E.LATTICE))
    assert len(tgt) == n + 40 and len(np.unique(tgt, axis=0)) == n
    assert np.array_equal(tgt * 2, np.round(tgt * 2))                         # dyadic
    assert not np.array_equal(np.lexsort(tgt[:n].T[::-1]), np.arange(n))      # shuffled
    src = E.lattice_sources()
    assert len(src["cells"]) == 11 * 11 * 5
    _, d = E.nearest_lowest_index(src["edges"], tgt, 1.0)
    assert np.all(d == 0.25)
    _, d = E.nearest_lowest_index(src["cells"], tgt, 1.0)
    assert np.all(d == np.sqrt(0.1875))
    lat = {tuple(p) for p in tgt}
    for name, T in E.lattice_poses().items():
        assert np.array_equal(T * 2, np.round(T * 2))
        moved = O.apply_transformation(tgt, T)
        inside = np.all((moved >= 0) & (moved <= (np.array(E.LATTICE) - 1) * E.SPACING), axis=1)
        assert all(tuple(p) in lat for p in moved[inside])                   # lattice points go to lattice points
        if name == "turn":
            assert inside.all()                                               # ... the quarter turn maps it onto itself


def test_last_accepted_offset():
    o, d2, d_c = E.last_accepted_offset()
    assert np.array_equal(o * 64, np.round(o * 64)) and np.max(np.abs(o)) < 0.25
    assert d2 == o[0] * o[0] + o[1] * o[1] + o[2] * o[2] == o[2] * o[2] + o[1] * o[1] + o[0] * o[0]
    assert np.sqrt(d2) <= d_c < np.sqrt(np.nextafter(d2, np.inf)) and d_c * d_c != d2
    assert np.sqrt(d2) > np.nextafter(d_c, 0)
    tgt = E.lattice_target()
    idx, dist = E.nearest_lowest_index(tgt[:100] + o, tgt, d_c)
    assert np.all(dist == d_c) and np.all(idx >= 0) and np.array_equal(tgt[idx], tgt[:100])


# ----------------------------------------------------------------------------- D
def test_covariance_report_on_the_oracles_own_output():
    """The criteria of the covariance tests hold for the oracle itself: counts, eigenvalue structure to
    1e-12, eigen-residual of np.linalg.eigh's normal far below the 1e-13 the kernel is held to."""
    from gicp import synthetic as S
    _, tgt, _ = S.scene_pair_3d(4000)
    for eps, ratio, k, mn in ((100.0, 0.1, 20, 3), (1.0, 0.01, 10, 5)):
        C, cnt = O.covariances(tgt, 3.0, k, eps, ratio, mn, faithful=False)
        rep = E.covariance_report(tgt, 3.0, k, eps, ratio, mn, C, cnt)
        assert rep["count_ok"] and rep["identity_ok"] and rep["surface"].mean() > 0.5
        assert rep["structure"].max() < 1e-12
        assert rep["residual"].max() < 5e-15, rep["residual"].max()
        assert rep["entry_err"].max() == 0.0
    pts2 = S.segment_scene_2d(2000)[1]
    C, cnt = O.covariances(pts2, 25.0, 10, 1.0, 0.01, 5, faithful=False)
    rep = E.covariance_report(pts2, 25.0, 10, 1.0, 0.01, 5, C, cnt)
    assert rep["count_ok"] and rep["structure"].max() < 1e-12 and rep["residual"].max() < 5e-15


def test_tied_kth_cloud():
    pts, tied = E.tied_kth_cloud()
    d2 = (pts ** 2).sum(1)
    assert np.all(d2[tied] == 0.3125) and len(tied) == 24 and len(np.unique(pts[tied], axis=0)) == 24
    assert np.all(d2[25:] > 0.81) and len(pts) == 425
    idx, valid, _ = O.neighbourhoods(pts, 1.0, 20)
    assert valid[0].sum() == 20 and set(idx[0][1:]) <= set(tied)
    # the enumeration contains the subset the KD-tree chose: its eigenvector has residual ~0 there
    S = E.sample_covariance(pts[idx[0]])
    n = np.linalg.eigh(S)[1][:, 0]
    assert E.tied_subset_residuals(pts, tied, 19, n) < 5e-15


# ----------------------------------------------------------------------------- E
@pytest.mark.parametrize("dim", [2, 3])
def test_dense_patch_has_surfaces_and_correspondences(dim):
    for n, m in E.LADDER_PAIRS:
        src, tgt = E.dense_patch(dim, n, m)
        assert src.shape == (n, dim) and tgt.shape == (m, dim)
        if n >= 64 and m >= 64:
            idx, _ = O.correspondences(src, tgt, 0.5)
            assert np.mean(idx >= 0) >= 0.5
            _, cnt = O.covariances(tgt, 1.0)
            assert np.mean(cnt >= dim) >= 0.5
