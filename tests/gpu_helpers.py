"""Helpers shared by the GPU tests that drive engines directly (test_gpu_edges.py, test_gpu_history.py,
test_gpu_density.py): engines created under GICP_* switches, one pass against the oracle, the covariance
criteria, the graph rows' coverage, and the small input builders the files share.  References: the oracle
(cKDTree, fp64) and tests/edge_ref.py."""
import numpy as np
import pytest

import edge_ref as E
from oracle import gicp_oracle as O

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402
from gicp import synthetic as S  # noqa: E402

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
P2 = dict(max_distance_correspondence=20.0, max_distance_nearest_neighbors=25.0)
FLAGS = ("GICP_NO_CERTS", "GICP_NO_LISTS", "GICP_NO_GRAPH", "GICP_SPARSE_WALK", "GICP_SPARSE_AMB", "GICP_SRC_TILE")
DEFAULTS = dict(GICP_NO_CERTS="0", GICP_NO_LISTS="0", GICP_NO_GRAPH="0", GICP_SPARSE_WALK="2", GICP_SPARSE_AMB="2",
                GICP_SRC_TILE="64")


LIBRARY = "LIBRARY_DEFAULTS"   # make_engine(**{LIBRARY: "1"}): none of the GICP_* switches set


def make_engine(monkeypatch, **env):
    """An engine created under the given GICP_* switches (read at creation), the others at DEFAULTS; with
    LIBRARY given, with every switch unset, so that the library's own defaults are what runs (they are not
    DEFAULTS: the library walks sparsely up to 4 lanes, DEFAULTS pins GICP_SPARSE_WALK=2)."""
    if env.pop(LIBRARY, None):
        assert not env, env
        for k in FLAGS:
            monkeypatch.delenv(k, raising=False)
        return gicp.Engine(0)
    for k in FLAGS:
        monkeypatch.setenv(k, str(env.get(k, DEFAULTS[k])))
    e = gicp.Engine(0)
    for k in FLAGS:
        monkeypatch.delenv(k)
    return e


VARIANTS = {"default": {}, "no_certs": dict(GICP_NO_CERTS="1"), "no_lists": dict(GICP_NO_LISTS="1"),
            "plain": dict(GICP_NO_CERTS="1", GICP_NO_LISTS="1"), "no_graph": dict(GICP_NO_GRAPH="1"),
            "sparse_walk_0": dict(GICP_SPARSE_WALK="0"), "sparse_walk_64": dict(GICP_SPARSE_WALK="64"),
            "sparse_amb_0": dict(GICP_SPARSE_AMB="0"), "sparse_amb_64": dict(GICP_SPARSE_AMB="64"),
            "library": {LIBRARY: "1"}}


def check_pass(eng, src, tgt, T, d_c, model="plane_to_plane", min_neighbors=None, what="", coord_atol=False):
    """One iterate at T against the oracle with the tolerances of test_iteration_3d_vs_oracle: index
    bit-exact, finite distances rtol 1e-12, W rtol 1e-9, statistics rtol 1e-9.

    coord_atol (the 2-D scene at large rotations only): the distance also gets the absolute error that
    R s + t itself has in fp64, on the oracle's side and on the kernel's: three roundings (two products
    summed, plus t) of relative size 2^-53 on terms as large as |R||s| + |t|, per coordinate and per side:
    2 * 3 * sqrt(d) * 2^-53 * max(|R||s| + |t|).  With coordinates to 1500 px turned by 45 degrees that is
    2e-12 px, where rtol 1e-12 alone asks for 5e-14 px of a 0.05 px distance, less than one ulp of a
    coordinate: measured there on the GPU, 3 of 4000 distances differ by 1.1e-13 px, 2.5e-12 relative."""
    C_t = eng.covariances("target")
    C_s = eng.covariances("source")
    cnt_t = eng.neighbor_counts("target")
    st, dbg = eng.iterate(T, debug=True)
    idx, dist, W, ref = E.pass_reference(src, tgt, T, d_c, C_s, C_t, model, cnt_t, min_neighbors)
    assert np.array_equal(dbg["index"], idx), (what, int(np.sum(dbg["index"] != idx)))
    fin = np.isfinite(dbg["distance"])
    assert np.all(fin[idx >= 0]) and np.all(dist[~fin] > d_c), what
    d = src.shape[1]
    size = np.max(np.abs(src) @ np.abs(T[:d, :d]).T + np.abs(T[:d, d]))
    np.testing.assert_allclose(dbg["distance"][fin], dist[fin], rtol=1e-12,
                               atol=6 * np.sqrt(d) * 2.0 ** -53 * size if coord_atol else 0.0, err_msg=what)
    np.testing.assert_allclose(dbg["weight"], W, rtol=1e-9, atol=1e-15 if model == "plane_to_plane" else 1e-12,
                               err_msg=what)
    np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * max(np.max(np.abs(ref)), 1e-300), err_msg=what)
    return st, idx


RESIDUAL_BOUND = 1e-13     # np.linalg.eigh's own residual is <= 7.3e-16; ~130x for one-pass sums and Jacobi sweeps


def check_covariances(eng, pts, d_n, which="target", max_left_out=0.02, **kw):
    """The covariance criteria on the engine's `which` cloud (already set with the same parameters):
    counts exact; C = a I - m m^T with eigenvalues {eps ratio, eps, ...} to 1e-12; the recovered normal's
    eigen-residual against the oracle neighbourhood's sample covariance <= 1e-13; entrywise 1e-8 wherever
    the relative eigen-gap is >= 1e-2, which may leave out at most 2 % of the points."""
    d = pts.shape[1]
    k = kw.get("k_neighbors", O.default_k(d))
    eps, ratio = kw.get("epsilon", O.EPSILON), kw.get("ratio", O.RATIO)
    mn = kw.get("min_neighbors", d)
    C = eng.covariances(which)
    cnt = eng.neighbor_counts(which)
    rep = E.covariance_report(pts, d_n, k, eps, ratio, mn, C, cnt)
    assert np.all(np.isfinite(C))
    assert rep["count_ok"], int(np.sum(cnt != rep["counts"]))
    assert rep["identity_ok"]
    surf = rep["surface"]
    if surf.any():
        print(f"covariances {which} n={len(pts)} {kw}: structure {rep['structure'].max():.2e} residual "
              f"{rep['residual'].max():.2e} small-gap {np.mean(rep['gap'][surf] < 1e-2):.4f}")
        assert rep["structure"].max() <= 1e-12, rep["structure"].max()
        assert rep["residual"].max() <= RESIDUAL_BOUND, (rep["residual"].max(), int(np.argmax(rep["residual"])))
        wide = surf & (rep["gap"] >= 1e-2)
        assert np.sum(surf & ~wide) <= max_left_out * len(pts)
        assert rep["entry_err"][wide].max(initial=0.0) <= 1e-8, rep["entry_err"][wide].max()
    assert np.all(rep["entry_err"][~surf] == 0)
    return rep


def graph_rows_cover_their_radius(pts, idx, rad):
    """The property of test_target_graph_rows_cover_their_radius for EVERY row, by brute force in fp64: rows
    hold distinct other points, real entries first, nearest first; every other point strictly inside radius[i]
    is in row i.  (A row whose ties overflowed has radius 0 and covers nothing: test_graph_rows_on_the_lattice.)"""
    n = len(pts)
    assert idx.shape == (n, _lib.GRAPH_K) and rad.shape == (n,)
    assert np.all(np.isfinite(rad)) and np.all(rad >= 0)
    assert np.all((idx >= -1) & (idx < n))
    real = idx >= 0
    assert np.all(real[:, :-1] >= real[:, 1:])                      # real entries first, then the -1 pads
    for lo in range(0, n, 512):
        rows = np.arange(lo, min(n, lo + 512))
        d2 = np.zeros((len(rows), n))
        for a in range(pts.shape[1]):
            d2 += (pts[rows, a][:, None] - pts[None, :, a]) ** 2
        d2[np.arange(len(rows)), rows] = np.inf
        inrow = np.zeros((len(rows), n + 1), dtype=np.int32)
        np.add.at(inrow, (np.arange(len(rows))[:, None], np.where(real[rows], idx[rows], n)), 1)
        inrow = inrow[:, :n]
        assert inrow.max(initial=0) <= 1, "a row holds a point twice"
        assert not np.any(inrow[np.arange(len(rows)), rows]), "a row holds its own point"
        missing = (d2 < (rad[rows] ** 2)[:, None]) & (inrow == 0)
        assert not np.any(missing), (int(missing.sum()), rows[np.nonzero(missing.any(axis=1))[0][:5]])
        d = np.sqrt(np.take_along_axis(d2, np.where(real[rows], idx[rows], rows[:, None]), axis=1))
        d = np.where(real[rows], d, 0.0)                               # (the pads' entries are not compared)
        both = real[rows][:, 1:]                                       # (real entries come first)
        assert np.all(np.diff(d, axis=1)[both] >= -1e-6 * (1.0 + d[:, 1:][both])), "not nearest first"


def planar_lattice(seed=3):
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.5
    pts = np.concatenate([g, np.zeros((len(g), 1))], axis=1)
    return pts[np.random.default_rng(seed).permutation(len(pts))]


def ladder_params(dim, **kw):
    return gicp.default_params(dim, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0, **kw)


def ladder_pose(src):
    """A 1.5 degree turn about the cloud's centre plus a centimetre-scale shift."""
    dim = src.shape[1]
    if dim == 2:
        return E.pose_about(src.mean(axis=0), O.rot2(np.deg2rad(1.5)), [0.02, -0.01])
    return E.pose_about(src.mean(axis=0), S.axis_angle([1.0, -2.0, 0.5], np.deg2rad(1.5)), [0.02, -0.01, 0.015])
