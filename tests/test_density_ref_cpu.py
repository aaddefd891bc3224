"""CPU preconditions of tests/density_ref.py: every property of the fixtures that test_gpu_density.py relies
on, from the oracle and NumPy alone.  No GPU is used."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import density_ref as D
import edge_ref as E
from oracle import gicp_oracle as O


@pytest.mark.parametrize("name", D.FIXTURES)
def test_fixtures_are_what_they_say(name):
    f = D.fixture(name)
    assert f is D.fixture(name) and not f["source"].flags.writeable
    sizes = {"stretched_3d": (8000, 12), "offset_origin_3d": (8000, 12), "halo_3d": (6000, 2000),
             "lidar_small": (8000, 0), "stretched_2d": (6000, 12)}[name]
    for which in ("source", "target"):
        pts, core = f[which], f["core_" + which]
        assert pts.shape == (sum(sizes), f["dim"]) and (int(core.sum()), int((~core).sum())) == sizes
        assert np.all(np.isfinite(pts))
        # shuffled: the extra rows are spread over the cloud, not at its end
        if sizes[1]:
            assert np.nonzero(~core)[0].min() < len(pts) // 4 and np.nonzero(~core)[0].max() > 3 * len(pts) // 4
    extra_s, extra_t = f["source"][~f["core_source"]], f["target"][~f["core_target"]]
    if sizes[1]:
        assert not np.array_equal(np.sort(extra_s, axis=0), np.sort(extra_t, axis=0))      # each cloud has its own
    if name in ("stretched_3d", "stretched_2d"):
        half, low = (D.FAR_3D, 60.0) if name == "stretched_3d" else (D.FAR_2D, 3000.0)
        for x in (extra_s, extra_t):
            assert np.all(x.min(axis=0) == -(half + low)) and np.all(x.max(axis=0) == half)
            assert np.any(np.all(x == -(half + low), axis=1)) and np.any(np.all(x == half, axis=1))
            d = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2)
            assert d[~np.eye(len(x), dtype=bool)].min() > f["d_n"]           # every far point is alone
    if name == "offset_origin_3d":
        for x in (extra_s, extra_t):
            assert np.linalg.norm(x, axis=1).max() < 1.0 and len(np.unique(x, axis=0)) == D.N_FAR
        room = D.fixture("stretched_3d")
        rows = lambda a: a[np.lexsort(a.T)]      # noqa: E731  (each fixture has its own permutation)
        assert np.array_equal(rows(f["source"][f["core_source"]]), rows(room["source"][room["core_source"]] + D.OFFSET))
    if name == "lidar_small":
        rng_ = np.linalg.norm(f["target"], axis=1)
        print(f"lidar_small ranges {rng_.min():.2f} .. {rng_.max():.2f} m")
        assert rng_.min() < 5.0 and 30.0 < rng_.max() < 40.0          # a factor of 7 in range, 50 in density


@pytest.mark.parametrize("name", D.COLLAPSED)
def test_the_grid_collapses_on_the_core(name):
    """All core points of each cloud share one grid cell of the build on every axis, and there are more than
    64 * 64 of them: more than kListMax tiles of 64 points whose boxes all are the core."""
    f = D.fixture(name)
    for which in ("source", "target"):
        cells = D.grid_cells(f[which], f["bits"])
        core = cells[f["core_" + which]]
        assert cells.min() >= 0 and cells.max() <= 2 ** f["bits"] - 1
        print(f"{name} {which}: core cell {core[0]}, {len(core)} points")
        assert np.all(core == core[0]), np.unique(core, axis=0)
        assert len(core) > 64 * 64
        # ... and strictly inside it: a quarter of a percent of a cell from every face at least
        p = f[which]
        lo = p.min(axis=0)
        ext = np.max(p.max(axis=0) - lo) * (1.0 + 1e-9) + 1e-12 * (1.0 + abs(lo[0]))
        frac = (p[f["core_" + which]] - lo) * (2.0 ** f["bits"] / ext) - core[0]
        if name != "offset_origin_3d":          # (there the room lies in the clipped last cell of the y axis)
            assert frac.min() > 0.0025 and frac.max() < 0.9975, (frac.min(), frac.max())


def test_the_halo_grid_keeps_a_few_cells():
    f = D.fixture("halo_3d")
    for which in ("source", "target"):
        cells = D.grid_cells(f[which], f["bits"])
        uniq, cnt = np.unique(cells[f["core_" + which]], axis=0, return_counts=True)
        print(f"halo_3d {which}: the core occupies {len(uniq)} cells, the fullest holds {cnt.max()}")
        assert len(uniq) <= 27 and cnt.max() >= 1000


@pytest.fixture(scope="module")
def trees():
    return {name: cKDTree(D.fixture(name)["target"]) for name in D.FIXTURES}


@pytest.mark.parametrize("name", D.FIXTURES)
def test_acceptance_and_unique_nearest_neighbours_along_the_sequence(trees, name):
    """At every pose of the moving sequence between 25 % and 95 % of the source points are accepted at d_c, and
    no accepted correspondence has an exact tie between distinct targets."""
    f = D.fixture(name)
    poses = D.moving_poses(f)
    assert len(poses) == 8 and np.array_equal(poses[0], np.eye(f["dim"] + 1))
    shares = []
    for k, T in enumerate(poses):
        R = T[:f["dim"], :f["dim"]]
        assert np.max(np.abs(R @ R.T - np.eye(f["dim"]))) < 1e-15
        moved = O.apply_transformation(f["source"], T)
        dist, idx = trees[name].query(moved, k=2)
        ok = dist[:, 0] <= f["d_c"]
        shares.append(float(ok.mean()))
        assert 0.25 <= shares[-1] <= 0.95, (k, shares[-1])
        assert np.all(dist[ok, 0] < dist[ok, 1]), (k, int(np.sum(dist[ok, 0] == dist[ok, 1])))
    print(f"{name}: accepted share per pose {[round(s, 3) for s in shares]}")


@pytest.mark.parametrize("which", ["source", "target"])
@pytest.mark.parametrize("name", D.FIXTURES)
def test_covariance_conditioning(name, which):
    """The share of points whose oracle neighbourhood has a relative eigen-gap below 1e-2 (the entrywise
    covariance comparison leaves them out) is at most 0.20, at least 30 % of the points are surfaces, and the
    count is the constant the GPU test passes to check_covariances."""
    f = D.fixture(name)
    pts, d = f[which], f["dim"]
    C, cnt = O.covariances(pts, f["d_n"], faithful=False)
    rep = E.covariance_report(pts, f["d_n"], O.default_k(d), O.EPSILON, O.RATIO, d, C, cnt)
    surf = rep["surface"]
    left = int(np.sum(surf & (rep["gap"] < 1e-2)))
    print(f"{name} {which}: surfaces {surf.mean():.3f}, eigen-gap below 1e-2 on {left} points ({left / len(pts):.4f}), "
          f"neighbourhoods cut by k {np.mean(cnt == O.default_k(d)):.3f}")
    assert left <= 0.20 * len(pts) and surf.mean() >= 0.30
    assert left == D.LEFT_OUT[name, which]
    assert 0.0 < D.max_left_out(name, which) * len(pts) - left < 1.0
    extra = ~f["core_" + which]
    if name in ("stretched_3d", "stretched_2d"):
        assert np.all(cnt[extra] == 1) and np.all(C[extra] == np.eye(d))        # alone: the identity
    if name == "lidar_small":       # half its neighbourhoods are cut by d_n and half by k
        assert 0.25 < np.mean(cnt == O.default_k(d)) < 0.75
