"""k_corr's statistics epilogue (LDS transpose of the wave's points, 16x16 fp64 MFMA product, mapping of the
product onto the statistics vector) at every fill of a source tile and at chosen patterns of accepted lanes.

Each case's statistics are held to the oracle's at 1e-9 relative (the tolerance of the other statistics
tests) and, bit for bit, to tests/golden/stats_epilogue/stats_epilogue_parent.npz: the raw 64-bit words the build before
the epilogue's transpose went from four phases of 16 points to two of 32 gave on an MI355X
(scripts/make_stats_epilogue_golden.py).  The summation order of a wave's points is part of the contract."""
import os

import numpy as np
import pytest

import edge_ref as E
import stats_epilogue_cases as K

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")

# (in a directory of its own: every tests/golden/*.npz is taken for a fixture captured from the reference)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_epilogue",
                      "stats_epilogue_parent.npz")


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def run_pass(eng, src, tgt, T, d_c, d_n, model="plane_to_plane"):
    """One cold pass at T: (statistics, accepted mask in input order, pass_info); the statistics and the
    correspondences are checked against the oracle's on the way."""
    st, dbg, info = K.engine_pass(gicp, eng, src, tgt, T, d_c, d_n, model)
    idx, _, _, ref = E.pass_reference(src, tgt, T, d_c, eng.covariances("source"), eng.covariances("target"), model,
                                      eng.neighbor_counts("target"))
    assert np.array_equal(dbg["index"], idx)
    err = np.max(np.abs(st - ref)) / max(np.max(np.abs(ref)), 1e-300)
    print(f"accepted {int(np.sum(idx >= 0))} of {len(src)}, statistics vs oracle {err:.2e} of the largest")
    np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * max(np.max(np.abs(ref)), 1e-300))
    return st, dbg["index"] >= 0, info


def same_bits(st, golden, key):
    got = np.ascontiguousarray(st).view(np.uint64)
    assert golden[key].dtype == np.uint64
    diff = np.nonzero(got != golden[key])[0]
    assert len(diff) == 0, (key, diff.tolist(), st[diff].tolist(), golden[key].view(np.float64)[diff].tolist())


@pytest.mark.parametrize("n", K.FILL_N)
@pytest.mark.parametrize("dim", [2, 3])
def test_fill_ladder(eng, golden, dim, n):
    """A tight cluster of n source points in a 2000-point target, at the identity and at a 1.5 degree pose."""
    src, tgt, poses = K.fill_case(dim, n)
    for k, T in enumerate(poses):
        st, acc, _ = run_pass(eng, src, tgt, T, K.FILL_D_C, K.FILL_D_N)
        assert acc.sum() >= (n + 1) // 2          # the cluster lies on the target
        same_bits(st, golden, f"fill_{dim}d_n{n}_p{k}")


@pytest.mark.parametrize("name", list(K.PATTERNS))
@pytest.mark.parametrize("dim", [2, 3])
def test_acceptance_patterns(eng, golden, dim, name):
    """64-point source tiles in which exactly the pattern's lanes are accepted (stats_epilogue_cases.py: the
    sorted order is the input order, one tile per 64 points)."""
    src, tgt, T, mask = K.pattern_case(dim, name)
    st, acc, info = run_pass(eng, src, tgt, T, K.PAT_D_C, K.PAT_D_N)
    # 16 segments of 64 points, each at least one tile, every tile walks on a cold pass: 16 walks = 16 tiles
    assert info["walked_tiles"] == K.GROUPS, info
    assert np.array_equal(acc, mask), (name, np.nonzero(acc != mask)[0].tolist())
    lanes = acc.reshape(K.GROUPS, K.TILE)
    assert np.all(lanes == lanes[0]) and np.nonzero(lanes[0])[0].tolist() == K.PATTERNS[name]
    same_bits(st, golden, f"pattern_{dim}d_{name}")


@pytest.mark.parametrize("model", K.MODELS)
def test_covariance_models(eng, golden, model):
    """W = I (ICP) and W = n n^T (point to plane) through the same epilogue: the 300-point cluster in 3-D."""
    src, tgt, poses = K.fill_case(3, 300)
    st, acc, _ = run_pass(eng, src, tgt, poses[1], K.FILL_D_C, K.FILL_D_N, model=model)
    assert acc.sum() >= 150
    same_bits(st, golden, f"model_{model}")
