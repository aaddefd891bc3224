"""The clouds' 48-byte point records (x, y, z, m0, m1, m2): what k_corr, the covariance getters and the sharded build
read from them is what the separate position and covariance arrays gave.

`a` of C = a I - m m^T is no longer stored: it is the epsilon the cloud was built with, or 1 for an isolated point,
which the record marks.  Every case is held, bit for bit, to tests/golden/point_record/point_record_parent.npz: the
raw words (large arrays: row checksums and a SHA-256, point_record_cases.py) the build before the records gave on an
MI355X (scripts/make_point_record_golden.py), and to the oracle where the case says so."""
import os

import numpy as np
import pytest

import edge_ref as E
import point_record_cases as K
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")

# (in a directory of its own: every tests/golden/*.npz is taken for a fixture captured from the reference)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_record", "point_record_parent.npz")


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same_words(got, golden, key):
    got = K.words(got)
    want = golden[key]
    assert want.dtype == np.uint64 and want.shape == got.shape, (key, want.dtype, want.shape, got.shape)
    diff = np.nonzero(got.ravel() != want.ravel())[0]
    assert len(diff) == 0, (key, diff.tolist()[:8], got.ravel()[diff][:8].view(np.float64).tolist(),
                            want.ravel()[diff][:8].view(np.float64).tolist())


def same_digest(a, golden, key):
    rows = K.row_sums(a)
    bad = np.nonzero(rows != golden[key + ".rows"])[0]
    assert len(bad) == 0, (key, "rows that differ", bad.tolist()[:16], np.asarray(a)[bad[:2]].tolist())
    assert np.array_equal(K.sha(a), golden[key + ".sha"]), key


def oracle_covariances(pts, d_n, eps, ratio):
    return O.covariances(pts, d_n, epsilon=eps, ratio=K.ratio_value(ratio))[0]


# ----------------------------------------------------------------------------- 1: decode of a and m
@pytest.fixture(scope="module")
def decode_clouds():
    """The 2000-point pairs and the oracle's covariances of both clouds at both ratios, computed once."""
    out = {}
    for d in (2, 3):
        src, tgt, iso_s, iso_t = K.isolated_pair(d, K.DEC_N)
        cov = {rk: (oracle_covariances(src, K.DEC_D_N, K.EPS_SRC, r), oracle_covariances(tgt, K.DEC_D_N, K.EPS_TGT, r))
               for rk, r in K.RATIOS.items()}
        out[d] = (src, tgt, iso_s, iso_t, cov)
    return out


@pytest.mark.parametrize("model", K.MODELS)
@pytest.mark.parametrize("rk", list(K.RATIOS))
@pytest.mark.parametrize("dim", [2, 3])
def test_decode(eng, golden, decode_clouds, dim, rk, model):
    """Source epsilon 1e-3, target 4e-3, at least 50 isolated points a cloud, ratio default and 1: both clouds'
    covariances bit-equal to the golden and within 1e-10 of the oracle's; one pass's statistics, indices and weights
    bit-equal to the golden."""
    src, tgt, iso_s, iso_t, cov = decode_clouds[dim]
    ratio = K.RATIOS[rk]
    ps = K.params(gicp, dim, K.EPS_SRC, ratio, K.DEC_D_C, K.DEC_D_N, model)
    pt = K.params(gicp, dim, K.EPS_TGT, ratio, K.DEC_D_C, K.DEC_D_N, model)
    st, dbg = K.engine_pass(gicp, eng, src, tgt, K.decode_pose(dim, src), ps, pt)
    C_s, C_t = eng.covariances("source"), eng.covariances("target")
    eye = np.eye(dim)
    for name, C, iso, ref in (("source", C_s, iso_s, cov[rk][0]), ("target", C_t, iso_t, cov[rk][1])):
        ident = np.all(C == eye, axis=(1, 2))
        assert iso.sum() >= 50 and np.all(ident[iso]), (name, int(iso.sum()), np.nonzero(iso & ~ident)[0].tolist())
        err = np.max(np.abs(C - ref))
        print(f"{name}: {int(ident.sum())} identity rows, covariances vs oracle {err:.2e}")
        assert err <= 1e-10, (name, err)
        same_digest(C, golden, f"decode_{dim}d_{rk}.cov_{name}")
    if ratio == 1.0:   # m = 0 for every surface point, a still epsilon: C = epsilon I exactly, never the isolated mark
        assert np.all(C_s[~np.all(C_s == eye, axis=(1, 2))] == K.EPS_SRC * eye)
        assert np.all(C_t[~np.all(C_t == eye, axis=(1, 2))] == K.EPS_TGT * eye)
    key = f"decode_{dim}d_{rk}_{model}"
    # surface and isolated points on both sides of accepted pairs
    idx = dbg["index"]
    acc = idx >= 0
    assert np.sum(acc & iso_s) >= 50 and np.sum(iso_t[idx[acc]]) >= 50 and np.sum(acc & ~iso_s) >= 500
    assert np.array_equal(idx.astype(np.int32), golden[key + ".index"]), key
    same_words(st, golden, key + ".stats")
    same_digest(dbg["weight"], golden, key + ".weight")


# ----------------------------------------------------------------------------- 2: epsilon travels with the cloud
@pytest.mark.parametrize("dim", [2, 3])
def test_epsilon_travels_with_the_cloud(eng, dim):
    """A target built with epsilon 4e-3 is promoted to source, then another target is set with 1e-3: the pass equals,
    bit for bit, the one of the same clouds set directly with those parameters."""
    tgt, src, _, _ = K.isolated_pair(dim, K.DEC_N)       # (the pair's source is the later target)
    p4 = K.params(gicp, dim, K.EPS_TGT, None, K.DEC_D_C, K.DEC_D_N)
    p1 = K.params(gicp, dim, K.EPS_SRC, None, K.DEC_D_C, K.DEC_D_N)
    T = K.decode_pose(dim, src)
    eng.set_target(src, p4)
    eng.target_to_source()
    eng.set_target(tgt, p1)
    st, dbg = eng.iterate(T, debug=True)
    C_s, C_t = eng.covariances("source"), eng.covariances("target")
    eng.set_target(tgt, p1)
    eng.set_source(src, p4)
    st2, dbg2 = eng.iterate(T, debug=True)
    assert np.sum(dbg2["index"] >= 0) >= 500
    assert np.array_equal(dbg["index"], dbg2["index"])
    assert np.array_equal(K.words(st), K.words(st2)), (st - st2).tolist()
    assert np.array_equal(K.words(dbg["weight"]), K.words(dbg2["weight"]))
    assert np.array_equal(K.words(C_s), K.words(eng.covariances("source")))
    assert np.array_equal(K.words(C_t), K.words(eng.covariances("target")))
    surf = ~np.all(C_s == np.eye(dim), axis=(1, 2))
    assert np.allclose(np.trace(C_s[surf], axis1=1, axis2=2), K.EPS_TGT * (dim - 1 + O.RATIO), rtol=1e-9)


# ----------------------------------------------------------------------------- 3: sharded build
@pytest.mark.parametrize("dim", [2, 3])
def test_sharded_build(eng, golden, dim):
    """The source built as shard 0 and as shard 1 of 2: the other shard's rows of covariances("source") are NaN, the
    own rows bit-equal to the unsharded build's, isolated rows the identity; the shards' statistics summed in rank
    order equal the golden."""
    src, tgt, iso_s, _ = K.isolated_pair(dim, K.SHARD_N)
    ps = K.params(gicp, dim, K.EPS_SRC, None, K.DEC_D_C, K.DEC_D_N)
    pt = K.params(gicp, dim, K.EPS_TGT, None, K.DEC_D_C, K.DEC_D_N)
    T = K.decode_pose(dim, src)
    K.engine_pass(gicp, eng, src, tgt, T, ps, pt)
    whole = eng.covariances("source")
    assert np.all(np.isfinite(whole))
    parts, own = [], []
    for r in (0, 1):
        st, _ = K.engine_pass(gicp, eng, src, tgt, T, ps, pt, shard=r, nshards=2)
        C = eng.covariances("source")
        rot = eng.rotated_covariances(T[:dim, :dim], "source")
        nan = np.all(np.isnan(C), axis=(1, 2))
        assert np.all(nan | np.all(np.isfinite(C), axis=(1, 2)))            # a row is NaN throughout or not at all
        assert np.array_equal(np.all(np.isnan(rot), axis=(1, 2)), nan)
        assert np.array_equal(K.words(C[~nan]), K.words(whole[~nan]))
        assert np.all(C[iso_s & ~nan] == np.eye(dim))                      # isolated, not "not computed"
        parts.append(st)
        own.append(~nan)
    print(f"own rows {own[0].sum()} + {own[1].sum()}, isolated among them {np.sum(iso_s & own[0])} + {np.sum(iso_s & own[1])}")
    assert np.all(own[0] ^ own[1]) and own[0].sum() >= 64 and own[1].sum() >= 64
    assert np.sum(iso_s & own[0]) + np.sum(iso_s & own[1]) >= 50
    same_words(parts[0] + parts[1], golden, f"shard_{dim}d.stats_sum")


# ----------------------------------------------------------------------------- 4: the lanes' fp32 offsets far from the origin
OFFSET_CASES = {c[0]: c[1:] for c in K.offset_cases()}


@pytest.mark.parametrize("key", list(OFFSET_CASES))
def test_offset_from_record(eng, golden, key):
    """Clouds 1e5 from the origin at 5 cm spacing, source clusters of 1 .. 64 points and sixteen full tiles, three
    poses on one cache: the indices are the oracle's at every pose, statistics and pass_info counts bit-equal to the
    golden.  The walk (cold), the certificates (0.04 mm away) and the graph descent (centimetres away) run in turn.
    At 1e5 a lane's fp32 screen offset is exact only relative to its tile centre: wherever k_corr takes it from (the
    source's rel32, or the record's position minus the centre), these bits pin it."""
    src, tgt, poses = OFFSET_CASES[key]
    n, dim = src.shape
    p = K.params(gicp, dim, K.EPS_SRC, None, K.OFF_D_C, K.OFF_D_N)
    infos = []
    for k, (st, dbg, info) in enumerate(K.moving_sequence(gicp, eng, src, tgt, poses, p)):
        idx, _ = O.correspondences(O.apply_transformation(src, poses[k]), tgt, K.OFF_D_C)
        assert np.array_equal(dbg["index"], idx), (k, np.nonzero(dbg["index"] != idx)[0].tolist())
        assert np.sum(idx >= 0) >= (n + 1) // 2
        same_words(st, golden, f"{key}_p{k}.stats")
        got = {a: float(v) for a, v in zip(K.INFO_KEYS, K.info_words(info).view(np.float64))}
        want = {a: float(v) for a, v in zip(K.INFO_KEYS, golden[f"{key}_p{k}.info"].view(np.float64))}
        assert got == want, (k, got, want)
        infos.append(info)
    if key.endswith("full"):
        assert infos[0]["walked_tiles"] == K.FULL_GROUPS        # one tile per group of 64, every one walks when cold
    assert infos[0]["walked_tiles"] >= 1 and infos[0]["graph_proved"] == 0
    assert infos[1]["walked_tiles"] == 0 and infos[1]["graph_proved"] < n     # lanes kept by their certificates
    assert infos[2]["graph_proved"] >= 1


# ----------------------------------------------------------------------------- 5: record boundaries
@pytest.mark.parametrize("n", K.BND_N)
@pytest.mark.parametrize("dim", [2, 3])
def test_record_boundaries(eng, dim, n):
    """n points a side, n = 1 .. 65: records that straddle 128-byte lines and the allocation's last record.  One pass:
    indices exact, statistics within 1e-9 of the oracle's; both clouds' covariances against the oracle's."""
    src, tgt, T = K.boundary_case(dim, n)
    ps = K.params(gicp, dim, K.EPS_SRC, None, K.BND_D_C, K.BND_D_N)
    pt = K.params(gicp, dim, K.EPS_TGT, None, K.BND_D_C, K.BND_D_N)
    st, dbg = K.engine_pass(gicp, eng, src, tgt, T, ps, pt)
    C_s, C_t = eng.covariances("source"), eng.covariances("target")
    for name, C, pts, eps in (("source", C_s, src, K.EPS_SRC), ("target", C_t, tgt, K.EPS_TGT)):
        ref = oracle_covariances(pts, K.BND_D_N, eps, None)
        err = np.max(np.abs(C - ref))
        print(f"{name}: covariances vs oracle {err:.2e}")
        assert err <= 1e-10, (name, err)
    idx, _, _, ref = E.pass_reference(src, tgt, T, K.BND_D_C, C_s, C_t)
    assert np.array_equal(dbg["index"], idx) and np.all(idx >= 0)
    np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * max(np.max(np.abs(ref)), 1e-300))
    assert np.array_equal(eng.points("source"), src) and np.array_equal(eng.points("target"), tgt)
