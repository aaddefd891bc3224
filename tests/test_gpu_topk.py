"""GPU tests of the top-k of det(W) (k_top1 / k_top2, gicp_top_weights, the top_* rows of gicp_align_trace) against
tests/topk_ref.py, bit for bit: the last k of a stable argsort of det_closed_form(dbg["weight"]) with dbg["index"]
of the same pass.  Ties are the normal case (point to point: every accepted det is 1; Tukey: accepted rows with
det 0; rejected rows: det 0, target -1), so the fixtures are lattices whose dets are exact powers of two; then
distinct dets and the nesting of the k; the sizes at which a k_top1 thread sees a second and a third row
(kTopBlocks = 256 blocks of 256 threads: n > 65 536, n > 131 072); and the rows of a shard, merged."""
import numpy as np
import pytest

import gpu_helpers as H
import topk_ref as TR

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gicp import synthetic as S  # noqa: E402

POINT_TO_POINT = 1
KS = range(1, 17)
# the offset of a source row from its lattice point at the identity pose, per class: e = |offset|^2 is 0, 0.0625
# and 0.1875 exactly; the last class is shifted out of the lattice's hull and is rejected
OFFSETS = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.25, 0.25, 0.25]])
# det(w I_3) per class: Cauchy, c = 0.25: w = 1 / (1 + e / 0.0625) = 1, 1/2, 1/4; Tukey, c = 0.25: w = (1 - e / 0.0625)^2
# below e = 0.0625 and 0 from there on, so the second and third class are accepted rows with det 0
CLASS_DET = {"none": (1.0, 1.0, 1.0, 0.0), "cauchy": (1.0, 0.125, 0.015625, 0.0), "tukey": (1.0, 0.0, 0.0, 0.0)}
LAYOUTS = {"index_alone": (150, 150, 150, 150),               # every class > 16 rows
           "three_classes": (5, 6, 289, 300),                 # the top 16 under Cauchy: 5 + 6 + 5 of the third
           "ten_accepted": (4, 3, 3, 590)}                    # rejected rows (target -1) fill the front


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


def _lattice(side, rng):
    g = np.stack(np.meshgrid(*(np.arange(float(side)),) * 3, indexing="ij"), -1).reshape(-1, 3)
    return g[rng.permutation(len(g))]


def _tie_scene(side, counts, seed):
    """(src, tgt, cls, match): a side^3 unit lattice in random row order; sum(counts) distinct lattice points in
    random order, row i of class cls[i] offset by OFFSETS[cls[i]], the rows of class 3 shifted by 2 + side along x
    (at least 2 units outside the hull).  match[i]: the target row an accepted row i must find."""
    rng = np.random.default_rng(seed)
    tgt = _lattice(side, rng)
    n = int(sum(counts))
    pick = rng.permutation(len(tgt))[:n]
    cls = np.repeat(np.arange(4), counts)[rng.permutation(n)]
    src = tgt[pick].copy()
    acc = cls < 3
    src[acc] += OFFSETS[cls[acc]]
    src[~acc, 0] += 2.0 + side
    return src, tgt, cls, np.where(acc, pick, -1)


def _params(kernel, **kw):
    if kernel != "none":
        kw.update(robust_kernel=kernel, robust_scale=0.25)
    return gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.5,
                               cov_model=POINT_TO_POINT, **kw)


def _reference_of_pass(e, T, cls, match, kernel):
    """(det, index) of the pass at T after asserting the regime: every row found its lattice point or was
    rejected as built, and the reference dets are the class's exact value, row by row."""
    _, dbg = e.iterate(T, debug=True)
    det = TR.det_closed_form(dbg["weight"])
    assert np.array_equal(dbg["index"], match)
    assert np.array_equal(det, np.asarray(CLASS_DET[kernel])[cls])
    assert not np.any(np.signbit(det))
    return det, dbg["index"]


def _same(got, ref, what):
    for name, a, b in zip(("src", "tgt", "det"), got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, name, a, b)


# a. tie classes, every k ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["none", "cauchy", "tukey"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_tie_classes(eng, layout, kernel):
    counts = LAYOUTS[layout]
    src, tgt, cls, match = _tie_scene(9, counts, seed=11)
    assert len(src) == 600 and len(np.unique(src, axis=0)) == 600
    assert [int(np.sum(cls == c)) for c in range(4)] == list(counts)
    p = _params(kernel)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    T = np.eye(4)
    det, index = _reference_of_pass(eng, T, cls, match, kernel)
    n_one = int(np.sum(det == 1.0))
    if layout == "index_alone":
        assert min(np.unique(det, return_counts=True)[1]) > 16
    elif layout == "three_classes":
        assert n_one == (300 if kernel == "none" else 5)
        if kernel == "cauchy":
            assert len(np.unique(TR.top_reference(det, index, 16)[2])) == 3
        if kernel == "tukey":                                 # det 0 on accepted rows and on rejected ones
            top = TR.top_reference(det, index, 16)
            assert np.sum(top[2] == 0.0) == 11 and np.any(top[1][:11] >= 0)
    else:
        assert int(np.sum(index >= 0)) == 10
        top = TR.top_reference(det, index, 16)
        assert np.all(top[1][:6] == -1) and np.all(top[2][:6] == 0.0) and np.all(top[0][:6] >= 0)
    for k in KS:
        _, si, ti, dt = eng.iterate_top(T, k)
        _same((si, ti, dt), TR.top_reference(det, index, k), (layout, kernel, k))
    for k in (1, 5, 16):                                      # the first pass of align runs at T0
        _, res, tr = eng.align(T, _params(kernel, max_iterations=1), trace=True, top_k=k)
        assert res["iterations"] == 1 and np.array_equal(tr["poses"][0], T)
        _same((tr["top_src"][0], tr["top_tgt"][0], tr["top_det"][0]), TR.top_reference(det, index, k),
              (layout, kernel, "align", k))


# b. distinct values and nesting ---------------------------------------------------------------------------
def _pose3():
    """The pose of test_gpu_extensions.py::test_top_weights_vs_argsort."""
    T = np.eye(4)
    T[:3, :3] = S.axis_angle([1.0, -2.0, 0.5], np.deg2rad(1.5))
    T[:3, 3] = [0.05, -0.02, 0.01]
    return T


@pytest.mark.parametrize("dim", [3, 2])
def test_distinct_values_and_nesting(eng, dim):
    if dim == 3:
        src, tgt, _ = S.scene_pair_3d(3000)
        p = gicp.default_params(3, **H.P3)
        T = _pose3()
    else:
        src, tgt, _ = S.segment_scene_2d(5000)
        p = gicp.default_params(2, **H.P2)
        T = np.eye(3)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    _, dbg = eng.iterate(T, debug=True)
    det = TR.det_closed_form(dbg["weight"])
    assert np.sum(dbg["index"] >= 0) > 16
    _, s16, t16, d16 = eng.iterate_top(T, 16)
    kth = np.sort(det)[::-1]
    for k in KS:
        _, si, ti, dt = eng.iterate_top(T, k)
        _same((si, ti, dt), (s16[-k:], t16[-k:], d16[-k:]), (dim, k))               # nested in the k = 16 rows
        assert np.all(si >= 0) and len(np.unique(si)) == k
        later = (dt[1:] > dt[:-1]) | ((dt[1:] == dt[:-1]) & (si[1:] > si[:-1]))
        assert np.all(later), (dim, k, dt, si)                                      # strictly ascending in (det, src)
        assert np.array_equal(ti, dbg["index"][si])
        # the kernel's det is this formula, contracted or not: about ten roundings of 2^-53 against rtol 1e-12
        np.testing.assert_allclose(dt, det[si], rtol=1e-12, atol=0.0)
        assert np.all(det[si] >= kth[k - 1] * (1.0 - 1e-12)), (dim, k)              # each belongs to the top k


# c. sizes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jittered():
    """A 3000-row target, and 140 001 source rows: target rows drawn at random plus a normal jitter of 0.05 per
    axis.  With d_c = 0.1 (two sigma) about a quarter of the rows is rejected; the sizes are prefixes."""
    tgt = S.scene_pair_3d(3000)[1]
    rng = np.random.default_rng(21)
    src = tgt[rng.integers(0, len(tgt), 140001)] + rng.normal(0.0, 0.05, (140001, 3))
    return src, tgt


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 65536, 65537, 140001])
def test_sizes(eng, jittered, n):
    """65 537 rows: the first size at which a k_top1 thread sees two rows; 140 001: chunks of 547 rows, three rows
    for some threads, which for k = 1 and k = 2 is an insert into a full list.  Point to point: det is 0 or 1."""
    src, tgt = jittered
    src = np.ascontiguousarray(src[:n])
    p = gicp.default_params(3, max_distance_correspondence=0.1, max_distance_nearest_neighbors=1.0,
                            cov_model=POINT_TO_POINT)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    T = np.eye(4)
    _, dbg = eng.iterate(T, debug=True)
    det = TR.det_closed_form(dbg["weight"])
    acc = dbg["index"] >= 0
    assert np.array_equal(det, np.where(acc, 1.0, 0.0))
    print(f"n = {n}: {int(acc.sum())} accepted")
    if n >= 255:
        assert 16 < acc.sum() < n - 16
    for k in (1, 2, 16):
        _, si, ti, dt = eng.iterate_top(T, k)
        ref = TR.top_reference(det, dbg["index"], k)
        if n < k:
            assert np.all(ref[0][:k - n] == -1) and np.all(ref[0][k - n:] >= 0)
        _same((si, ti, dt), ref, (n, k))


# d. shards ------------------------------------------------------------------------------------------------
def test_shards_merge_to_the_whole(monkeypatch):
    """16-point source tiles: a shard chunk is 64 tiles, at most 1024 rows, and the chunks are dealt round-robin
    (gicp_set_source).  A tile's extent is capped, so the lattice's tiles hold fewer than 16 rows and 4000 rows
    make more than 4 chunks: their number comes from the tile count (the tiles that walk on the cold pass of an
    engine without certificates, lists or graph, as test_gpu_edges.py counts them), and with 7 shards the shards
    beyond it are empty."""
    counts = (1000, 1000, 1000, 1000)
    src, tgt, cls, match = _tie_scene(17, counts, seed=13)
    assert len(src) == 4000 and len(np.unique(src, axis=0)) == 4000
    p = _params("cauchy")
    T = np.eye(4)
    plain = H.make_engine(monkeypatch, GICP_SRC_TILE="16", GICP_NO_CERTS="1", GICP_NO_LISTS="1", GICP_NO_GRAPH="1")
    try:
        plain.set_target(tgt, p)
        plain.set_source(src, p)
        plain.iterate(T)
        tiles = int(plain.pass_info()["walked_tiles"])
    finally:
        plain.close()
    nchunks = -(-tiles // 64)
    print(f"{tiles} tiles, {nchunks} chunks")
    assert 4000 / 16 <= tiles and 3 < nchunks < 7             # more chunks than 3 shards, fewer than 7
    e = H.make_engine(monkeypatch, GICP_SRC_TILE="16")
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        det, index = _reference_of_pass(e, T, cls, match, "cauchy")
        whole = {}
        for k in (16, 5):
            whole[k] = e.iterate_top(T, k)[1:]
            _same(whole[k], TR.top_reference(det, index, k), ("unsharded", k))
        for nshards in (3, 7):
            rows = {16: [], 5: []}
            owned = np.zeros(len(src), dtype=np.int32)
            owners = []
            for s in range(nshards):
                e.set_source(src, p, shard=s, nshards=nshards)
                mine = np.all(np.isfinite(e.covariances("source")), axis=(1, 2))
                assert np.all(np.isnan(e.covariances("source")[~mine]))
                owned += mine
                assert mine.sum() <= 1024 * len(range(s, nchunks, nshards))
                for k in (16, 5):
                    st, si, ti, dt = e.iterate_top(T, k)
                    assert st[-1] == np.sum(index[mine] >= 0)
                    # this shard's rows alone: the reference over them, the others' dets NaN on the device
                    rs, rt, rd = TR.top_reference(det[mine], index[mine], k)
                    here = np.nonzero(mine)[0]
                    rs = np.where(rs >= 0, here[np.maximum(rs, 0)], -1) if len(here) else rs
                    _same((si, ti, dt), (rs, rt, rd), (nshards, s, k))
                    assert np.all(mine[si[si >= 0]])
                    if not mine.any():
                        assert np.all(si == -1) and np.all(ti == -1) and np.all(dt == 0.0)
                    rows[k].append((si, ti, dt))
                if mine.any():
                    owners.append(s)
            assert np.all(owned == 1)                         # the shards partition the rows
            print(f"{nshards} shards: owners {owners}")
            assert owners == list(range(min(nshards, nchunks))), owners
            for k in (16, 5):
                _same(gicp._merge_top(rows[k], k), whole[k], (nshards, "merged", k))
                _same(TR.merge_reference(rows[k], k), whole[k], (nshards, "merged by the reference", k))
    finally:
        e.close()
