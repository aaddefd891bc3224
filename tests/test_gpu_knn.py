"""Exact k-nearest-neighbour queries on the GPU (gicp_knn, gicp_knn_points; csrc/gicp_knn.hip) against
the NumPy brute force of the contract (tests/knn_ref.py).  Every comparison is bit for bit: the distances are the
fp64 expression of the contract, the order is (d2, original index), no tolerance is involved.

The cases are knn_ref.cases(): query counts at the wave and workgroup edges, k at every instantiation boundary
(1 | 8 | 16 | 32), databases from one row to a second super-block, exact ties (shuffled lattice, 70 coincident rows),
max_distance on and one ulp below a shell, queries far from and outside the database's frame.  Then the near-tie
fixtures, clouds of uneven density, the cross-checks against k_knn_cov and k_corr, filtered and sharded clouds,
history independence, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import density_ref as D
import knn_ref as K
import near_tie_ref as N
from gpu_helpers import P2, P3, gicp
from gicp import _lib
from gicp import synthetic as S

pytestmark = pytest.mark.gpu

PARAMS = {2: P2, 3: P3}


def params(dim, **kw):
    return gicp.default_params(dim, **{**PARAMS[dim], **kw})


def check(got, want, what):
    idx, d2 = got
    want_i, want_d, want_c = want
    assert K.same_bits(idx, want_i), (what, np.argwhere(idx != want_i)[:5].tolist())
    assert K.same_bits(d2, want_d), (what, np.argwhere(d2 != want_d)[:5].tolist())
    assert np.array_equal((idx >= 0).sum(axis=1), want_c), what


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


def _cases():
    return [(dim, name) for dim in (2, 3) for name in K.case_table(dim, True)]


@pytest.mark.parametrize("dim,name", _cases())
def test_one_shot_equals_the_reference(dim, name):
    _, pts, qs, k, r = K.case_table(dim, True)[name]
    check(gicp.knn(pts, qs, k=k, max_distance=r, squared=True), K.expected(dim, name, True), name)


@pytest.mark.parametrize("dim", [2, 3])
def test_resident_target_equals_the_reference(eng, dim):
    """Engine.knn against a resident target: every case whose database holds at least a tile, each database built
    once (with covariances and graph, which the queries neither need nor touch)."""
    table = K.case_table(dim, True)
    done = 0
    for key in sorted({id(c[1]) for c in table.values() if 64 <= len(c[1]) < 100000}):
        group = [c for c in table.values() if id(c[1]) == key]
        eng.set_target(group[0][1], params(dim))
        for name, pts, qs, k, r in group:
            check(eng.knn(qs, k=k, max_distance=r, squared=True), K.expected(dim, name, True), name)
            done += 1
    assert done >= 30


def test_distances_are_the_square_roots(eng):
    pts, qs = K.lattice(3), K.lattice_queries(3)
    idx2, d2 = gicp.knn(pts, qs, k=9, max_distance=1.0, squared=True)
    idx, d = gicp.knn(pts, qs, k=9, max_distance=1.0)
    assert K.same_bits(idx, idx2) and K.same_bits(d, np.sqrt(d2)) and np.isinf(d[idx < 0]).all()
    # the count output and NULL outputs of the C ABI
    lib = _lib.load()
    cnt = np.full(len(qs), -5, dtype=np.int32)
    rc = lib.gicp_knn_points(gicp._engine(0)._ctx, _lib.dptr(pts), len(pts), _lib.dptr(qs), len(qs), 3, 9, 1.0, None, None,
                             cnt.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0 and np.array_equal(cnt, (idx >= 0).sum(axis=1))


@pytest.mark.parametrize("dim", [2, 3])
def test_near_ties_are_ordered_in_fp64(dim):
    """The near-tie fixtures as database and query sets: rivals the fp32 screen cannot tell apart (gaps down to
    2^-46 relative, and exact ties) come out in the order of the fp64 d2, ties by index."""
    sc = N.corr_scene(dim)
    tgt, src = np.ascontiguousarray(sc["target"]), np.ascontiguousarray(sc["source"])
    for k in (1, 2, 4, 9):
        check(gicp.knn(tgt, src, k=k, squared=True), K.knn(tgt, src, k), ("corr_scene", k))
    check(gicp.knn(tgt, src, k=2, max_distance=sc["d_c"], squared=True), K.knn(tgt, src, 2, sc["d_c"]), "corr_scene d_c")
    kc = np.ascontiguousarray(N.kth_cloud(dim, 6 if dim == 2 else 10)["points"])
    kk = 6 if dim == 2 else 10
    for k in (kk - 1, kk, kk + 1):
        check(gicp.knn(kc, None, k=k, squared=True), K.knn(kc, None, k), ("kth_cloud", k))


@pytest.mark.parametrize("name", ["stretched_3d", "halo_3d"])
def test_uneven_density(name):
    """A collapsed grid (far points stretch the Morton frame: the room falls into a few cells) and a halo (the
    margin is dominated by the cloud's extent): the database stretched, queries from the other cloud of the pair."""
    f = D.fixture(name)
    tgt, src = np.ascontiguousarray(f["target"]), np.ascontiguousarray(f["source"][:700])
    check(gicp.knn(tgt, src, k=8, squared=True), K.knn(tgt, src, 8), name)
    check(gicp.knn(tgt, src, k=1, max_distance=f["d_c"], squared=True), K.knn(tgt, src, 1, f["d_c"]), name)


def _scenes():
    src, tgt, _ = S.scene_pair_3d(4000)
    f = D.fixture("lidar_small")
    return {"room": (src, tgt, 3), "lidar_small": (np.ascontiguousarray(f["source"]), np.ascontiguousarray(f["target"]), 3)}


@pytest.mark.parametrize("scene", ["room", "lidar_small"])
def test_self_query_agrees_with_the_covariance_search(eng, scene):
    """k = k_neighbors, no limit: the rows strictly inside d_n are the neighbours k_knn_cov counted."""
    src, tgt, dim = _scenes()[scene]
    p = params(dim)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    dn = p.max_distance_nearest_neighbors
    for which, pts in (("target", tgt), ("source", src)):
        idx, d2 = eng.knn(k=p.k_neighbors, which=which, squared=True)
        assert np.array_equal((d2 < dn * dn).sum(axis=1), eng.neighbor_counts(which)), which
        check((idx, d2), K.knn(pts, None, p.k_neighbors), (scene, which))


@pytest.mark.parametrize("scene", ["room", "lidar_small"])
def test_nearest_agrees_with_the_correspondence_search(eng, scene):
    src, tgt, dim = _scenes()[scene]
    p = params(dim)
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    dc = p.max_distance_correspondence
    _, dbg = eng.iterate(np.eye(dim + 1), debug=True)
    idx, d2 = eng.knn(eng.points("source"), k=1, max_distance=dc, squared=True)
    _, ref2, _ = K.knn(tgt, src, 2)
    unique = ref2[:, 0] < ref2[:, 1]
    assert unique.sum() > 0.9 * len(src)
    assert np.array_equal(idx[unique, 0], dbg["index"][unique])
    assert (idx[:, 0] >= 0).sum() > 100


def test_filtered_clouds_answer_in_their_own_rows():
    """With set_voxel / set_filter in force the rows and indices are those of Engine.points(which)."""
    src, tgt, _ = S.scene_pair_3d(4000)
    e = gicp.Engine(0)
    try:
        e.set_voxel(1.0)
        e.set_target(tgt, params(3))
        kept = e.points("target")
        assert 64 < len(kept) < len(tgt)
        check(e.knn(src[:300], k=8, squared=True), K.knn(kept, src[:300], 8), "voxel")
        check(e.knn(k=3, squared=True), K.knn(kept, None, 3), "voxel self")
        e.set_voxel(0.0)
        e.set_filter(center=[0.0, 0.0, 0.0], max_range=15.0, radius=1.0, min_neighbors=2)
        e.set_source(src, params(3))
        kept = e.points("source")
        assert 64 < len(kept) < len(src)
        check(e.knn(tgt[:300], k=8, which="source", squared=True), K.knn(kept, tgt[:300], 8), "filter")
    finally:
        e.close()


def test_source_shards_do_not_matter():
    src, tgt, _ = S.scene_pair_3d(4000)
    e = gicp.Engine(0)
    try:
        e.set_target(tgt, params(3))
        e.set_source(src, params(3), shard=1, nshards=2)
        want = K.knn(src, tgt[:500], 8)
        check(e.knn(tgt[:500], k=8, which="source", squared=True), want, "shard 1 of 2")
        check(e.knn(k=2, which="source", squared=True), K.knn(src, None, 2), "shard 1 of 2, self")
    finally:
        e.close()


def test_history_independence():
    """align's poses and statistics do not change with knn calls around and between its passes, and knn does not
    change with what the engine did before."""
    src, tgt, _ = S.scene_pair_3d(4000)
    p = params(3, max_iterations=8)
    qs = K.random_cloud(300, 3, 41, scale=4.0)

    def run(with_knn):
        e = gicp.Engine(0)
        try:
            e.set_target(tgt, p)
            e.set_source(src, p)
            out, T = [], np.eye(4)
            for it in range(3):
                if with_knn:
                    e.knn(qs, k=8)
                    e.knn(k=20, which="source", max_distance=1.0)
                    e.knn_points(src[:900], qs, k=1)
                out.append(e.iterate(T).tobytes())
            if with_knn:
                e.knn(qs, k=32, which="source")
            T1, res = e.align(None, p)
            out += [T1.tobytes(), np.array([res[f] for f in ("iterations", "final_loss", "mse", "correspondences")],
                                           dtype=np.float64).tobytes()]
            return out, e.knn(qs, k=8, squared=True)
        finally:
            e.close()

    plain, after_align = run(False)
    mixed, after_mixed = run(True)
    assert plain == mixed
    want = K.knn(tgt, qs, 8)
    check(after_align, want, "after an align")
    check(after_mixed, want, "after an align with interleaved queries")
    e = gicp.Engine(0)
    try:
        e.set_target(tgt, p)
        first = e.knn(qs, k=8, squared=True)
        check(first, want, "fresh engine")
        check(e.knn(qs, k=8, squared=True), want, "twice")
        e.stage_target(src, p)                      # a staged target pending: its build runs beside the query
        check(e.knn(qs, k=8, squared=True), want, "with a staged target pending")
        e.commit_target()
        check(e.knn(qs, k=8, which="source", squared=True), want, "the former target, now the source")
        check(e.knn(qs, k=8, squared=True), K.knn(src, qs, 8), "the committed target")
    finally:
        e.close()


def _raw(e, which, qs, Q, dim, k, r, idx, d2, cnt):
    return _lib.load().gicp_knn(e._ctx, which, None if qs is None else _lib.dptr(qs), Q, dim, k, r,
                                idx.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(d2), cnt.ctypes.data_as(C.POINTER(C.c_int32)))


def test_refusals_and_recovery():
    lib = _lib.load()
    pts, qs = K.random_cloud(500, 3, 1), K.random_cloud(40, 3, 2)
    bad = qs.copy()
    bad[7, 2] = np.nan
    q2 = np.ascontiguousarray(qs[:, :2])
    e = gicp.Engine(0)
    try:
        idx = np.full((40, 4), 77, dtype=np.int64)
        d2 = np.full((40, 4), 7.5)
        cnt = np.full(40, 77, dtype=np.int32)

        def refused(code, text, *args):
            assert _raw(e, *args, idx, d2, cnt) == code
            assert text in lib.gicp_last_error(e._ctx).decode(), lib.gicp_last_error(e._ctx)
            assert np.all(idx == 77) and np.all(d2 == 7.5) and np.all(cnt == 77)      # a refused call writes nothing

        refused(_lib.GICP_E_STATE, "cloud not set", 0, qs, 40, 3, 4, 0.0)
        refused(_lib.GICP_E_STATE, "cloud not set", 1, None, 0, 0, 4, 0.0)
        e.set_target(pts, params(3))
        refused(_lib.GICP_E_STATE, "cloud not set", 1, qs, 40, 3, 4, 0.0)
        refused(_lib.GICP_E_INVALID, "k must be 1..gicp_knn_max_k()", 0, qs, 40, 3, 0, 0.0)
        refused(_lib.GICP_E_INVALID, "k must be 1..gicp_knn_max_k()", 0, qs, 40, 3, 33, 0.0)
        refused(_lib.GICP_E_INVALID, "dim must be 2 or 3", 0, qs, 40, 4, 4, 0.0)
        refused(_lib.GICP_E_INVALID, "queries must have the cloud's dim", 0, q2, 40, 2, 4, 0.0)
        refused(_lib.GICP_E_INVALID, "Q >= 1", 0, qs, 0, 3, 4, 0.0)
        refused(_lib.GICP_E_INVALID, "non-finite", 0, bad, 40, 3, 4, 0.0)
        refused(_lib.GICP_E_INVALID, "max_distance must be finite and >= 0", 0, qs, 40, 3, 4, -0.5)
        refused(_lib.GICP_E_INVALID, "max_distance must be finite and >= 0", 0, qs, 40, 3, 4, float("inf"))
        refused(_lib.GICP_E_INVALID, "which must be 0 (target) or 1 (source)", 2, qs, 40, 3, 4, 0.0)
        # the one-shot's: M < 1, a non-finite point
        args = (idx.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(d2), cnt.ctypes.data_as(C.POINTER(C.c_int32)))
        assert lib.gicp_knn_points(e._ctx, _lib.dptr(pts), 0, _lib.dptr(qs), 40, 3, 4, 0.0, *args) == _lib.GICP_E_INVALID
        badp = pts.copy()
        badp[3, 0] = np.inf
        assert lib.gicp_knn_points(e._ctx, _lib.dptr(badp), 500, _lib.dptr(qs), 40, 3, 4, 0.0, *args) == _lib.GICP_E_INVALID
        assert "non-finite" in lib.gicp_last_error(e._ctx).decode()
        assert np.all(idx == 77) and np.all(d2 == 7.5) and np.all(cnt == 77)
        # Python raises with the library's text
        with pytest.raises(ValueError, match="k must be 1..gicp_knn_max_k"):
            e.knn(qs, k=0)
        with pytest.raises(ValueError, match="non-finite"):
            gicp.knn(pts, bad, k=2)
        with pytest.raises(ValueError, match="max_distance must be finite"):
            e.knn(qs, k=2, max_distance=-1.0)
        # ... and a valid call afterwards succeeds
        assert _raw(e, 0, qs, 40, 3, 4, 0.0, idx, d2, cnt) == 0
        want = K.knn(pts, qs, 4)
        assert K.same_bits(idx, want[0]) and K.same_bits(d2, want[1]) and K.same_bits(cnt, want[2])
    finally:
        e.close()
