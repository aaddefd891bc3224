"""Every fp32-screen decision of k_corr and k_knn_cov pinned to exact arithmetic on clouds in which every lane
is a near tie of a designed size (tests/near_tie_ref.py; the builders and references are checked on the CPU by
test_near_tie_ref_cpu.py).  The classes: relative gaps in d^2 of 0, 2^-46, 2^-40, 2^-34, 2^-28, 2^-24, 2^-20
(all inside the screen's band: the fp64 re-resolution decides), 2^-16 and 2^-12 (the fp32 screen may decide)."""
import functools

import numpy as np
import pytest

import near_tie_ref as N
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")
from gpu_helpers import RESIDUAL_BOUND, VARIANTS, ladder_pose, make_engine  # noqa: E402

INFO = ("ambiguous", "pairs", "list_rebuilds", "sum_sq", "graph_proved", "walked_tiles")
TURNED_VARIANTS = ("default", "plain", "no_graph", "sparse_amb_0", "sparse_amb_64")


def params(dim, **kw):
    return gicp.default_params(dim, max_distance_correspondence=N.D_C[dim], max_distance_nearest_neighbors=N.D_N[dim],
                               **kw)


@functools.lru_cache(maxsize=None)
def corr_case(dim):
    """(scene, [(name, T, truth)]): the fixture of one dimension and the exact truth at every pose of the sequence,
    computed once (per distinct translation) and shared by every test and variant; nothing changes it."""
    sc = N.corr_scene(dim)
    truths = {}
    seq = []
    for name, T in N.pose_sequence(sc):
        key = float(T[0, -1])
        if key not in truths:
            truths[key] = N.nearest_truth(N.moved_exactly(sc["source"], T), sc["target"], sc["d_c"])
        seq.append((name, T, truths[key]))
    return sc, seq


def by_class(sc, rows):
    """'kind class: wrong of total, ...' of the given rows, for a failure message that says which decision failed
    at which class (a string: pytest prints it whole)."""
    out = []
    for kind in ("pair", "quad", "clump", "boundary"):
        for c in N.CLASSES:
            m = (sc["kind"] == kind) & (sc["cls"] == c)
            k = int(np.sum(m[np.asarray(rows, dtype=np.int64)]))
            if k:
                out.append(f"{kind} {'tie' if c == N.TIE else f'2^{c}'}: {k} of {int(m.sum())}")
    return ", ".join(out)


def check_indices_and_distances(sc, dbg, tr, what, rows=None):
    rows = np.arange(len(tr["index"])) if rows is None else rows
    bad = rows[dbg["index"][rows] != tr["index"][rows]]
    assert len(bad) == 0, f"{what}: {len(bad)} wrong indices -- {by_class(sc, bad)}"
    acc = rows[tr["index"][rows] >= 0]
    err = np.abs(dbg["distance"][acc] - tr["distance"][acc]) / np.spacing(tr["distance"][acc])
    assert np.all(err <= 2), f"{what}: distance off by {err.max():.1f} ulp -- {by_class(sc, acc[err > 2])}"
    rej = rows[tr["index"][rows] < 0]
    fin = np.isfinite(dbg["distance"][rej])
    assert np.all(dbg["distance"][rej][fin] > sc["d_c"]), what


# ============================================================================= k_corr
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_corr_near_ties_along_flips(monkeypatch, variant, dim):
    """Target = pairs + quads (3-D) + clumped pairs + boundary targets, one set_source, then pose_sequence in order
    on the warm context: the identity twice, six translations that each flip the winner of every class up to
    theirs, the identity again.  Per pass the index equals the exact truth everywhere, the distance is within
    2 ulp of the correctly rounded root of the exact d^2 (a d^2 with <= 2 ulp error halves under the root, plus
    the root's own rounding), the count is the exact number accepted, and the statistics match O.stats built
    from the truth indices at check_pass's tolerances.

    The re-resolution must have run: without certificates, lists and graph ('plain') the cold pass's ambiguous
    count is at least the number of accepted pair and quad sources of classes <= 2^-20 (the screen's c = 2^-16
    alone puts them inside the band); with everything on ('default') at least one pass from the first flip on has
    lanes proved by the graph descent (the plain pairs and the quads: near ties the descent resolves in fp64
    from the row, counted in graph_proved) and at least one has ambiguous lanes (the clumped pairs, which no row
    can prove: they walk, and the walk's screen leaves them ambiguous)."""
    sc, seq = corr_case(dim)
    src, tgt, d_c = sc["source"], sc["target"], sc["d_c"]
    assert len(tgt) < 4000 and len(src) < 4000
    p = params(dim)
    e = make_engine(monkeypatch, **VARIANTS[variant])
    infos = []
    try:
        e.set_target(tgt, p)
        e.set_source(src, p)
        C_s, C_t = e.covariances("source"), e.covariances("target")
        for k, (name, T, tr) in enumerate(seq):
            what = f"{dim}-D {variant} pass {k} ({name})"
            st, dbg = e.iterate(T, debug=True)
            info = e.pass_info()
            infos.append(info)
            print(f"{what}: " + ", ".join(f"{key} {info[key]:.6g}" for key in INFO))
            check_indices_and_distances(sc, dbg, tr, what)
            assert st[-1] == int(tr["accepted"].sum()), (what, st[-1])
            W, ref = N.pass_stats_reference(src, tgt, T, tr["index"], C_s, C_t)
            np.testing.assert_allclose(dbg["weight"], W, rtol=1e-9, atol=1e-15, err_msg=what)
            np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-9 * np.max(np.abs(ref)), err_msg=what)
    finally:
        e.close()
    tr0 = seq[0][2]
    designed = np.isin(sc["kind"], ("pair", "quad", "clump")) & (sc["cls"] <= -20) & tr0["accepted"]
    if variant == "plain":
        assert infos[0]["ambiguous"] >= designed.sum(), (infos[0]["ambiguous"], int(designed.sum()))
    if variant == "default":
        after = infos[2:]
        assert any(i["graph_proved"] > 0 for i in after), [i["graph_proved"] for i in after]
        assert any(i["ambiguous"] > 0 for i in after), [i["ambiguous"] for i in after]


@pytest.mark.parametrize("variant", TURNED_VARIANTS)
def test_corr_near_ties_turned(monkeypatch, variant):
    """The 3-D fixture seen through two rotations, two passes each (the second on the warm context).  The exact
    quarter turn about z with a dyadic translation: the source is T^-1 of the tie points, the round trip is exact,
    so every class is held index for index, distances to 2 ulp.  A generic pose (gpu_helpers.ladder_pose): the
    truth is taken at the fp64 moved points of O.apply_transformation, whose rounding moves d^2 by about 2^-47
    relative, so the sources whose exact gap there is >= 2^-40 are held index for index (at least 60 % of them,
    every class 2^-40 ... 2^-20 among them: test_near_tie_ref_cpu.py) and the others to the candidates within
    2^-40 of their nearest (a pair's two points, a quad's corners); a boundary row there is held to its truth
    unless its distance lies within 2^-40 of d_c."""
    sc, seq = corr_case(3)
    tgt, d_c = sc["target"], sc["d_c"]
    p = params(3)
    src_q, T_q = N.quarter_turn(sc)
    tr_q = seq[0][2]
    T_g = ladder_pose(sc["source"])
    src_g, tr_g = N.generic_case(sc, T_g)
    e = make_engine(monkeypatch, **VARIANTS[variant])
    try:
        e.set_target(tgt, p)
        e.set_source(src_q, p)
        for rep in range(2):
            st, dbg = e.iterate(T_q, debug=True)
            check_indices_and_distances(sc, dbg, tr_q, f"{variant} quarter turn pass {rep}")
            assert st[-1] == int(tr_q["accepted"].sum())
        e.set_source(src_g, p)
        near_dc = np.abs(tr_g["distance"] - d_c) < d_c * 2.0 ** -40
        firm = tr_g["compared"] & ~near_dc
        assert firm.mean() >= 0.6
        for rep in range(2):
            what = f"{variant} generic pose pass {rep}"
            st, dbg = e.iterate(T_g, debug=True)
            info = e.pass_info()
            print(f"{what}: " + ", ".join(f"{key} {info[key]:.6g}" for key in INFO))
            rows = np.nonzero(firm)[0]
            bad = rows[dbg["index"][rows] != tr_g["index"][rows]]
            assert len(bad) == 0, f"{what}: {len(bad)} wrong indices -- {by_class(sc, bad)}"
            acc = firm & (tr_g["index"] >= 0)
            # p' itself may differ by an ulp of a coordinate between the kernel and NumPy here: check_pass's rtol
            np.testing.assert_allclose(dbg["distance"][acc], tr_g["distance"][acc], rtol=1e-12, err_msg=what)
            for i in np.nonzero(~firm)[0]:
                got = int(dbg["index"][i])
                assert got in tr_g["allowed"][i] or (near_dc[i] and got == -1), \
                    f"{what}: row {i} ({by_class(sc, [i])}) -> {got}"
                assert got >= 0 or near_dc[i], (what, i)
    finally:
        e.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_corr_near_d_c(monkeypatch, dim):
    """The boundary rows (one isolated target each, the source at exactly d_c (1 + eta) from it, eta = 0 and
    +-2^c for the ladder) across the pose sequence: accepted iff the exact distance is <= d_c -- the sideways
    translations add t^2 to these d^2, so the truth is the pose's own -- and a rejected row gives index -1 and a
    zero weight."""
    sc, seq = corr_case(dim)
    rows = np.nonzero(sc["kind"] == "boundary")[0]
    p = params(dim)
    e = make_engine(monkeypatch)
    try:
        e.set_target(sc["target"], p)
        e.set_source(sc["source"], p)
        seen = set()
        for k, (name, T, tr) in enumerate(seq):
            st, dbg = e.iterate(T, debug=True)
            got = dbg["index"][rows] >= 0
            want = tr["accepted"][rows]
            bad = rows[got != want]
            assert len(bad) == 0, \
                f"{dim}-D pass {k} ({name}): {by_class(sc, bad)}, eta {sc['boundary']['eta'][bad - rows[0]]}"
            assert np.array_equal(dbg["index"][rows], tr["index"][rows]), (dim, k, name)
            rej = rows[~want]
            assert np.all(dbg["index"][rej] == -1) and np.all(dbg["weight"][rej] == 0), (dim, k, name)
            assert np.all(np.linalg.det(dbg["weight"][rows[want]]) > 0)
            seen.add(tuple(want))
        assert len(seen) > 1          # the larger flips did reject rows that the identity accepts
        eta = sc["boundary"]["eta"]
        assert np.array_equal(seq[0][2]["accepted"][rows], eta <= 0)
    finally:
        e.close()


# ============================================================================= k_knn_cov
KNN_CASES = [("kth", d, k) for d, k in N.KTH_CASES] + [("dn", 3, 20), ("dn", 2, 6)]


@functools.lru_cache(maxsize=None)
def knn_case(kind, dim, K):
    cl = N.kth_cloud(dim, K) if kind == "kth" else N.dn_cloud(dim)
    return cl, N.exact_neighbourhoods(cl["points"], cl["d_n"], K)


@pytest.fixture(scope="module")
def eng():
    e = gicp.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("which", ["target", "source"])
@pytest.mark.parametrize("kind,dim,K", KNN_CASES, ids=[f"{c}-{d}d-k{k}" for c, d, k in KNN_CASES])
def test_knn_near_ties(eng, kind, dim, K, which):
    """kth_cloud (the K-th against the (K+1)-th neighbour of every cluster centre differ by the ladder, 2^-46 up)
    and dn_cloud (a probe at exactly d_n (1 + eta), eta = 0 and +-2^c) as the target (k_knn_cov with the graph
    build) and as the source (without): neighbour counts equal the exact counts, and the covariances meet
    check_covariances' criteria against the exact neighbourhoods -- structure 1e-12, eigen-residual <=
    RESIDUAL_BOUND, entrywise 1e-8 where the relative eigen-gap is >= 1e-2, with no designed centre left out
    (the 2 % cap applies to the rest).  A wrong competitor moves an entry by >= 0.1 (test_near_tie_ref_cpu.py)."""
    cl, ref = knn_case(kind, dim, K)
    pts = cl["points"]
    p = params(dim, k_neighbors=K)
    if which == "target":
        eng.set_target(pts, p)
    else:
        eng.set_target(pts[:8], p)
        eng.set_source(pts, p)
    C = eng.covariances(which)
    cnt = eng.neighbor_counts(which)
    assert np.all(np.isfinite(C))
    bad = np.nonzero(cnt != ref["count"])[0]
    ctr = cl["centre"]
    assert len(bad) == 0, (len(bad), {f"2^{c}": int(np.sum(np.isin(ctr[cl['cls'] == c], bad))) for c in set(cl["cls"])})
    rep = N.covariance_report_exact(pts, ref, O.EPSILON, O.RATIO, dim, C, cnt)
    surf = rep["surface"]
    assert rep["count_ok"] and rep["identity_ok"] and np.all(surf[ctr])
    print(f"{kind} {dim}-D K={K} {which}: structure {rep['structure'].max():.2e} residual {rep['residual'].max():.2e} "
          f"entry error at the centres {rep['entry_err'][ctr].max():.2e} smallest eigen-gap there "
          f"{rep['gap'][ctr].min():.3f}")
    assert rep["structure"].max() <= 1e-12, rep["structure"].max()
    assert rep["residual"].max() <= RESIDUAL_BOUND, (rep["residual"].max(), int(np.argmax(rep["residual"])))
    wide = surf & (rep["gap"] >= 1e-2)
    assert np.all(wide[ctr]), rep["gap"][ctr].min()
    assert np.sum(surf & ~wide) <= 0.02 * len(pts)
    worst = int(np.argmax(np.where(wide, rep["entry_err"], 0)))
    assert rep["entry_err"][wide].max() <= 1e-8, (rep["entry_err"][worst], worst, worst in set(ctr))
    assert np.all(rep["entry_err"][~surf] == 0)


@pytest.mark.parametrize("cloud", ["pairs", "kth"])
def test_graph_radius_on_near_ties(eng, cloud):
    """The property of test_target_graph_rows_cover_their_radius on clouds of near ties -- every row of the 3-D
    pair cloud and of kth_cloud(3, 20): every other target with fp64 distance < radius[i] is
    in row i, rows hold distinct other points, -1 pads come last; and the radius is positive for at least 90 % of
    the rows, so the property is not vacuous."""
    pts = corr_case(3)[0]["pairs"]["target"] if cloud == "pairs" else knn_case("kth", 3, 20)[0]["points"]
    eng.set_target(pts, params(3))
    idx, rad = eng.graph()
    assert idx.shape == (len(pts), 20) and np.all(rad >= 0) and np.all(np.isfinite(rad))
    diff = pts[:, None, :] - pts[None, :, :]
    d2 = np.zeros((len(pts), len(pts)))
    for a in range(3):
        d2 += diff[:, :, a] * diff[:, :, a]
    np.fill_diagonal(d2, np.inf)
    for i in range(len(pts)):
        row = idx[i][idx[i] >= 0]
        assert i not in row and len(set(row)) == len(row), i
        assert np.all(idx[i][len(row):] < 0), i
        inside = np.nonzero(np.sqrt(d2[i]) < rad[i])[0]
        assert set(inside) <= set(row), (i, rad[i], sorted(set(inside) - set(row)))
    print(f"{cloud}: radius > 0 on {np.mean(rad > 0):.3f} of {len(pts)} rows, median {np.median(rad):.3f}")
    assert np.mean(rad > 0) >= 0.9
