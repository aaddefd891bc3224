"""The near-tie builders and exact references of tests/near_tie_ref.py on their own (no GPU): every designed
decision has its designed gap in exact rational arithmetic, the fixtures tell a kernel that trusts fp32 from one
that does not, nothing undesigned comes near the fp64 floor, and a wrong K-th neighbour would be seen."""
from fractions import Fraction

import numpy as np
import pytest

import edge_ref as E
import near_tie_ref as N
from oracle import gicp_oracle as O


@pytest.fixture(scope="module", params=[3, 2], ids=["3d", "2d"])
def scene(request):
    sc = N.corr_scene(request.param)
    return sc, N.nearest_truth(sc["source"], sc["target"], sc["d_c"])


def test_pairs_have_their_designed_gaps(scene):
    """Every pair source has exactly its class's gap (2 h eps / d_b^2, a rational), the winner is b (the lower
    index of a, b for an exact tie), the runner-up the other one, and the third target is at more than twice the
    squared distance: nothing else comes near the band."""
    sc, tr = scene
    pc = sc["pairs"]
    n = len(pc["source"])
    assert 800 <= n <= 1000 and len(pc["target"]) < 2000 and len(sc["target"]) < 4000
    assert np.all(tr["accepted"][:n])
    a, b = pc["pair"][:, 0], pc["pair"][:, 1]
    tie = pc["cls"] == N.TIE
    assert np.array_equal(tr["nearest"][:n], np.where(tie, np.minimum(a, b), b))
    assert np.array_equal(tr["second"][:n], np.where(tie, np.maximum(a, b), a))
    for c in N.CLASSES:
        m = np.nonzero(pc["cls"] == c)[0]
        assert len(m) >= 90
        assert all(N.in_class(tr["gap"][i], c) for i in m), c
    S = N.common_scale(pc["source"], pc["target"])
    h = Fraction(pc["h"])
    for i in range(0, n, 7):                                   # the closed form, on a sample
        e = Fraction(float(pc["eps"][i]))
        d_b2 = sum((Fraction(float(x)) - Fraction(float(y))) ** 2 for x, y in zip(pc["source"][i], pc["target"][b[i]]))
        assert tr["gap"][i] == 2 * h * e / d_b2
    assert S <= 52
    assert min(tr["third_gap"][:n]) > 1


def test_quads_hold_four_candidates_in_order():
    """The four corners of a quad lie at d0^2 + 2 h eps2 (0, 1, 2, 3) (+ common terms): the exact order is the
    designed one (any order by index for an exact tie), all four within 4x the class's gap, a fifth far away."""
    qc = N.quad_cloud()
    nn = N.exact_nearest(qc["source"], qc["target"])
    for i, c in enumerate(qc["cls"]):
        d2 = [int(x) for x in nn["d2"][i]]
        if c == N.TIE:
            assert d2[0] == d2[3] and list(nn["index"][i][:4]) == sorted(qc["quad"][i])
        else:
            assert list(nn["index"][i][:4]) == list(qc["quad"][i]), i
            assert d2[1] - d2[0] == d2[2] - d2[1] == d2[3] - d2[2] > 0
            assert N.in_class(Fraction(d2[1] - d2[0], d2[0]), c)
        assert d2[4] > 2 * d2[3]


def test_clumped_pairs_cannot_be_proved_from_a_graph_row(scene):
    """The clumped pairs have their class's exact gap and a or b as winner like the plain pairs; the third
    target is >= 8 % farther in d^2 (far outside the band); and each of a, b has its 22 clump points -- more
    than a graph row holds -- nearer than its partner, all within 0.5 h and under half the source's distance to
    a, so neither's row holds the other, and its radius (at most the 22nd neighbour's distance) stays below the
    d(p', a) + d(p', b) that a proof from the row needs."""
    sc, tr = scene
    cc = sc["clumps"]
    rows = np.nonzero(sc["kind"] == "clump")[0]
    off = sc["offsets"]["clump"]
    a, b = cc["pair"][:, 0] + off, cc["pair"][:, 1] + off
    tie = cc["cls"] == N.TIE
    assert set(cc["cls"].tolist()) == set(N.CLASSES)
    assert np.array_equal(tr["nearest"][rows], np.where(tie, np.minimum(a, b), b))
    assert np.array_equal(tr["second"][rows], np.where(tie, np.maximum(a, b), a))
    assert all(N.in_class(g, c) for g, c in zip(tr["gap"][rows], cc["cls"]))
    assert min(tr["third_gap"][rows]) >= Fraction(8, 100)
    tgt = sc["target"]
    for i in range(len(rows)):
        for side, p in enumerate((a[i], b[i])):
            d = np.linalg.norm(tgt - tgt[p], axis=1)
            near = np.argsort(d)[1:N.CLUMP + 1]
            assert set(near) == set(cc["clump"][i, side] + off)
            assert d[near].max() <= 0.5 * cc["h"] and d[near].max() < 0.5 * tr["distance"][rows[i]]


def test_boundary_points_sit_exactly_off_d_c(scene):
    sc, tr = scene
    bc = sc["boundary"]
    d_c = sc["d_c"]
    b = sc["kind"] == "boundary"
    assert np.array_equal(tr["accepted"][b], bc["eta"] <= 0)
    assert set(np.abs(bc["eta"]).tolist()) == {0.0} | {2.0 ** c for c in N.LADDER}
    nn = N.exact_nearest(bc["source"], sc["target"])
    dc2 = Fraction(d_c) ** 2
    for i, e in enumerate(bc["eta"]):
        assert Fraction(int(nn["d2"][i][0]), 1 << nn["S2"]) == dc2 * (1 + Fraction(float(e))) ** 2
        assert Fraction(int(nn["d2"][i][1]), 1 << nn["S2"]) >= 2 * dc2      # no other target near d_c
    lo = sc["offsets"]["boundary"]
    for t in sc["target"][lo:]:                                              # isolated: >= 2 d_c from the rest
        assert np.sort(np.linalg.norm(sc["target"] - t, axis=1))[1] >= 2 * d_c
    # and no other source sees a boundary target within d_c
    lo = sc["offsets"]["boundary"]
    assert np.all(tr["nearest"][~b] < lo)


def test_the_fixture_discriminates(scene):
    """fp32 brute force is wrong for at least a quarter of the pair sources of classes <= 2^-20 (measured: about
    half of every class whose eps is lost in an fp32 coordinate); fp64 coordinate-wise brute force is right for
    every source of every class, 2^-46 included."""
    sc, tr = scene
    n = len(sc["pairs"]["source"])
    f32 = N.fp32_nearest(sc["source"], sc["target"])
    low = np.nonzero((sc["pairs"]["cls"] != N.TIE) & (sc["pairs"]["cls"] <= -20))[0]
    wrong = np.mean(f32[low] != tr["nearest"][low])
    print(f"{sc['dim']}-D: fp32 brute force wrong for {wrong:.3f} of {len(low)} sources of classes <= 2^-20")
    assert wrong >= 0.25
    idx64, dist64 = E.nearest_lowest_index(sc["source"], sc["target"], sc["d_c"])
    assert np.array_equal(idx64, tr["index"])
    assert np.all(np.abs(dist64 - tr["distance"]) <= 2 * np.spacing(tr["distance"]))
    assert n == len(sc["pairs"]["cls"])


def test_pose_sequence_flips_the_classes(scene):
    """Every pose of the sequence keeps the moved points exact (asserted by the builder); at the flip of class c
    every pair of a class <= c (ties included) has a as its winner, every pair of a higher class still b; the
    truth stays within {a, b}, and every gap is an exact tie or at least 2^-47 -- nothing below the fp64 floor."""
    sc, _ = scene
    pc = sc["pairs"]
    n = len(pc["source"])
    a, b = pc["pair"][:, 0], pc["pair"][:, 1]
    seq = N.pose_sequence(sc)
    assert [name for name, _ in seq][:2] == ["identity", "identity again"] and len(seq) == 9
    for (name, T), c in zip(seq[2:8], N.FLIPS):
        tr = N.nearest_truth(N.moved_exactly(sc["source"], T), sc["target"], sc["d_c"])
        low = pc["cls"] <= c                                  # TIE = -999 is among them
        assert np.array_equal(tr["nearest"][:n], np.where(low, a, b)), name
        assert all(g == 0 or g >= Fraction(1, 2 ** 47) for g in tr["gap"]), name
        assert min(tr["third_gap"][:n]) > 1
        # the boundary rows: d^2 = (d_c (1 + eta))^2 + t^2 exactly, so a sideways shift can reject a point that
        # lay just inside; accepted is the exact comparison wherever d^2 is 2^-50 or more away from d_c^2
        # (relative), and a d^2 that exceeds d_c^2 by 2^-52 or less has the fp64 distance d_c itself (the rows
        # with eta = 0: an excess of t^2 / d_c^2 = 2^-96 ... 2^-52 at the smaller flips)
        dc2, t2 = Fraction(sc["d_c"]) ** 2, Fraction(float(T[0, -1])) ** 2
        for i, e in zip(np.nonzero(sc["kind"] == "boundary")[0], sc["boundary"]["eta"]):
            excess = ((1 + Fraction(float(e))) ** 2 * dc2 + t2) / dc2 - 1
            assert abs(excess) >= Fraction(1, 2 ** 50) or (e == 0 and 0 < excess <= Fraction(1, 2 ** 52)), (name, i)
            assert tr["accepted"][i] == (excess <= Fraction(1, 2 ** 52)), (name, i)


def test_quarter_turn_round_trip_is_exact():
    sc = N.corr_scene(3)
    src, T = N.quarter_turn(sc)
    assert np.array_equal(O.apply_transformation(src, T), sc["source"])
    assert np.array_equal(T[:3, :3], E.rot_z90())


def test_generic_pose_keeps_enough_of_the_ladder():
    """At gpu_helpers.ladder_pose the fp64 moved points carry their own rounding (about 2^-47 of d^2), so only
    gaps >= 2^-40 at those points are compared index for index: they are at least 60 % of the sources and still
    hold every designed class 2^-40 ... 2^-20; the others' gaps are so small that both candidates are their
    pair (all within 2^-40 of the nearest: the pair's two points, or up to four corners of a quad)."""
    from gpu_helpers import ladder_pose
    sc = N.corr_scene(3)
    T = ladder_pose(sc["source"])
    src, tr = N.generic_case(sc, T)
    share = tr["compared"].mean()
    print(f"generic pose: {share:.3f} of {len(src)} sources compared index for index")
    assert share >= 0.60
    pk = sc["kind"] == "pair"
    for c in (-40, -34, -28, -24, -20):
        m = pk & (sc["cls"] == c) & tr["compared"]
        assert m.sum() >= 10, c
        assert all(N.in_class(g, c) for g in tr["gap"][m]), c   # the pose's rounding did not move them out
    n = len(sc["pairs"]["source"])
    pair = np.sort(sc["pairs"]["pair"], axis=1)
    two = np.sort(np.stack([tr["nearest"][:n], tr["second"][:n]], axis=1), axis=1)
    assert np.array_equal(two, pair)
    # what a source that is not compared may return: its pair's two points, a quad's corners -- never more
    for i in np.nonzero(~tr["compared"])[0]:
        assert tr["nearest"][i] in tr["allowed"][i]
        assert 2 <= len(tr["allowed"][i]) <= (4 if sc["kind"][i] == "quad" else 2)
    for i in np.nonzero(tr["compared"])[0]:
        assert tr["allowed"][i] == {int(tr["nearest"][i])}


@pytest.mark.parametrize("dim,K", N.KTH_CASES, ids=[f"{d}d-k{k}" for d, k in N.KTH_CASES])
def test_kth_cloud(dim, K):
    """The centre's K-th against (K+1)-th comparison is A against B with the designed gap and the designed winner;
    every other point's deciding comparison has a relative gap >= 2^-40; a wrong choice is observable: the
    reference covariance with A and the one with B differ entrywise by >= 1e-3 epsilon, 10^5 x the 1e-8 entry
    tolerance of check_covariances; and the exact neighbourhoods are the oracle's (cKDTree), counts and all."""
    kc = N.kth_cloud(dim, K)
    pts = kc["points"]
    assert len(pts) < 4000
    ref = N.exact_neighbourhoods(pts, kc["d_n"], K)
    ctr = kc["centre"]
    assert set(kc["cls"].tolist()) == set(N.LADDER) and set(kc["sign"].tolist()) == {1, -1}
    worst = np.inf
    for i, c in enumerate(ctr):
        assert ref["decided_by"][c] == "kth" and ref["count"][c] == K
        assert N.in_class(ref["gap"][c], kc["cls"][i]), (i, float(ref["gap"][c]))
        win, lose = (kc["A"][i], kc["B"][i]) if kc["sign"][i] > 0 else (kc["B"][i], kc["A"][i])
        assert ref["index"][c][-1] == win and lose not in ref["index"][c]
        assert set(ref["index"][c][:-1]) == {c} | set(kc["neighbours"][i])
        other = np.concatenate([ref["index"][c][:-1], [lose]])
        diff = np.max(np.abs(N.reference_covariance(pts[other], dim) - ref["cov"][c]))
        worst = min(worst, diff)
    print(f"kth_cloud({dim}, {K}): covariance with the wrong competitor differs by >= {worst:.3g}")
    assert worst >= 1e-3 * O.EPSILON
    rest = np.setdiff1d(np.arange(len(pts)), ctr)
    assert min(ref["gap"][rest]) >= Fraction(1, 2 ** 40)
    C_or, cnt_or = O.covariances(pts, kc["d_n"], K, faithful=False)
    assert np.array_equal(cnt_or, ref["count"])
    assert np.max(np.abs(C_or - ref["cov"])) <= 1e-9


@pytest.mark.parametrize("dim", [3, 2])
def test_dn_cloud(dim):
    """The probe lies at exactly d_n (1 + eta) from its centre and counts iff eta < 0 (strict); the centre has a
    surface either way (min_neighbors + 1 points without the probe); every other decision has a gap >= 2^-40."""
    dc = N.dn_cloud(dim)
    pts = dc["points"]
    ref = N.exact_neighbourhoods(pts, dc["d_n"], O.default_k(dim))
    assert set(np.abs(dc["eta"]).tolist()) == {0.0} | {2.0 ** c for c in N.LADDER}
    for i, c in enumerate(dc["centre"]):
        e = Fraction(float(dc["eta"][i]))
        assert (dc["probe"][i] in ref["index"][c]) == (e < 0)
        assert ref["count"][c] == dim + 1 + (e < 0) and ref["decided_by"][c] == "dn"
        assert ref["gap"][c] == abs(2 * e + e * e)               # |(d_n (1 + eta))^2 - d_n^2| / d_n^2
    designed = np.concatenate([dc["centre"], dc["probe"]])       # the probe's own nearest-to-d_n is its centre
    rest = np.setdiff1d(np.arange(len(pts)), designed)
    assert min(ref["gap"][rest]) >= Fraction(1, 2 ** 40)
    for i, p in enumerate(dc["probe"]):
        assert ref["gap"][p] == ref["gap"][dc["centre"][i]] or ref["gap"][p] >= Fraction(1, 2 ** 40)
