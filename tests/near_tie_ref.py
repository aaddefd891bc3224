"""Near-tie fixtures and their exact references (test_gpu_near_ties.py; checked by test_near_tie_ref_cpu.py).
Nothing here touches the engine.

Both hot kernels decide in fp32 first and fall back to fp64 where the fp32 answer lies within the screen's
error bound ("Precision model of the fp32 screen").  These clouds make every decision a near
tie of a designed size, and say exactly who wins: every coordinate is a double, hence a dyadic rational, so
all of them are scaled by one power of two to Python ints and squared distances are compared as integers.
Equal distances go to the lower original index (edge_ref.nearest_lowest_index's rule).

The class ladder: the relative gap in d^2 between the winner and the runner-up of a designed decision is
0 (an exact tie) or about 2^c for c in LADDER.  "About": an offset eps = rel d^2 / (2 h) is rounded to a power
of two so that it survives in the coordinate, which moves the gap by a factor below sqrt 2; a class holds the
gaps g with 2^(c-1) < g < 2^(c+1), and the classes are at least 16x apart.  2^-46 is 32x the rounding of a
three-term fp64 sum of squares (<= 2 ulp = 2^-51 relative), so a correct fp64 re-resolution must decide it;
the screen's c = 2^-16 term alone makes every class <= 2^-20 ambiguous in fp32 (a gap below 2 c d^2); 2^-12
lies outside the band."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

import edge_ref as E
from oracle import gicp_oracle as O

TIE = -999                                    # the class of an exact tie (rel = 0)
LADDER = (-46, -40, -34, -28, -24, -20, -16, -12)
CLASSES = (TIE,) + LADDER
FLIPS = (-46, -34, -24, -20, -16, -12)        # pose_sequence: translations by -2 eps_c e_x
GENERIC_FLOOR = Fraction(1, 2 ** 40)          # generic pose: gaps below this are not compared index for index
D_C = {3: 0.5, 2: 20.0}
D_N = {3: 1.0, 2: 25.0}


def in_class(gap, c):
    """Whether the exact relative gap (a Fraction) belongs to class c."""
    c = int(c)
    if c == TIE:
        return gap == 0
    return Fraction(2) ** (c - 1) < gap < Fraction(2) ** (c + 1)


def pow2_round(x):
    """The power of two nearest to x > 0 on the log scale."""
    return 2.0 ** round(math.log2(x))


# ----------------------------------------------------------------------------- exact arithmetic
def common_scale(*arrays):
    """The smallest S with x 2^S an integer for every x of the arrays."""
    s = 0
    for a in arrays:
        for x in np.asarray(a, dtype=np.float64).ravel():
            s = max(s, float(x).as_integer_ratio()[1].bit_length() - 1)
    return s


def to_ints(a, S):
    """x 2^S of every element, as an object array of Python ints (exact)."""
    a = np.asarray(a, dtype=np.float64)
    flat = []
    for x in a.ravel():
        n, d = float(x).as_integer_ratio()
        q, r = divmod(n << S, d)
        assert r == 0
        flat.append(q)
    out = np.empty(a.size, dtype=object)
    out[:] = flat
    return out.reshape(a.shape)


def _sq_int(x, S2):
    """x^2 2^S2 of a double x as a Fraction (an integer whenever S2 is large enough)."""
    return Fraction(x) ** 2 * (1 << S2)


def sqrt_rounded(num, S2):
    """The correctly rounded fp64 square root of the rational num / 2^S2 (num a Python int)."""
    if num == 0:
        return 0.0
    with mp.workprec(600):
        return float(mp.sqrt(mp.mpf(int(num)) / mp.mpf(1 << S2)))


def _preselect(points, target, n_cand):
    """fp64 brute force, coordinate by coordinate: the n_cand nearest targets of every point (unordered)."""
    cand = np.empty((len(points), n_cand), dtype=np.int64)
    for lo in range(0, len(points), 512):
        diff = points[lo:lo + 512, None, :] - target[None, :, :]
        d2 = np.zeros(diff.shape[:2])
        for a in range(diff.shape[2]):
            d2 += diff[:, :, a] * diff[:, :, a]
        if n_cand < len(target):
            cand[lo:lo + 512] = np.argpartition(d2, n_cand - 1, axis=1)[:, :n_cand]
        else:
            cand[lo:lo + 512] = np.arange(len(target))
    return cand


def exact_nearest(points, target, n_cand=8):
    """The n_cand nearest targets of every point in exact order: candidates preselected by fp64 brute force,
    then ordered by (exact integer d^2, original index).  Returns dict(index [n, c], d2 [n, c] Python ints,
    S2: d^2 = d2 / 2^S2)."""
    points = np.asarray(points, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    n_cand = min(n_cand, len(target))
    cand = _preselect(points, target, n_cand)
    S = common_scale(points, target)
    Pi, Ti = to_ints(points, S), to_ints(target, S)
    diff = Pi[:, None, :] - Ti[cand]
    d2 = (diff * diff).sum(axis=2)
    idx = np.empty_like(cand)
    out = np.empty(d2.shape, dtype=object)
    for i in range(len(points)):
        order = sorted(range(n_cand), key=lambda k: (d2[i, k], cand[i, k]))
        idx[i] = cand[i, order]
        out[i] = d2[i, order]
    return dict(index=idx, d2=out, S2=2 * S)


def rel_gap(lo, hi):
    """(hi - lo) / lo of two exact squared distances, a Fraction; infinite (None) when lo is 0."""
    return None if lo == 0 else Fraction(int(hi) - int(lo), int(lo))


def nearest_truth(points, target, d_c):
    """The exact pass truth at the moved points `points` (doubles, taken as exact): dict(
    index: the nearest target by exact arithmetic (lowest original index among equals), -1 where rejected;
    nearest, second: the two nearest whether accepted or not; distance: the correctly rounded square root of the
    exact d^2; gap: the exact relative gap in d^2 between nearest and second (Fractions); third_gap: the same
    between nearest and third; accepted; cand_index, cand_d2 [n, 8]: the eight nearest in exact order and their
    exact d^2 as Python ints).

    Accepted means distance <= d_c (gicp.py:136) with the distance the correctly rounded root of the exact d^2:
    the reference compares an fp64 distance, and a d^2 that exceeds d_c^2 by less than the root's own rounding
    (a 2^-98 relative excess arises when a point at exactly d_c is shifted sideways by 2^-49) has the distance
    d_c itself."""
    nn = exact_nearest(points, target)
    d2, S2 = nn["d2"], nn["S2"]
    dist = np.array([sqrt_rounded(x, S2) for x in d2[:, 0]])
    acc = dist <= d_c
    gap = np.array([rel_gap(a, b) for a, b in zip(d2[:, 0], d2[:, 1])], dtype=object)
    third = np.array([rel_gap(a, b) for a, b in zip(d2[:, 0], d2[:, 2])], dtype=object)
    return dict(index=np.where(acc, nn["index"][:, 0], -1), nearest=nn["index"][:, 0], second=nn["index"][:, 1],
                distance=dist, gap=gap, third_gap=third, accepted=acc, cand_index=nn["index"], cand_d2=d2)


def fp32_nearest(points, target):
    """What a kernel that trusted fp32 would answer: brute force on the coordinates rounded to fp32, the squared
    distance summed in fp32, first index among equal minima."""
    p = np.asarray(points, dtype=np.float32)
    t = np.asarray(target, dtype=np.float32)
    idx = np.empty(len(p), dtype=np.int64)
    for lo in range(0, len(p), 512):
        diff = p[lo:lo + 512, None, :] - t[None, :, :]
        d2 = np.zeros(diff.shape[:2], dtype=np.float32)
        for a in range(diff.shape[2]):
            d2 += diff[:, :, a] * diff[:, :, a]
        idx[lo:lo + 512] = np.argmin(d2, axis=1)
    return idx


def exact_sum(a, b):
    """Whether the fp64 sum a + b of two arrays is exact everywhere."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    s = a + b
    return all(Fraction(float(x)) + Fraction(float(y)) == Fraction(float(z))
               for x, y, z in zip(a.ravel(), b.ravel(), s.ravel()))


# ----------------------------------------------------------------------------- correspondences: the clouds
_PAIR_CFG = {
    # h: pair length along x; grid, spacing, origin: the grid of the pairs' first points; jit: jitter quantum
    # (up to 4 quanta per axis); lat: the lateral offsets of the sources, all of one length, so that a class has
    # one eps.  3-D: |lat|^2 = 25 / 4096, d^2 = 29 / 4096, eps = rel / 16, x within +-1.2 (eps >= 2^-50 survives).
    # 2-D (pixel scale): |lat| = 1, d^2 = 1.25, eps = rel / 2, |x| < 64 (2^-47 survives).
    3: dict(h=2.0 ** -4, grid=(8, 12, 9), spacing=(0.25, 0.375, 0.375), origin=(-1.0, -2.0625, -1.5),
            jit=2.0 ** -7,
            lat=[(0, 3, 4), (0, 4, 3), (0, -3, 4), (0, 4, -3), (0, 3, -4), (0, -4, 3), (0, -3, -4), (0, -4, -3),
                 (0, 5, 0), (0, -5, 0), (0, 0, 5), (0, 0, -5)], lat_unit=2.0 ** -6),
    2: dict(h=1.0, grid=(16, 56), spacing=(8.0, 4.0), origin=(-60.0, -110.0), jit=2.0 ** -3,
            lat=[(0, 1), (0, -1)], lat_unit=1.0),
}


def _pairs_at(a, cfg, rng):
    """b = a + h e_x and one source per pair at mid + lateral + eps e_x, the classes dealt round-robin."""
    n, dim = a.shape
    h = cfg["h"]
    ex = np.zeros(dim)
    ex[0] = 1.0
    b = a + h * ex
    lat = np.asarray(cfg["lat"], dtype=np.float64)[rng.integers(0, len(cfg["lat"]), n)] * cfg["lat_unit"]
    d2 = h * h / 4 + float(np.sum(lat[0] ** 2))
    assert np.all(np.sum(lat ** 2, axis=1) + h * h / 4 == d2)
    cls = np.array([CLASSES[i % len(CLASSES)] for i in range(n)])
    eps_of = {c: (0.0 if c == TIE else pow2_round(2.0 ** c * d2 / (2 * h))) for c in CLASSES}
    eps = np.array([eps_of[c] for c in cls])
    mid = a + (h / 2) * ex
    source = mid + lat + eps[:, None] * ex
    assert np.array_equal(source[:, 0] - mid[:, 0], eps), "an eps did not survive in the coordinate"
    assert exact_sum(mid[:, 0], eps)
    return b, lat, source, cls, eps, eps_of


def pair_cloud(dim, seed=5):
    """Target pairs a, b = a + h e_x on a jittered dyadic grid in shuffled order, so far apart that no third
    target interferes, and one source per pair at mid + lateral + eps e_x: its squared distances to b and a
    differ by exactly 2 h eps, eps = rel d^2 / (2 h) rounded to a power of two, the classes dealt round-robin.
    With eps > 0 the winner is b; an exact tie goes to whichever of a, b has the lower index.
    Returns dict(target, source, pair [n, 2]: the indices of (a, b), cls [n], eps [n], eps_of {class: eps},
    h, dim)."""
    cfg = _PAIR_CFG[dim]
    rng = np.random.default_rng([seed, dim])
    g = np.stack(np.meshgrid(*[np.arange(n) for n in cfg["grid"]], indexing="ij"), -1).reshape(-1, dim)
    a = np.asarray(cfg["origin"]) + g * np.asarray(cfg["spacing"]) + rng.integers(-4, 5, g.shape) * cfg["jit"]
    a = a[rng.permutation(len(a))]
    n = len(a)
    b, _, source, cls, eps, eps_of = _pairs_at(a, cfg, rng)
    both = np.concatenate([a, b])
    perm = rng.permutation(2 * n)                      # target[k] = both[perm[k]]
    inv = np.argsort(perm)
    return dict(target=both[perm], source=source, pair=np.stack([inv[:n], inv[n:]], axis=1), cls=cls, eps=eps,
                eps_of=eps_of, h=cfg["h"], dim=dim)


CLUMP = 22        # more than the graph row's 20 entries


def clump_cloud(dim, seed=10, per_class=3):
    """Pairs as in pair_cloud (same h, lateral offsets and eps, so pose_sequence flips them alike), but a and b
    each carry a clump of 22 further targets at a - c_k lat, b - c_k lat, c_k = (k + 4) / 64: on the far side of
    the source (each at least 8 % farther in d^2 than a and b: outside the band) and all nearer to a (to b) than
    the pair's other point.  So the graph row of a holds its clump and not b, and its radius is the clump's,
    a fraction of the source's distance: no descent from a or b can prove the nearest, and these lanes walk
    and meet the fp32 screen's ambiguity in every pass in which their certificate does not hold -- with
    certificates, lists and graph all on.  They lie beside the pair cloud.
    Returns dict(target, source, pair [n, 2], cls, eps, clump [n, 2, 22]: the clump indices of a and of b)."""
    cfg = _PAIR_CFG[dim]
    rng = np.random.default_rng([seed, dim])
    n = per_class * len(CLASSES)
    k = np.arange(n)
    if dim == 3:
        a = np.stack([-1.0 + 0.25 * (k % 9), -1.0 + 0.5 * (k // 9), np.full(n, 2.5)], axis=1)
    else:
        a = np.stack([-60.0 + 8.0 * (k % 9), -150.0 + 4.0 * (k // 9)], axis=1)
    a = a + rng.integers(-4, 5, a.shape) * cfg["jit"]
    a = a[rng.permutation(n)]
    b, lat, source, cls, eps, eps_of = _pairs_at(a, cfg, rng)
    assert eps_of == pair_cloud(dim)["eps_of"]
    c = (np.arange(CLUMP) + 4) / 64.0
    ca = a[:, None, :] - c[None, :, None] * lat[:, None, :]
    cb = b[:, None, :] - c[None, :, None] * lat[:, None, :]
    allp = np.concatenate([a, b, ca.reshape(-1, dim), cb.reshape(-1, dim)])
    perm = rng.permutation(len(allp))
    inv = np.argsort(perm)
    clump = np.stack([inv[2 * n:2 * n + n * CLUMP].reshape(n, CLUMP), inv[2 * n + n * CLUMP:].reshape(n, CLUMP)],
                     axis=1)
    return dict(target=allp[perm], source=source, pair=np.stack([inv[:n], inv[n:2 * n]], axis=1), cls=cls, eps=eps,
                clump=clump, h=cfg["h"], dim=dim)


def quad_cloud(seed=6, per_class=8):
    """3-D: four targets on a dyadic square of side h = 2^-4 in a plane z = const, the source 5/64 above its
    centre, offset by (eps1, eps2, 0) with eps1 = 2 eps2 and eps2 from the ladder: the corners' squared distances
    are d0^2 + 2 h (0, eps2, 2 eps2, 3 eps2) up to the common eps^2 terms, four candidates inside the band in a
    known order, where the screen keeps two keys.  The quads lie beside the pair cloud (y <= -2.7).
    Returns dict(target, source, quad [n, 4]: the corner indices nearest first by design (++, +-, -+, --),
    cls [n], eps2 [n])."""
    rng = np.random.default_rng(seed)
    h = 2.0 ** -4
    z0 = 5 * 2.0 ** -6
    d2 = 2 * (h / 2) ** 2 + z0 * z0
    n = per_class * len(CLASSES)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(3), np.arange(-(-n // 24)), indexing="ij"), -1).reshape(-1, 3)[:n]
    ctr = np.array([-1.0, -3.5, -0.5]) + g * np.array([0.25, 0.375, 0.5]) + rng.integers(-4, 5, g.shape) * 2.0 ** -7
    ctr = ctr[rng.permutation(n)]
    corners = np.array([[1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]]) * (h / 2)
    tgt = (ctr[:, None, :] + corners[None, :, :]).reshape(-1, 3)
    perm = rng.permutation(len(tgt))
    inv = np.argsort(perm)
    cls = np.array([CLASSES[i % len(CLASSES)] for i in range(n)])
    eps2 = np.array([0.0 if c == TIE else pow2_round(2.0 ** c * d2 / (2 * h)) for c in cls])
    off = np.stack([2 * eps2, eps2, np.full(n, z0)], axis=1)
    source = ctr + off
    assert np.array_equal(source[:, :2] - ctr[:, :2], off[:, :2]), "an eps did not survive in the coordinate"
    return dict(target=tgt[perm], source=source, quad=inv.reshape(n, 4), cls=cls, eps2=eps2, h=h)


def eta_ladder():
    """The signed offsets of a boundary fixture in units of the bound: 0 and +-2^c for the ladder."""
    return [0.0] + [sg * 2.0 ** c for c in LADDER for sg in (1.0, -1.0)]


def boundary_points(d_c, dim=3, seed=7):
    """Isolated targets, at least 2 d_c from each other and from each other's sources (and, laid beside the
    other clouds, from everything else), each with one source at distance exactly d_c + eta along y:
    eta = +-d_c 2^c for the ladder, and 0; three copies of each in 3-D, one in 2-D, where |y| must stay below
    256 for the offsets and |x| below 128 for pose_sequence's translations to be exact.
    Accepted iff eta <= 0 (gicp.py:136, inclusive).  Returns dict(target, source, eta [n] in units of d_c)."""
    rng = np.random.default_rng([seed, dim])
    eta = np.array(eta_ladder() * (3 if dim == 3 else 1))
    n = len(eta)
    eta = eta[rng.permutation(n)]
    k = np.arange(n)
    if dim == 3:
        tgt = np.stack([-6.0 + 3 * d_c * (k % 9), np.full(n, 5.0), -4.0 + 3 * d_c * (k // 9)], axis=1)
    else:
        tgt = np.stack([-123.0 + 41.0 * (k % 7), np.array([160.0, 222.0, -200.0])[k // 7]], axis=1) * (d_c / 20.0)
    tgt[:, 0] += rng.integers(-4, 5, n) * 2.0 ** -5
    src = tgt.copy()
    off = d_c + d_c * eta
    assert all(Fraction(d_c) * (1 + Fraction(float(e))) == Fraction(float(o)) for e, o in zip(eta, off))
    src[:, 1] += off
    assert np.array_equal(src[:, 1] - tgt[:, 1], off) and exact_sum(tgt[:, 1], off)
    return dict(target=tgt, source=src, eta=eta)


def corr_scene(dim, seed=5):
    """The correspondence fixture of one dimension: target = pairs (+ quads in 3-D) + clumped pairs + boundary
    targets, source = their sources in the same order.  Returns dict(target, source, kind [n] in {'pair', 'quad',
    'clump', 'boundary'}, cls [n] (the designed class; TIE for eta = 0, the ladder exponent of |eta| otherwise,
    for the boundary rows), pairs, quads (None in 2-D), clumps, boundary, offsets {kind: first target index},
    d_c, d_n, dim)."""
    pc = pair_cloud(dim, seed)
    parts = [("pair", pc)]
    qc = quad_cloud() if dim == 3 else None
    if qc is not None:
        parts.append(("quad", qc))
    cc = clump_cloud(dim)
    parts.append(("clump", cc))
    bc = boundary_points(D_C[dim], dim)
    parts.append(("boundary", bc))
    target = np.concatenate([p["target"] for _, p in parts])
    source = np.concatenate([p["source"] for _, p in parts])
    kind = np.concatenate([[k] * len(p["source"]) for k, p in parts])
    bcls = np.array([TIE if e == 0 else int(round(math.log2(abs(e)))) for e in bc["eta"]])
    cls = np.concatenate([pc["cls"]] + ([qc["cls"]] if qc is not None else []) + [cc["cls"], bcls])
    off = np.cumsum([0] + [len(p["target"]) for _, p in parts])
    return dict(target=target, source=source, kind=kind, cls=cls, pairs=pc, quads=qc, clumps=cc, boundary=bc,
                offsets=dict(zip([k for k, _ in parts], off[:-1])), d_c=D_C[dim], d_n=D_N[dim], dim=dim)


def pose_sequence(cloud):
    """[(name, T)]: the identity twice (the second pass meets certificates at zero displacement), then the pure
    translations -2 eps_c e_x for c in FLIPS, each of which flips the winner of every pair of a class <= c from
    b to a, then the identity again.  Every moved coordinate s + t is asserted exactly representable, so the
    moved points are known exactly and the truth is computed per pose.  `cloud` is a corr_scene."""
    d = cloud["dim"]
    eps_of = cloud["pairs"]["eps_of"]
    seq = [("identity", np.eye(d + 1)), ("identity again", np.eye(d + 1))]
    for c in FLIPS:
        t = np.zeros(d)
        t[0] = -2.0 * eps_of[c]
        assert exact_sum(cloud["source"][:, 0], t[0]), c
        seq.append((f"flip 2^{c}", E.rigid(d, t=t)))
    seq.append(("identity after the flips", np.eye(d + 1)))
    return seq


def moved_exactly(src, T):
    """The moved points of a pure translation or of the identity, exact by pose_sequence's assertion."""
    d = src.shape[1]
    assert np.array_equal(T[:d, :d], np.eye(d))
    return src + T[:d, d]


def quarter_turn(cloud):
    """(source, T): the exact quarter turn about z with a dyadic translation; the source is T^-1 of the tie
    points and the round trip is exact (asserted), as in the lattice fixture."""
    T = E.rigid(3, E.rot_z90(), [0.25, -0.5, 0.125])
    src = E.inverse_moved(cloud["source"], T)
    assert np.array_equal(O.apply_transformation(src, T), cloud["source"]), "the quarter turn's round trip is not exact"
    return src, T


def generic_case(cloud, T):
    """The tie points seen through a generic pose T: source = T^-1 (tie points) in fp64 and the truth at the fp64
    moved points p' = R s + t of O.apply_transformation, taken as exact.  The rounding of p' (and of the kernel's
    own p', a fused multiply-add away) moves d^2 by about 2^-47 relative, so `compared` marks the sources whose
    exact gap at that p' is >= 2^-40: they are held index for index, the others to `allowed`, the candidates whose
    exact d^2 lies within 2^-40 of the nearest's (a pair's two points, up to all four corners of a quad).
    Returns (source, truth dict with `compared`, `allowed` (a list of sets) and `moved`)."""
    src = E.inverse_moved(cloud["source"], T)
    moved = O.apply_transformation(src, T)
    tr = nearest_truth(moved, cloud["target"], cloud["d_c"])
    tr["compared"] = np.array([g is not None and g >= GENERIC_FLOOR for g in tr["gap"]])
    tr["allowed"] = [{int(j) for j, x in zip(ci, cd) if rel_gap(cd[0], x) < GENERIC_FLOOR}
                     for ci, cd in zip(tr["cand_index"], tr["cand_d2"])]
    tr["moved"] = moved
    return src, tr


def pass_stats_reference(src, tgt, T, idx, C_s, C_t):
    """(W, statistics) of one plane-to-plane pass from the truth indices `idx` (not from O.correspondences)
    and the engine's covariances, as edge_ref.pass_reference builds them."""
    d = src.shape[1]
    R = T[:d, :d]
    W = O.weights(np.einsum("ab,nbc,dc->nad", R, C_s, R), C_t, idx)
    q = np.zeros_like(src)
    q[idx >= 0] = tgt[idx[idx >= 0]]
    return W, O.stats(src, q, W, idx, T)


# ----------------------------------------------------------------------------- neighbourhoods: the clouds
KTH_CASES = ((3, 20), (3, 10), (2, 6), (2, 10))


def _cluster_grid(n, dim, spacing):
    """n cluster centres: two columns in x (so that x stays small and small offsets survive in it), the rest
    of the grid in y (and z)."""
    k = np.arange(n)
    if dim == 3:
        return np.stack([(k % 2 - 0.5) * spacing, (k // 2 % 6 - 2.5) * spacing, (k // 12 - 1.5) * spacing], axis=1)
    return np.stack([(k % 2 - 0.5) * spacing, (k // 2) * spacing], axis=1)


def kth_cloud(dim, K, seed=8, copies=3):
    """Clusters farther than d_n apart, each a centre, K - 2 in-plane neighbours (3-D: in the plane z = 0 around
    it; 2-D: along the line y = 0, gently off it) at distinct radii, and two competitors A = (x_A, 0, z_0) and
    B = (-(x_A + eta), 0, z_0) (2-D: (x_A, y_0), (-(x_A + eta), y_0)) outside all of them, on opposite sides and
    out of plane the same way.  Their squared distances from the centre differ by 2 x_A eta + eta^2, eta = +-rel
    d_A^2 / (2 x_A) rounded to a power of two, the ladder from 2^-46 (exact ties at K: edge_ref.tied_kth_cloud)
    with both signs: whichever is nearer completes the centre's K neighbourhood (self included), and the normal
    tilts the other way if the wrong one is taken.
    Returns dict(points, centre [m], A [m], B [m], neighbours [m, K - 2], cls [m], sign [m], dim, K, d_n)."""
    rng = np.random.default_rng([seed, dim, K])
    d_n = D_N[dim]
    u = d_n / 64                                     # the clusters' dyadic unit: 2^-6 (3-D), 25/64 (2-D)
    combos = [(c, sg) for c in LADDER for sg in (1, -1)] * copies
    m = len(combos)
    ctr = _cluster_grid(m, dim, 2.5 * d_n)
    ctr = ctr[rng.permutation(m)]
    xA, off = 36 * u, 16 * u                         # |A| = 0.62 d_n; the neighbours lie within 0.47 d_n
    dA2 = xA * xA + off * off
    pts, centre, A, B, nbs, cls, sign = [], [], [], [], [], [], []
    for k, (c, sg) in enumerate(combos):
        eta = sg * pow2_round(2.0 ** c * dA2 / (2 * xA))
        while True:
            if dim == 3:
                q = rng.integers(-30 * 16, 30 * 16 + 1, (K - 2, 2)) * (u / 16)
                q = np.concatenate([q, np.zeros((K - 2, 1))], axis=1)
            else:
                q = np.stack([rng.integers(-30 * 16, 30 * 16 + 1, K - 2) * (u / 16),
                              rng.integers(-16, 17, K - 2) * (u / 16)], axis=1)
            r2 = np.sum(q * q, axis=1)
            if np.all(r2 > (4 * u) ** 2) and np.all(r2 < (30 * u) ** 2) and len(set(r2.tolist())) == K - 2:
                break
        a = np.zeros(dim)
        b = np.zeros(dim)
        a[0], a[-1] = xA, off
        b[0], b[-1] = -(xA + eta), off
        assert b[0] + xA == -eta
        local = np.concatenate([np.zeros((1, dim)), q, a[None], b[None]])
        base = len(pts)
        pts.extend(ctr[k] + local)
        assert exact_sum(ctr[k][0], local[:, 0])
        centre.append(base)
        nbs.append(base + 1 + np.arange(K - 2))
        A.append(base + K - 1)
        B.append(base + K)
        cls.append(c)
        sign.append(sg)
    pts = np.array(pts)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    return dict(points=pts[perm], centre=inv[np.array(centre)], A=inv[np.array(A)], B=inv[np.array(B)],
                neighbours=inv[np.array(nbs)], cls=np.array(cls), sign=np.array(sign), dim=dim, K=K, d_n=d_n)


def dn_cloud(dim, seed=9, copies=2):
    """Clusters of min_neighbors + 1 points (a centre and min_neighbors = dim points near it) plus one probe at
    exactly d_n + eta from the centre along y, eta = +-d_n 2^c for the ladder, and 0.  d_n is strict
    (gicp.py:24), so the probe counts for the centre iff eta < 0.  Every member's neighbourhood has a relative
    eigen-gap >= 0.05, so the entrywise covariance criterion leaves nobody out.
    Returns dict(points, centre [m], probe [m], eta [m] in units of d_n, cls [m], dim, d_n)."""
    rng = np.random.default_rng([seed, dim])
    d_n = D_N[dim]
    u = d_n / 64
    eta = np.array(eta_ladder() * copies)
    m = len(eta)
    eta = eta[rng.permutation(m)]
    k = np.arange(m)
    if dim == 3:
        ctr = np.stack([(k % 6 - 2.5) * 3.0 * d_n, (k % 2) * 0.25 * d_n, (k // 6 - 2.5) * 3.0 * d_n], axis=1)
    else:
        ctr = np.stack([k * 3.0 * d_n, (k % 2) * 0.25 * d_n], axis=1)
    pts, centre, probe = [], [], []

    def eigen_gaps(local):
        """The relative eigen-gap of every member's neighbourhood within the cluster (clusters are 3 d_n apart)."""
        d = np.linalg.norm(local[:, None, :] - local[None, :, :], axis=2)      # centre to probe: exact
        out = []
        for j in range(len(local)):
            nb = local[d[j] < d_n]
            if len(nb) >= dim:
                w = np.linalg.eigvalsh(E.sample_covariance(nb))
                out.append((w[1] - w[0]) / w[-1] if w[-1] > 0 else 0.0)
        return out

    for i in range(m):
        off = d_n + d_n * eta[i]
        assert Fraction(d_n) * (1 + Fraction(float(eta[i]))) == Fraction(float(off))
        pr = np.zeros(dim)
        pr[1] = off
        while True:      # distinct radii, and no neighbourhood so thin or so round that its normal is ill-defined
            q = rng.integers(-12 * 16, 12 * 16 + 1, (dim, dim)) * (u / 16)
            r2 = np.sum(q * q, axis=1)
            local = np.concatenate([np.zeros((1, dim)), q, pr[None]])
            if np.all(r2 > (3 * u) ** 2) and len(set(r2.tolist())) == dim and min(eigen_gaps(local)) >= 0.05:
                break
        assert exact_sum(ctr[i][1], off)
        base = len(pts)
        pts.extend(ctr[i] + local)
        centre.append(base)
        probe.append(base + dim + 1)
    pts = np.array(pts)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    cls = np.array([TIE if e == 0 else int(round(math.log2(abs(e)))) for e in eta])
    return dict(points=pts[perm], centre=inv[np.array(centre)], probe=inv[np.array(probe)], eta=eta, cls=cls,
                dim=dim, d_n=d_n)


# ----------------------------------------------------------------------------- neighbourhoods: the reference
def reference_covariance(nb, dim, epsilon=O.EPSILON, ratio=O.RATIO):
    """The oracle's formula (O.covariances, batched form) on one neighbourhood: the normal is the eigenvector of
    the smallest eigenvalue of the sample covariance (2-D: the principal one turned by 90 degrees), and
    C = eps I - eps (1 - ratio) n n^T."""
    S = E.sample_covariance(nb)
    if dim == 2:
        ev, evec = np.linalg.eig(S)
        e = evec[:, np.argmax(ev)]
        nrm = np.array([-e[1], e[0]])
    else:
        nrm = np.linalg.eigh(S)[1][:, 0]
    return epsilon * np.eye(dim) - epsilon * (1 - ratio) * np.outer(nrm, nrm)


def exact_neighbourhoods(points, d_n, k, epsilon=O.EPSILON, ratio=O.RATIO, min_neighbors=None):
    """For every point: the k nearest (self included) strictly within d_n by exact arithmetic, nearest first,
    equal distances by the lower index.  Returns dict(
    index: list of index arrays; count [n];
    gap [n]: the exact relative gap (a Fraction) of the point's deciding comparison -- with more than k points
    within d_n the k-th against the (k+1)-th squared distance, (d2_{k+1} - d2_k) / d2_k; otherwise the squared
    distance nearest to d_n^2 against d_n^2, |d2 - d_n^2| / d_n^2 (5/4, a lower bound, with nothing within 1.5 d_n);
    decided_by [n]: 'kth' or 'dn';
    cov [n, d, d]: reference_covariance of the exact neighbourhood, the identity below min_neighbors)."""
    pts = np.asarray(points, dtype=np.float64)
    n, dim = pts.shape
    mn = dim if min_neighbors is None else min_neighbors
    S = common_scale(pts, [d_n])
    Pi = to_ints(pts, S)
    dn2 = int(_sq_int(d_n, 2 * S))
    # fp64 preselection: everything within 1.5 d_n (the exact test follows), plus the nearest point beyond d_n
    diff = pts[:, None, :] - pts[None, :, :]
    d2f = np.zeros((n, n))
    for a in range(dim):
        d2f += diff[:, :, a] * diff[:, :, a]
    index, count, gap, by = [], np.zeros(n, dtype=np.int64), np.empty(n, dtype=object), []
    cov = np.empty((n, dim, dim))
    for i in range(n):
        cand = np.nonzero(d2f[i] < 2.25 * d_n * d_n)[0]
        dd = Pi[cand] - Pi[i]
        d2 = (dd * dd).sum(axis=1)
        order = sorted(range(len(cand)), key=lambda j: (d2[j], cand[j]))
        cand, d2 = cand[order], d2[order]
        inside = int(sum(1 for x in d2 if x < dn2))
        assert cand[0] == i or d2[0] == 0
        take = min(inside, k)
        index.append(cand[:take])
        count[i] = take
        if inside > k:
            gap[i] = Fraction(int(d2[k]) - int(d2[k - 1]), int(d2[k - 1]))
            by.append("kth")
        else:
            others = [abs(int(x) - dn2) for j, x in enumerate(d2) if cand[j] != i]
            # nothing within 1.5 d_n: whatever lies beyond differs from d_n^2 by more than 1.25 d_n^2
            gap[i] = Fraction(min(others), dn2) if others else Fraction(5, 4)
            by.append("dn")
        cov[i] = reference_covariance(pts[cand[:take]], dim, epsilon, ratio) if take >= mn else np.eye(dim)
    return dict(index=index, count=count, gap=gap, decided_by=np.array(by), cov=cov)


def covariance_report_exact(points, ref, epsilon, ratio, min_neighbors, C, counts):
    """edge_ref.covariance_report's figures with the exact neighbourhoods `ref` in the oracle's place."""
    points = np.asarray(points, dtype=np.float64)
    n, d = points.shape
    surf = ref["count"] >= min_neighbors
    res = np.zeros(n)
    gap = np.ones(n)
    nrm = E.normal_of(C, epsilon, ratio)
    for i in np.nonzero(surf)[0]:
        S = E.sample_covariance(points[ref["index"][i]])
        w = np.linalg.eigvalsh(S)
        if w[-1] > 0:
            res[i] = E.eigen_residual(S, nrm[i])
            gap[i] = (w[1] - w[0]) / w[-1]
    return dict(count_ok=np.array_equal(counts, ref["count"]), structure=E.cov_structure_error(C[surf], epsilon, ratio),
                identity_ok=bool(np.all(C[~surf] == np.eye(d))), residual=res, gap=gap,
                entry_err=np.max(np.abs(C - ref["cov"]), axis=(1, 2)), surface=surf, counts=ref["count"])
