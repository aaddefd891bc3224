"""Plain NumPy / mpmath references and input builders for the edge-case GPU tests
(test_gpu_solve_injected.py, test_gpu_edges.py).  Nothing here touches the engine; test_edge_ref_cpu.py
checks these helpers on their own."""
import itertools

import mpmath as mp
import numpy as np

from oracle import gicp_oracle as O

MP_DIGITS = 50
SOLVE_ANGLES = (0.01, 0.031, 0.032, 0.05, 0.2, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0)
# The host solver (gicp.solve_pose) on every solve_cases() input, measured against solve_reference (the
# worst case per dimension, rounded up; test_edge_ref_cpu.py holds the host to them): max |T - T_ref|,
# |loss - quadratic(T)| / loss_ref with the quadratic evaluated in 50 digits at the solver's own pose, and
# max |R R^T - I|.  The device solve is allowed ten times these, and never less than 1e-12.
HOST_POSE_ERR = {2: 8.9e-10, 3: 7.7e-10}
HOST_LOSS_ERR = {2: 1.2e-10, 3: 4.6e-11}
HOST_ORTH_ERR = {2: 6.7e-16, 3: 1.0e-15}


def device_bound(host_err):
    return max(10.0 * host_err, 1e-12)


# ----------------------------------------------------------------------------- A: the inner solve
def _rot(d, rng, angle):
    if d == 2:
        return O.rot2(angle)
    ax = rng.normal(size=3)
    return O.so3_exp(angle * ax / np.linalg.norm(ax))


def solve_case(d, angle, identity_start, seed=0):
    """n = 300 synthetic correspondences (uniform +-5 points, random SPD W, 0.01 noise, every 17th point
    rejected) whose true motion turns by `angle`, and the pose T_k the solve starts from: the identity, or
    a random pose 0.3 rad and ~1 unit away from it.  Returns (s, q, W, idx, T_k, statistics at T_k)."""
    rng = np.random.default_rng([seed, d, int(round(abs(angle) * 1e6)), int(angle < 0), int(identity_start)])
    n = 300
    s = rng.uniform(-5, 5, (n, d))
    Tg = np.eye(d + 1)
    Tg[:d, :d] = _rot(d, rng, angle)
    Tg[:d, d] = rng.normal(0, 0.3, d)
    q = O.apply_transformation(s, Tg) + rng.normal(0, 0.01, (n, d))
    A = rng.normal(size=(n, d, d))
    W = np.einsum("nij,nkj->nik", A, A) + 0.5 * np.eye(d)
    idx = np.arange(n)
    idx[::17] = -1
    Tk = np.eye(d + 1)
    if not identity_start:
        Tk[:d, :d] = _rot(d, rng, 0.3)
        Tk[:d, d] = rng.normal(0, 1.0, d)
    return s, q, W, idx, Tk, O.stats(s, q, W, idx, Tk)


def solve_cases(d):
    """(angle, identity_start) of every case of section A: the angles, both signs in 2-D, from both starts."""
    angles = SOLVE_ANGLES if d == 3 else tuple(sg * a for a in SOLVE_ANGLES for sg in (1, -1))
    return [(a, ident) for a in angles for ident in (True, False)]


def _mp_quadratic(st, d, Tk):
    H, g, c0, _ = O.expand_stats(np.asarray(st, dtype=np.float64), d)
    nz = d * d + d
    Hm = mp.matrix(nz, nz)
    for i in range(nz):
        for j in range(nz):
            Hm[i, j] = mp.mpf(float(H[i, j]))
    gm = mp.matrix([mp.mpf(float(x)) for x in g])
    zk = mp.matrix([mp.mpf(float(x)) for x in O.pose_vector(np.asarray(Tk, dtype=np.float64))])
    return Hm, gm, mp.mpf(float(c0)), zk


def _mp_pose_vector(R, t, d):
    return mp.matrix([R[a, b] for a in range(d) for b in range(d)] + [t[a] for a in range(d)])


def _mp_generators(d):
    if d == 2:
        return [mp.matrix([[0, -1], [1, 0]])]
    out = []
    for k in range(3):
        e = [0, 0, 0]
        e[k] = 1
        out.append(mp.matrix([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]]))
    return out


def _mp_exp(w, d):
    if d == 2:
        c, s = mp.cos(w[0]), mp.sin(w[0])
        return mp.matrix([[c, -s], [s, c]])
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)


def _mp_tangent(Hm, gm, zk, R, t, d):
    """Tangent gradient and Hessian of the quadratic at (R, t) for the step R <- exp(w) R, t <- t + dt."""
    G = _mp_generators(d)
    M = len(G)
    nr = d * d
    nz = nr + d
    u = Hm * (_mp_pose_vector(R, t, d) - zk) - gm          # grad f = 2 u
    J = mp.matrix(nz, M + d)
    for k in range(M):
        GR = G[k] * R
        for a in range(d):
            for b in range(d):
                J[a * d + b, k] = GR[a, b]
    for a in range(d):
        J[nr + a, M + a] = 1
    grad = 2 * (J.T * u)
    Hs = 2 * (J.T * Hm * J)
    for k in range(M):
        for l in range(M):
            S = (G[k] * G[l] + G[l] * G[k]) * R / 2
            Hs[k, l] += 2 * sum(u[a * d + b] * S[a, b] for a in range(d) for b in range(d))
    return grad, Hs


def mp_quad_loss(st, Tk, T):
    """The closed-form loss of the statistics `st` (taken at T_k) at the pose T, in 50-digit arithmetic."""
    with mp.workdps(MP_DIGITS):
        d = np.asarray(Tk).shape[0] - 1
        Hm, gm, c0, zk = _mp_quadratic(st, d, Tk)
        dz = mp.matrix([mp.mpf(float(x)) for x in O.pose_vector(np.asarray(T, dtype=np.float64))]) - zk
        return float(c0 - 2 * (gm.T * dz)[0] + (dz.T * Hm * dz)[0])


def solve_reference(s, q, W, idx, Tk, st=None):
    """The minimiser over SE(d) of the closed-form quadratic of the statistics at T_k: O.inner_gn's result
    polished by Newton steps in 50-digit arithmetic until the tangent gradient is below 1e-30.  Returns a
    dict: T (rounded to fp64), loss, and, kept in 50 digits for the CPU check, grad_norm (max |tangent
    gradient|), hess_min_eig (smallest eigenvalue of the tangent Hessian), steps, gn_loss (inner_gn's)."""
    d = s.shape[1]
    st = O.stats(s, q, W, idx, Tk) if st is None else st
    T0, f0 = O.inner_gn(s, q, W, idx, Tk)
    with mp.workdps(MP_DIGITS):
        Hm, gm, c0, zk = _mp_quadratic(st, d, Tk)
        R = mp.matrix(d, d)
        for a in range(d):
            for b in range(d):
                R[a, b] = mp.mpf(float(T0[a, b]))
        # inner_gn's rotation is orthonormal to fp64 only: one polar step in 50 digits puts it on SO(d)
        for _ in range(4):
            R = (R + mp.inverse(R).T) / 2
        t = mp.matrix([mp.mpf(float(T0[a, d])) for a in range(d)])
        M = len(_mp_generators(d))
        steps = 0
        for steps in range(1, 41):
            grad, Hs = _mp_tangent(Hm, gm, zk, R, t, d)
            if max(abs(x) for x in grad) < mp.mpf("1e-30"):
                break
            step = mp.lu_solve(Hs, -grad)
            R = _mp_exp([step[k] for k in range(M)], d) * R
            t = t + mp.matrix([step[M + a] for a in range(d)])
        grad, Hs = _mp_tangent(Hm, gm, zk, R, t, d)
        dz = _mp_pose_vector(R, t, d) - zk
        loss = c0 - 2 * (gm.T * dz)[0] + (dz.T * Hm * dz)[0]
        T = np.eye(d + 1)
        for a in range(d):
            for b in range(d):
                T[a, b] = float(R[a, b])
            T[a, d] = float(t[a])
        ev = mp.eigsy(Hs, eigvals_only=True)
        return dict(T=T, loss=float(loss), grad_norm=max(abs(x) for x in grad), hess_min_eig=min(ev),
                    steps=steps, gn_loss=float(f0), gn_T=T0)


def parallel_normal_stats(d=3, seed=1):
    """Point-to-plane statistics with every normal parallel (W = n n^T, one n): the translation block
    sum W is rank one, not positive definite."""
    rng = np.random.default_rng(seed)
    n = 200
    s = rng.uniform(-5, 5, (n, d))
    q = s + rng.normal(0, 0.01, (n, d))
    nrm = np.zeros(d)
    nrm[-1] = 1.0
    W = np.broadcast_to(np.outer(nrm, nrm), (n, d, d)).copy()
    return O.stats(s, q, W, np.arange(n), np.eye(d + 1))


def collinear_stats(seed=2):
    """3-D statistics whose accepted source points all lie on one line through the origin (rotation about
    the line is free: the rotation Hessian is rank deficient); W is SPD."""
    rng = np.random.default_rng(seed)
    n = 200
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    s = rng.uniform(-5, 5, (n, 1)) * u
    Tg = np.eye(4)
    Tg[:3, :3] = O.so3_exp(np.array([0.02, -0.01, 0.03]))
    Tg[:3, 3] = [0.1, -0.05, 0.02]
    q = O.apply_transformation(s, Tg) + rng.normal(0, 0.01, (n, 3))
    A = rng.normal(size=(n, 3, 3))
    W = np.einsum("nij,nkj->nik", A, A) + 0.5 * np.eye(3)
    return O.stats(s, q, W, np.arange(n), np.eye(4))


# ----------------------------------------------------------------------------- B: poses
def rigid(d, R=None, t=None):
    T = np.eye(d + 1)
    if R is not None:
        T[:d, :d] = R
    if t is not None:
        T[:d, d] = t
    return T


def rot_z90():
    """The exact quarter turn about z (entries 0 and +-1)."""
    return np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def inverse_moved(src, T):
    """T^-1 applied to `src`: the cloud that T moves back onto where `src` lies."""
    return O.apply_transformation(src, np.linalg.inv(T))


def pass_reference(src, tgt, T, d_c, C_s, C_t, model="plane_to_plane", cnt_t=None, min_neighbors=None):
    """The oracle's correspondences, distances, weights and statistics of one pass at pose T, from the
    engine's own covariances (which the covariance tests check)."""
    d = src.shape[1]
    moved = O.apply_transformation(src, T)
    idx, dist = O.correspondences(moved, tgt, d_c)
    R = T[:d, :d]
    if model == "plane_to_plane":
        W = O.weights(np.einsum("ab,nbc,dc->nad", R, C_s, R), C_t, idx)
    else:
        W = O.weights_model(np.zeros((len(src), d, d)), C_t, idx, model, cnt_t, min_neighbors)
    q = np.zeros_like(src)
    q[idx >= 0] = tgt[idx[idx >= 0]]
    return idx, dist, W, O.stats(src, q, W, idx, T)


# ----------------------------------------------------------------------------- C: exact ties
def nearest_lowest_index(points, target, d_c):
    """Brute-force fp64 nearest neighbour: squared distances summed coordinate by coordinate, np.argmin
    (the first, i.e. lowest original index, among equal minima); accepted if d <= d_c.  Returns
    (index or -1, distance)."""
    points = np.asarray(points, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    idx = np.empty(len(points), dtype=np.int64)
    dist = np.empty(len(points))
    for lo in range(0, len(points), 1024):
        diff = points[lo:lo + 1024, None, :] - target[None, :, :]
        d2 = np.zeros(diff.shape[:2])
        for a in range(diff.shape[2]):
            d2 += diff[:, :, a] * diff[:, :, a]
        k = np.argmin(d2, axis=1)
        idx[lo:lo + 1024] = k
        dist[lo:lo + 1024] = np.sqrt(d2[np.arange(len(k)), k])
    return np.where(dist <= d_c, idx, -1), dist


LATTICE = (12, 12, 6)
SPACING = 0.5


def lattice_target(seed=11, duplicates=40):
    """The 12 x 12 x 6 lattice of spacing 0.5 (dyadic coordinates) in a fixed shuffled order, then
    `duplicates` exact copies of lattice points appended."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n) for n in LATTICE], indexing="ij"), -1).reshape(-1, 3) * SPACING
    g = g[rng.permutation(len(g))]
    return np.concatenate([g, g[rng.choice(len(g), duplicates, replace=False)]])


def lattice_sources():
    """{'cells': cell centres (8-way ties), 'faces': face centres (4-way), 'edges': edge midpoints (2-way,
    distance exactly 0.25)} of the lattice."""
    nx, ny, nz = LATTICE
    h = SPACING / 2

    def grid(ax, ay, az):
        return np.stack(np.meshgrid(ax, ay, az, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)

    full = [np.arange(n) * SPACING for n in LATTICE]
    half = [np.arange(n - 1) * SPACING + h for n in LATTICE]
    cells = grid(half[0], half[1], half[2])
    faces = np.concatenate([grid(half[0], half[1], full[2]), grid(half[0], full[1], half[2]),
                            grid(full[0], half[1], half[2])])
    edges = np.concatenate([grid(half[0], full[1], full[2]), grid(full[0], half[1], full[2]),
                            grid(full[0], full[1], half[2])])
    return dict(cells=cells, faces=faces, edges=edges)


def lattice_poses():
    """Identity, a dyadic translation by one whole cell, and the exact quarter turn about z with the
    translation that maps the (square in x, y) lattice onto itself."""
    span = (LATTICE[0] - 1) * SPACING
    return dict(identity=np.eye(4), shift=rigid(3, t=[SPACING, -SPACING, SPACING]),
                turn=rigid(3, rot_z90(), [span, 0.0, 0.0]))


def last_accepted_offset():
    """A dyadic offset o (multiples of 1/64, each component at most 12/64, so a lattice point + o has that
    point as its only nearest target) whose squared length d2 = |o|^2 is exact in fp64, is not a perfect
    square, and is the LAST value accepted for d_c = sqrt(d2): sqrt(d2) <= d_c but sqrt(nextafter(d2)) > d_c.
    (For a d_c such as 0.25 the next double above d_c^2 still has a square root that rounds to d_c, so a
    distance of exactly d_c does not tell `<=` from `<` in a test on squared distances; this one does.)
    Returns (o, d2, d_c)."""
    for i, j, k in itertools.product(range(2, 13), repeat=3):
        if len({i, j, k}) < 3:
            continue
        o = np.array([i, -j, k]) / 64.0
        d2 = float(o @ o)
        d_c = float(np.sqrt(d2))
        if d_c * d_c != d2 and float(np.sqrt(np.nextafter(d2, np.inf))) > d_c:
            return o, d2, d_c
    raise AssertionError("no such offset")


# ----------------------------------------------------------------------------- D: covariances
def cov_structure_error(C, epsilon, ratio):
    """Relative distance of the eigenvalues of each C from {eps*ratio, eps, ...} (ascending)."""
    w = np.linalg.eigvalsh(C)
    want = np.full(C.shape[-1], epsilon)
    want[0] = epsilon * ratio
    return np.max(np.abs(w - want) / want, axis=-1)


def normal_of(C, epsilon, ratio):
    """The unit normal m of C = eps I - eps (1 - ratio) m m^T (up to sign), from the matrix entries: the
    largest column of eps I - C."""
    B = epsilon * np.eye(C.shape[-1]) - C
    j = np.argmax(np.einsum("nii->ni", B), axis=1)
    col = B[np.arange(len(C)), :, j]
    nrm = np.linalg.norm(col, axis=1, keepdims=True)
    return col / np.where(nrm > 0, nrm, 1.0)


def sample_covariance(nb):
    c = nb - nb.mean(axis=0)
    return c.T @ c / max(len(nb) - 1, 1)


def eigen_residual(S, n):
    """|S n - (n^T S n) n| / lambda_max(S): how far n is from an eigenvector of S."""
    Sn = S @ n
    return float(np.linalg.norm(Sn - (n @ Sn) * n) / np.linalg.eigvalsh(S)[-1])


def covariance_report(points, d_n, k, epsilon, ratio, min_neighbors, C, counts):
    """Per-point figures of the covariance criteria against the oracle's neighbourhoods:
    dict(count_ok, structure (eigenvalue error where a surface exists), identity_ok (exact I elsewhere),
    residual (eigen-residual of the recovered normal, surface points), gap ((l1 - l0) / l_max of the
    oracle's sample covariance in 3-D, (l1 - l0)/l1 in 2-D), entry_err (max |C - C_oracle|), surface)."""
    points = np.asarray(points, dtype=np.float64)
    n, d = points.shape
    C_or, cnt_or = O.covariances(points, d_n, k, epsilon, ratio, min_neighbors, faithful=False)
    idx, valid, _ = O.neighbourhoods(points, d_n, k)
    surf = cnt_or >= min_neighbors
    res = np.zeros(n)
    gap = np.ones(n)
    nrm = normal_of(C, epsilon, ratio)
    for i in np.nonzero(surf)[0]:
        S = sample_covariance(points[idx[i][valid[i]]])
        w = np.linalg.eigvalsh(S)
        if w[-1] > 0:
            res[i] = eigen_residual(S, nrm[i])
            gap[i] = (w[1] - w[0]) / w[-1]
    return dict(count_ok=np.array_equal(counts, cnt_or), structure=cov_structure_error(C[surf], epsilon, ratio),
                identity_ok=bool(np.all(C[~surf] == np.eye(d))), residual=res, gap=gap,
                entry_err=np.max(np.abs(C - C_or), axis=(1, 2)), surface=surf, counts=cnt_or)


def tied_kth_cloud(seed=4):
    """A 3-D cloud whose first 25 points are point 0 (the origin) and 24 points at exactly the same distance
    from it: every (+-0.5, +-0.25, 0) with the coordinates in any of the axis orders (dyadic, squared
    distance 0.3125 however it is summed); then 400 random points at least 0.9 away from the origin.  With
    k = 20 (self included) 19 of the 24 tied points complete point 0's neighbourhood.
    Returns (points, indices of the tied points)."""
    rng = np.random.default_rng(seed)
    tied = []
    for zero in range(3):
        ax = [a for a in range(3) if a != zero]
        for u, v in ((0.5, 0.25), (0.25, 0.5)):
            for su in (1, -1):
                for sv in (1, -1):
                    p = [0.0, 0.0, 0.0]
                    p[ax[0]], p[ax[1]] = su * u, sv * v
                    tied.append(p)
    far = rng.uniform(-3, 3, (4000, 3))
    far = far[np.linalg.norm(far, axis=1) > 0.9][:400]
    pts = np.concatenate([np.zeros((1, 3)), np.array(tied, dtype=np.float64), far])
    return pts, np.arange(1, 25)


def tied_subset_residuals(pts, tied, take, n):
    """Smallest eigen-residual of the normal n over the sample covariances of {point 0} + every
    `take`-subset of the tied points (the neighbourhoods a k-nearest search may return)."""
    subs = np.array(list(itertools.combinations(tied, take)))             # [n_sub, take]
    nb = np.concatenate([np.zeros((len(subs), 1), dtype=np.int64), subs], axis=1)
    x = pts[nb]                                                            # [n_sub, take + 1, 3]
    c = x - x.mean(axis=1, keepdims=True)
    S = np.einsum("spi,spj->sij", c, c) / take
    Sn = S @ n
    r = np.linalg.norm(Sn - (Sn @ n)[:, None] * n, axis=1) / np.linalg.eigvalsh(S)[:, -1]
    return float(r.min())


# ----------------------------------------------------------------------------- E: sizes
LADDER = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025)
LADDER_PAIRS = [(n, n) for n in LADDER] + [(1, 1025), (1025, 1), (65, 3), (3, 65)]


def dense_patch(d, n_src, n_tgt, seed=0):
    """A dense random patch, about 0.12 apart on average: in 3-D a gently curved square surface, in 2-D
    gently curved rows 2 apart filling a square; source and target are independent samples of it with
    4 mm noise."""
    rng = np.random.default_rng([seed, d, n_src, n_tgt])
    big = max(n_src, n_tgt, 4)
    if d == 3:
        side, rows = 0.12 * big ** 0.5, 1
    else:
        rows = max(1, int(round((0.12 * big / 2.0) ** 0.5)))
        side = 0.12 * big / rows

    def sample(n):
        u = rng.uniform(0, side, n)
        if d == 3:
            v = rng.uniform(0, side, n)
            h = 0.05 * np.sin(u * 1.3) + 0.04 * np.cos(v * 0.9)
            pts = np.stack([u, v, h], axis=1)
        else:
            pts = np.stack([u, 2.0 * rng.integers(0, rows, n) + 0.05 * np.sin(u * 1.3)], axis=1)
        return pts + rng.normal(0, 0.004, (n, d))

    return sample(n_src), sample(n_tgt)


def pose_about(centre, R, t):
    """The rigid motion x -> R (x - centre) + centre + t."""
    centre = np.asarray(centre, dtype=np.float64)
    return rigid(len(centre), R, centre - R @ centre + np.asarray(t, dtype=np.float64))
