"""NumPy reference of the robust kernels (include/gicp_hip.h GICP_ROBUST_*): the weight
functions, one pass with W~ = w W, the fixed-iteration IRLS loop, and the outlier scene the robust tests
share.  Nothing here touches the engine; test_robust_cpu.py checks these helpers on their own."""
import numpy as np

import edge_ref as E
from oracle import gicp_oracle as O

KINDS = {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3, "tukey": 4}
ROBUST = ("huber", "cauchy", "geman_mcclure", "tukey")


def weight(kind, e, c):
    """w of the kernel `kind` (a name of KINDS or its code) at e = r^T W r (clamped at 0), scale c."""
    kind = KINDS.get(kind, kind)
    e = np.maximum(np.asarray(e, dtype=np.float64), 0.0)
    c2 = c * c
    if kind == 0:
        return np.ones_like(e)
    if kind == 1:
        s = np.sqrt(e)
        return np.where(s <= c, 1.0, c / np.where(s > 0, s, 1.0))
    if kind == 2:
        return 1.0 / (1.0 + e / c2)
    if kind == 3:
        g = c2 / (c2 + e)
        return g * g
    if kind == 4:
        g = 1.0 - e / c2
        return np.where(e < c2, g * g, 0.0)
    raise ValueError(kind)


def whitened_sq(src, q, W, idx, T):
    """e_i = r_i^T W_i r_i at pose T (0 for rejected points)."""
    r = q - O.apply_transformation(src, T)
    e = np.einsum("na,nab,nb->n", r, W, r)
    return np.where(idx >= 0, e, 0.0)


def reweight(src, tgt, idx, W, T, kind, c):
    """(q, e, w, w W) of a pass's correspondences `idx` and plain weights W at pose T."""
    q = np.zeros_like(src)
    q[idx >= 0] = tgt[idx[idx >= 0]]
    e = whitened_sq(src, q, W, idx, T)
    w = np.where(idx >= 0, weight(kind, e, c), 0.0)
    return q, e, w, W * w[:, None, None]


def pass_reference(src, tgt, T, d_c, C_s, C_t, model="plane_to_plane", cnt_t=None, min_neighbors=None,
                   kind="none", c=1.0):
    """edge_ref.pass_reference with W multiplied by the kernel's w before the statistics.  Returns
    (idx, dist, w W, statistics, e, w); e and w are those of the plain weights."""
    idx, dist, W, _ = E.pass_reference(src, tgt, T, d_c, C_s, C_t, model, cnt_t, min_neighbors)
    q, e, w, Ww = reweight(src, tgt, idx, W, T, kind, c)
    return idx, dist, Ww, O.stats(src, q, Ww, idx, T), e, w


def loop(src, tgt, kind, c, d_c, d_n, iterations, model="plane_to_plane", T0=None, clouds=None):
    """The fixed-iteration IRLS loop: per iteration the oracle's correspondences and weights of `model` at T_k
    (source covariances rotated), w frozen at T_k, then the exact inner minimiser O.inner_gn of
    sum w r^T W r.  `clouds` = (C_s, C_t, cnt_t) saves recomputing the covariances.  Returns (T, [T_0..])."""
    d = src.shape[1]
    if clouds is None:
        C_s, _ = O.covariances(src, d_n)
        C_t, cnt_t = O.covariances(tgt, d_n)
    else:
        C_s, C_t, cnt_t = clouds
    T = np.eye(d + 1) if T0 is None else np.array(T0, dtype=np.float64)
    poses = [T]
    for _ in range(iterations):
        idx, _, Ww, _, _, _ = pass_reference(src, tgt, T, d_c, C_s, C_t, model, cnt_t, None, kind, c)
        q = np.zeros_like(src)
        q[idx >= 0] = tgt[idx[idx >= 0]]
        T, _ = O.inner_gn(src, q, Ww, idx, T)
        poses.append(T)
    return T, poses


# ----------------------------------------------------------------------------- the outlier scene
OUTLIER_DC, OUTLIER_DN, OUTLIER_ITERS = 0.5, 1.0, 25
OUTLIER_SHIFT = (0.12, 0.10, 0.08)
# robust_scale per covariance model, in units of the whitened residual: plane-to-plane 0.01 is 4.5 cm along
# the normal (x sqrt(20)), point-to-point 0.05 is 5 cm; Tukey cuts off at c, so it takes three times the scale
OUTLIER_SCALE = {"plane_to_plane": 0.01, "point_to_point": 0.05}


def outlier_scale(kind, model):
    return OUTLIER_SCALE[model] * (3.0 if KINDS.get(kind, kind) == 4 else 1.0)


def outlier_scene(n=3000, seed=5, frac=0.2, sigma=0.005):
    """(source, target, T_gt): n points of synthetic.room_scene() (the 40 x 40 x 8 m room of scene_pair_3d; at
    n = 3000 about 1 m apart, so most covariances are the isolated point's identity); the target is the posed
    source plus `sigma` noise, and the `frac` of it nearest one of its points -- an object that moved between
    the scans -- is shifted by OUTLIER_SHIFT."""
    from gicp import synthetic as S
    rng = np.random.default_rng(seed)
    scene = S.room_scene()
    world = scene.sample(n, rng)
    T_gt = S.gt_transform_3d(deg=1.0, t=(0.06, -0.04, 0.02))
    src = (world - T_gt[:3, 3]) @ T_gt[:3, :3]
    tgt = world + rng.normal(0, sigma, world.shape)
    centre = tgt[rng.integers(n)]
    moved = np.argsort(np.linalg.norm(tgt - centre, axis=1))[:int(frac * n)]
    tgt[moved] += np.asarray(OUTLIER_SHIFT)
    return src, tgt, T_gt
