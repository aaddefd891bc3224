"""NumPy restatement of the registration report (include/gicp_hip.h "registration report"), written
from the definitions: the per-point Jacobians J_i = [[p_i]x, -I] (2-D: [-J2 p_i, -I]) of the left perturbation
T' = Exp(xi) T, H = sum J^T W J and b = sum J^T W r over the accepted points, the overlap table, and the lower
order statistics of the distances and of the whitened residuals.  Nothing here touches the engine;
test_report_cpu.py checks these helpers on their own."""
import numpy as np
from scipy.linalg import expm

from oracle import gicp_oracle as O

J2 = np.array([[0.0, -1.0], [1.0, 0.0]])


def twist_size(d):
    return 6 if d == 3 else 3


def hat(xi, d):
    """The (d+1) x (d+1) matrix of the twist xi = (omega, v): 3-D (w_x, w_y, w_z, v_x, v_y, v_z), 2-D (w, v_x, v_y)."""
    X = np.zeros((d + 1, d + 1))
    if d == 3:
        X[:3, :3] = O.skew(xi[:3])
        X[:3, 3] = xi[3:]
    else:
        X[:2, :2] = xi[0] * J2
        X[:2, 2] = xi[1:]
    return X


def perturbed(T, xi):
    """Exp(xi) T: the left perturbation."""
    return expm(hat(np.asarray(xi, dtype=np.float64), T.shape[0] - 1)) @ T


def jacobians(p):
    """J_i = d r_i / d xi at the moved points p [n, d]: [n, d, 6] (2-D: [n, 2, 3])."""
    n, d = p.shape
    J = np.zeros((n, d, twist_size(d)))
    if d == 3:
        J[:, 0, 1], J[:, 0, 2] = -p[:, 2], p[:, 1]          # [p]x, row by row
        J[:, 1, 0], J[:, 1, 2] = p[:, 2], -p[:, 0]
        J[:, 2, 0], J[:, 2, 1] = -p[:, 1], p[:, 0]
        J[:, :, 3:] = -np.eye(3)
    else:
        J[:, :, 0] = -(p @ J2.T)                            # -J2 p
        J[:, :, 1:] = -np.eye(2)
    return J


def accepted(src, q, W, idx, T):
    """(p, r, W) of the accepted points at pose T."""
    ok = idx >= 0
    p = O.apply_transformation(src[ok], T)
    return p, q[ok] - p, W[ok]


def information_ref(src, q, W, idx, T):
    """(H, b) as the per-point sums."""
    p, r, Wa = accepted(src, q, W, idx, T)
    J = jacobians(p)
    H = np.einsum("nai,nab,nbj->ij", J, Wa, J)
    b = np.einsum("nai,nab,nb->i", J, Wa, r)
    return H, b


def frozen_loss(src, q, W, idx, T):
    """sum r^T W r at pose T with the correspondences and weights held."""
    _, r, Wa = accepted(src, q, W, idx, T)
    return float(np.einsum("na,nab,nb->", r, Wa, r))


def whitened(src, q, W, idx, T):
    """s_i = sqrt(max(r_i^T W_i r_i, 0)) of the accepted points."""
    _, r, Wa = accepted(src, q, W, idx, T)
    return np.sqrt(np.maximum(np.einsum("na,nab,nb->n", r, Wa, r), 0.0))


def overlap_ref(dist, idx, thresholds):
    """(inliers, inlier_sum_sq) per threshold: accepted points with dist <= tau (inclusive)."""
    d = np.asarray(dist)[np.asarray(idx) >= 0]
    cnt = np.array([int(np.sum(d <= t)) for t in thresholds], dtype=np.int64)
    ssq = np.array([float(np.sum(d[d <= t] ** 2)) for t in thresholds])
    return cnt, ssq


def lower_quantile(v, pi):
    """The value at index floor(pi (n - 1)) of v sorted ascending (the product in fp64); NaN for no values."""
    v = np.sort(np.asarray(v, dtype=np.float64))
    if len(v) == 0:
        return float("nan")
    return float(v[int(np.floor(pi * (len(v) - 1)))])


def report_ref(src, q, W, idx, dist, T, thresholds=(), quantiles=()):
    """The report of a pass given its correspondences idx, matches q, weights W (already w W with a robust
    kernel) and distances dist at pose T, in the layout of Engine.evaluate."""
    d = src.shape[1]
    nw = twist_size(d) - d
    ok = idx >= 0
    H, b = information_ref(src, q, W, idx, T)
    cnt, ssq = overlap_ref(dist, idx, thresholds)
    s = whitened(src, q, W, idx, T)
    p, r, _ = accepted(src, q, W, idx, T)
    eig, vec = np.linalg.eigh(0.5 * (H + H.T))
    er, vr = np.linalg.eigh(H[:nw, :nw])
    et, vt = np.linalg.eigh(H[nw:, nw:])
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.where(cnt > 0, np.sqrt(ssq / np.maximum(cnt, 1)), np.nan)
    return dict(dim=d, n_source=len(src), n_matched=int(ok.sum()), sum_sq=float(np.sum(r * r)),
                loss=frozen_loss(src, q, W, idx, T), H=H, b=b, eig=eig, eigvec=vec, eig_rot=er, vec_rot=vr,
                eig_trans=et, vec_trans=vt, inliers=cnt, inlier_sum_sq=ssq, fitness=cnt / float(len(src)),
                inlier_rmse=rmse, dist_q={pi: lower_quantile(np.asarray(dist)[ok], pi) for pi in quantiles},
                white_q={pi: lower_quantile(s, pi) for pi in quantiles})


def matches(tgt, idx):
    """q [n, d]: the matched target point of every accepted row, zeros elsewhere."""
    q = np.zeros((len(idx), tgt.shape[1]))
    q[idx >= 0] = tgt[idx[idx >= 0]]
    return q
