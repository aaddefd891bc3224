"""Reference for the motion compensation of a sweep: p' = expm((tau - ref) xi^) p with SciPy's
matrix exponential (Pade approximant with scaling and squaring), one per distinct stamp.  An independent
formulation: no Rodrigues formula, no series, no closed form of the integral -- those are what is under test.
Also the cases the CPU and the GPU tests share."""
import functools

import numpy as np
from scipy.linalg import expm

# |omega| per stamp unit: exact zero, far below and around every threshold a closed form might switch at (the
# library's own switch is at |s omega| = 0.1), a typical sweep, and the largest a quarter turn admits
ANGLES = (0.0, 1e-12, 1e-8, 1e-5, 9e-4, 1.1e-3, 1e-2, 0.3, 1.5)
S_VALUES = (-0.5, 0.0, 0.25, 1.0, 1.7)    # tau - ref: before the reference stamp, at it, beyond one stamp unit
SPEED = 5.0                                # |v| per stamp unit
REF = 0.25                                 # the cases' reference stamp (exact in binary: tau = REF gives s = 0)
BOUND = 1e-12                              # |p' - reference| <= BOUND (1 + max|p| + |s| |v|)


def hat(xi):
    """The (dim+1) x (dim+1) matrix xi^ of a twist: 3-D (w, v) with 6 entries, 2-D (w, v) with 3."""
    xi = np.asarray(xi, dtype=np.float64)
    if len(xi) == 6:
        w, v = xi[:3], xi[3:]
        X = np.zeros((4, 4))
        X[:3, :3] = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
        X[:3, 3] = v
        return X
    X = np.zeros((3, 3))
    X[0, 1], X[1, 0] = -xi[0], xi[0]
    X[:2, 2] = xi[1:]
    return X


def motion_of(xi):
    """M = expm(xi^): the motion over one stamp unit whose twist is xi."""
    return expm(hat(xi))


def deskew_ref(points, stamps, xi, ref):
    """p'_i = expm((stamps_i - ref) xi^) p_i, one matrix exponential per distinct stamp."""
    points = np.asarray(points, dtype=np.float64)
    stamps = np.asarray(stamps, dtype=np.float64)
    d = points.shape[1]
    X = hat(xi)
    out = np.empty_like(points)
    for tau in np.unique(stamps):
        E = expm((tau - ref) * X)
        m = stamps == tau
        out[m] = points[m] @ E[:d, :d].T + E[:d, d]
    return out


def twist(dim, angle, seed):
    """A twist with |omega| = angle and |v| = SPEED, directions from rng(seed)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=dim)
    v *= SPEED / np.linalg.norm(v)
    if dim == 2:
        return np.concatenate([[angle if seed % 2 else -angle], v])
    w = rng.normal(size=3)
    return np.concatenate([w * (angle / np.linalg.norm(w)), v])


@functools.lru_cache(maxsize=None)
def case(dim, angle, n, seed=0):
    """(points, stamps, xi, M, reference): n points in +-50 whose stamps cycle through REF + S_VALUES (so they
    repeat, are negative and exceed 1), the cycle starting at a class-dependent value so that n = 1 meets every
    s over the classes.  Computed once and shared (read only)."""
    k = ANGLES.index(angle)
    rng = np.random.default_rng(1000 * dim + 10 * k + seed)
    pts = rng.uniform(-50.0, 50.0, (n, dim))
    stamps = REF + np.asarray(S_VALUES)[(np.arange(n) + k) % len(S_VALUES)]
    xi = twist(dim, angle, 7 * k + dim + seed)
    out = (pts, stamps, xi, motion_of(xi), deskew_ref(pts, stamps, xi, REF))
    for a in out:
        a.setflags(write=False)
    return out


def check_against_reference(got, pts, stamps, xi, want, what=""):
    """The issue's bound, per point: |p' - reference| <= 1e-12 (1 + max|p| + |s| |v|).  Prints the worst ratio."""
    v = np.linalg.norm(xi[-pts.shape[1]:])
    bound = BOUND * (1.0 + np.max(np.abs(pts)) + np.abs(stamps - REF) * v)
    err = np.max(np.abs(got - want), axis=1)
    print(f"de-skew {what}: max error / bound = {float(np.max(err / bound)):.3e}")
    assert np.all(err <= bound), (what, float(np.max(err / bound)))
