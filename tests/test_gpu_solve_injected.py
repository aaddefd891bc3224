"""The one-wave device solve (k_solve<2>, k_solve<3>: gicp_solve_dev.h, and the device-only sincos_lean of
gicp_solver.h) on injected statistics.  With a host exchange hook set, gicp_align runs k_corr, the hook,
then k_solve and never fuses the solve; the hook replaces the pass's statistics by the ones under test, so
one fixed iteration from T_k returns the device solve of exactly those statistics."""
import numpy as np
import pytest

import edge_ref as E
from oracle import gicp_oracle as O

pytestmark = pytest.mark.gpu

gicp = pytest.importorskip("gicp")


class Injector:
    """An engine holding one-point clouds (so the grid is not empty) whose solve can be fed any statistics."""

    def __init__(self):
        self.eng = gicp.Engine(0)
        self.dim = None

    def solve(self, st, Tk):
        d = Tk.shape[0] - 1
        p = gicp.default_params(d, fixed_iterations=1, max_iterations=1, tolerance=0.0)
        if self.dim != d:
            self.eng.set_target(np.zeros((1, d)), p)
            self.eng.set_source(np.full((1, d), 0.25), p)
            self.dim = d
        n = gicp.stats_size(d)
        st = np.asarray(st, dtype=np.float64)
        assert st.shape == (n,)

        def hook(buf):
            buf[:n] = st

        self.eng.set_allreduce(hook)
        try:
            T, res, tr = self.eng.align(Tk, p, trace=True)
        finally:
            self.eng.set_allreduce(None)
        assert res["iterations"] == 1 and len(tr["losses"]) == 1
        assert np.array_equal(tr["poses"][0], Tk)
        return T, float(tr["losses"][0])

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def inj():
    i = Injector()
    yield i
    i.close()


_CASES = [(d, a, ident) for d in (3, 2) for a, ident in E.solve_cases(d)]


@pytest.mark.parametrize("dim,angle,identity_start", _CASES,
                         ids=[f"{d}d-{a:+g}-{'I' if i else 'Tk'}" for d, a, i in _CASES])
def test_device_solve_vs_polished_reference(inj, dim, angle, identity_start):
    """k_solve on the statistics of 300 synthetic correspondences whose true motion turns by `angle`
    (0.01 ... 3.0 rad: Newton steps on both sides of sincos_lean's 1/32 rad threshold and through all of its
    halvings), from T_k = I and from a random T_k, against the minimiser polished in 50-digit arithmetic.

    Measured on the CPU over these same cases (edge_ref.HOST_*), host solver vs the polished reference:
    pose 8.9e-10 (2-D) / 7.7e-10 (3-D) -- the solver stops once a step's model decrease is below the
    rounding of the loss, i.e. ~sqrt(eps) from the minimiser --, loss 1.2e-10 / 4.6e-11 relative (the loss
    is c0 - 2 g.dz + dz.H.dz with c0 up to 1e6 times the minimum), orthonormality 6.7e-16 / 1.0e-15.
    The device runs the same algorithm with another summation order and its own sin/cos: it is allowed
    10x the host's figure, floor 1e-12: pose 8.9e-9 / 7.7e-9, loss 1.2e-9 / 4.6e-10, R R^T - I 1e-12.
    (Measured on an MI355X, worst case: pose 6.0e-11 / 5.4e-11, loss 1.1e-10 / 6.6e-11, R R^T - I 2e-14.)"""
    s, q, W, idx, Tk, st = E.solve_case(dim, angle, identity_start)
    ref = E.solve_reference(s, q, W, idx, Tk, st)
    T, loss = inj.solve(st, Tk)
    R = T[:dim, :dim]
    pose_err = np.max(np.abs(T - ref["T"]))
    loss_err = abs(loss - E.mp_quad_loss(st, Tk, T)) / ref["loss"]
    orth_err = np.max(np.abs(R @ R.T - np.eye(dim)))
    print(f"k_solve<{dim}> angle {angle:+g} {'I' if identity_start else 'Tk'}: pose {pose_err:.2e} "
          f"loss {loss_err:.2e} orth {orth_err:.2e}")
    assert np.all(np.isfinite(T)) and np.array_equal(T[dim], np.eye(dim + 1)[dim])
    assert pose_err <= E.device_bound(E.HOST_POSE_ERR[dim])
    assert loss_err <= E.device_bound(E.HOST_LOSS_ERR[dim])
    assert orth_err <= E.device_bound(E.HOST_ORTH_ERR[dim])
    assert np.linalg.det(R) > 0


@pytest.mark.parametrize("dim", [2, 3])
def test_device_solve_without_correspondences_keeps_the_pose(inj, dim):
    """count = 0 inside k_solve: pose unchanged bit for bit, loss 0 (the host's behaviour)."""
    Tk = E.solve_case(dim, 0.2, False)[4]
    st = np.zeros(gicp.stats_size(dim))
    Th, fh = gicp.solve_pose(st, Tk)
    assert np.array_equal(Th, Tk) and fh == 0.0
    T, loss = inj.solve(st, Tk)
    assert np.array_equal(T, Tk) and loss == 0.0
    # statistics that are not zero but whose count is: still no correspondences
    st = E.solve_case(dim, 0.2, False)[5].copy()
    st[-1] = 0.0
    T, loss = inj.solve(st, Tk)
    assert np.array_equal(T, Tk) and loss == 0.0


@pytest.mark.parametrize("dim", [2, 3])
def test_device_solve_translation_block_not_positive_definite(inj, dim):
    """Point-to-plane statistics with every normal parallel: sum W = N n n^T is singular.  The host's
    outcome is the specification, and it is a refusal: solve_pose_t finds the translation block not
    positive definite (spd_inv), returns ok = 0 and gicp.solve_pose raises ValueError (checked here and in
    test_edge_ref_cpu.py).  k_solve must take the same branch -- solve_pose_wave returns false, solve_fail
    is set -- and gicp_align must raise ValueError; the engine stays usable afterwards."""
    st = E.parallel_normal_stats(dim)
    Tk = np.eye(dim + 1)
    with pytest.raises(ValueError):
        gicp.solve_pose(st, Tk)
    with pytest.raises(ValueError):
        inj.solve(st, Tk)
    s, q, W, idx, Tk, st = E.solve_case(dim, 0.05, True)
    T, _ = inj.solve(st, Tk)
    assert np.max(np.abs(T - gicp.solve_pose(st, Tk)[0])) <= E.device_bound(E.HOST_POSE_ERR[dim])


def test_device_solve_collinear_sources(inj):
    """All accepted source points on one line: rotation about the line is free, the rotation Hessian is
    rank deficient and the damping escalates.  The result is finite and orthonormal, its loss is not above
    the starting loss c0, and equals the host's within the relative loss bound (4.6e-10)."""
    st = E.collinear_stats()
    Tk = np.eye(4)
    c0 = O.expand_stats(st, 3)[2]
    Th, fh = gicp.solve_pose(st, Tk)
    T, loss = inj.solve(st, Tk)
    R = T[:3, :3]
    print(f"collinear: host loss {fh!r} device loss {loss!r} c0 {c0!r}")
    assert np.all(np.isfinite(T)) and np.isfinite(loss)
    assert np.max(np.abs(R @ R.T - np.eye(3))) <= E.device_bound(E.HOST_ORTH_ERR[3])
    assert loss <= c0 and fh <= c0
    assert abs(loss - fh) <= E.device_bound(E.HOST_LOSS_ERR[3]) * fh
