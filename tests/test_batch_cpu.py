"""Batched registration, the parts that need no GPU: the entry points' binding and provenance, every
refusal of gicp_batch_align (checked before the context is looked at, so a NULL context serves), multistart's
selection rule, and the preconditions the GPU tests of test_gpu_batch.py lean on, measured here with the oracle."""
import ctypes as C
import inspect

import numpy as np
import pytest

import batch_ref as B
import gpu_helpers as H
from oracle import gicp_oracle as O

gicp = pytest.importorskip("gicp")
from gicp import _lib  # noqa: E402


def test_entry_points_are_bound_and_hashed():
    lib = _lib.load()
    for name in ("gicp_batch_align", "gicp_batch_max_points"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.gicp_version() >= 105
    i = _lib.HASH_SRCS.index("csrc/gicp_batch.hip")
    assert _lib.HASH_SRCS[i - 1] == "csrc/gicp_filter.hip" and _lib.HASH_SRCS[i + 1] == "csrc/gicp_batch.cpp"
    j = _lib.HASH_SRCS.index("csrc/gicp_cov_dev.h")
    assert _lib.HASH_SRCS[j - 1] == "csrc/gicp_filter.h"
    assert _lib.build_info()["src"] == _lib.source_hash()
    # the structs of include/gicp_hip.h
    assert C.sizeof(_lib.BatchProblem) == 2 * 4 + 16 * 8
    assert C.sizeof(_lib.BatchResult) == 6 * 4 + 8 + 2 * 8
    assert C.sizeof(_lib.BatchDebug) == 5 * C.sizeof(C.c_void_p)
    assert _lib.MAX_STATS == gicp.stats_size(3)
    assert lib.gicp_batch_max_points(2) >= 2048 and lib.gicp_batch_max_points(3) >= 2048
    assert lib.gicp_batch_max_points(4) == _lib.GICP_E_INVALID
    assert gicp.batch_max_points(3) == lib.gicp_batch_max_points(3) == B.COV_SIZES[-1]
    for name in ("align_batch", "multistart"):
        assert name in gicp.__all__ and callable(getattr(gicp, name))
    assert list(inspect.signature(gicp.Engine.align_batch).parameters) == ["self", "clouds", "pairs", "T0", "params", "debug"]
    assert inspect.signature(gicp.align_batch).parameters["device"].default == 0


def _call(dim, clouds, pairs, T0=None, params=None, ctx=None, raw=None):
    """(rc, this thread's message, T_out) of one raw gicp_batch_align call with a NULL context; `raw` replaces
    arguments by name (xyz, offsets, n_clouds, problems, n_problems, T_out)."""
    lib = _lib.load()
    xyz = np.ascontiguousarray(np.concatenate(clouds, axis=0), dtype=np.float64)
    off = np.zeros(len(clouds) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    nb = len(pairs)
    probs = (_lib.BatchProblem * max(nb, 1))()
    for b, (s, t) in enumerate(pairs):
        probs[b].source, probs[b].target = s, t
        T = np.eye(min(dim, 3) + 1) if T0 is None else np.asarray(T0[b], dtype=np.float64)
        for k, v in enumerate(T.ravel()):
            probs[b].T0[k] = v
    out = np.full((max(nb, 1), dim + 1, dim + 1), -7.0)
    res = (_lib.BatchResult * max(nb, 1))()
    for r in res:
        r.status = r.iterations = -7
    a = dict(xyz=_lib.dptr(xyz), offsets=off.ctypes.data_as(C.POINTER(C.c_int64)), n_clouds=len(clouds), problems=probs,
             n_problems=nb, T_out=_lib.dptr(out))
    if raw:
        for k, v in raw.items():
            a[k] = v(off) if callable(v) else v
    rc = lib.gicp_batch_align(ctx, dim, a["xyz"], a["offsets"], a["n_clouds"], a["problems"], a["n_problems"],
                              C.byref(params) if params is not None else None, a["T_out"], res, None)
    assert np.all(out == -7.0) and all(r.status == -7 and r.iterations == -7 for r in res), "a refused call wrote its outputs"
    return rc, lib.gicp_last_host_error().decode()


def _pts(dim, n, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, dim))


def _off(edit):
    def f(off):
        o = off.copy()
        edit(o)
        f.keep = o          # (alive until the call returns)
        return o.ctypes.data_as(C.POINTER(C.c_int64))
    return f


def test_refusals_and_their_messages():
    cl = [_pts(3, 40, 1), _pts(3, 50, 2), _pts(3, 7, 3)]
    pairs = [(0, 1), (2, 1), (1, 0)]
    nanT = np.tile(np.eye(4), (3, 1, 1))
    nanT[1, 0, 3] = np.nan
    infT = np.tile(np.eye(4), (3, 1, 1))
    infT[2, 1, 1] = np.inf
    bad = [c.copy() for c in cl]
    bad[1][13, 2] = np.inf
    big = [cl[0], _pts(3, gicp.batch_max_points(3) + 1, 4)]

    def p(**kw):
        return gicp.default_params(3, **kw)

    cases = [
        (dict(dim=4), "dim must be 2 or 3"),
        (dict(dim=1), "dim must be 2 or 3"),
        (dict(raw=dict(n_clouds=0)), "n_clouds must be >= 1"),
        (dict(pairs=[]), "n_problems must be >= 1"),
        (dict(raw=dict(n_problems=-2)), "n_problems must be >= 1"),
        (dict(raw=dict(xyz=None)), "must not be NULL"),
        (dict(raw=dict(offsets=None)), "must not be NULL"),
        (dict(raw=dict(problems=None)), "must not be NULL"),
        (dict(raw=dict(T_out=None)), "must not be NULL"),
        (dict(raw=dict(offsets=_off(lambda o: o.__setitem__(0, 1)))), "offsets must start at 0"),
        (dict(raw=dict(offsets=_off(lambda o: o.__setitem__(2, 30)))), "offsets do not ascend at cloud 1"),
        (dict(raw=dict(offsets=_off(lambda o: o.__setitem__(2, 40)))), "cloud 1 is empty"),
        (dict(clouds=big, pairs=[(0, 1)]), "cloud 1 has 2049 points, more than gicp_batch_max_points = 2048"),
        (dict(pairs=[(0, 1), (3, 1)]), "problem 1 names a cloud out of range (source 3"),
        (dict(pairs=[(0, -1)]), "problem 0 names a cloud out of range"),
        (dict(clouds=bad), "cloud 1 contains non-finite coordinates (row 13)"),
        (dict(T0=nanT), "T0 of problem 1 contains non-finite values"),
        (dict(T0=infT), "T0 of problem 2 contains non-finite values"),
        (dict(params=p(cov_model=7)), "cov_model must be"),
        (dict(params=p(robust_kernel=9, robust_scale=1.0)), "robust_kernel must be"),
        (dict(params=p(robust_kernel="huber", robust_scale=0.0)), "robust_scale must be finite and > 0"),
        (dict(params=p(robust_kernel="tukey", robust_scale=np.nan)), "robust_scale must be finite and > 0"),
        (dict(params=p(k_neighbors=7)), "unsupported k_neighbors"),
    ]
    for kw, text in cases:
        a = dict(dim=3, clouds=cl, pairs=pairs)
        a.update(kw)
        rc, msg = _call(**a)
        assert rc == _lib.GICP_E_INVALID and msg.startswith("gicp_batch_align: ") and text in msg, (kw.keys(), msg)
    # nothing to refuse but the missing context: still GICP_E_INVALID, without a HIP call
    rc, msg = _call(3, cl, pairs)
    assert rc == _lib.GICP_E_INVALID and "context must not be NULL" in msg
    rc, msg = _call(3, cl, pairs, params=p(k_neighbors=10, robust_kernel="tukey", robust_scale=2.0))
    assert rc == _lib.GICP_E_INVALID and "context must not be NULL" in msg
    rc, msg = _call(2, [_pts(2, 1), _pts(2, 2048)], [(0, 1), (1, 1)])       # sizes 1 and the limit pass the checks
    assert rc == _lib.GICP_E_INVALID and "context must not be NULL" in msg


def test_pick_start_rule():
    def r(status, n, mse):
        return dict(status=status, correspondences=n, mse=mse)

    assert gicp.pick_start([r(0, 10, 1.0), r(0, 12, 5.0), r(0, 11, 0.1)]) == 1          # most correspondences
    assert gicp.pick_start([r(0, 12, 2.0), r(0, 12, 1.0), r(0, 12, 3.0)]) == 1          # then the smaller mse
    assert gicp.pick_start([r(0, 12, 1.0), r(0, 12, 1.0), r(0, 3, 0.0)]) == 0           # then the lower index
    assert gicp.pick_start([r(-1, 99, 0.0), r(0, 5, 2.0), r(-1, 50, 0.0)]) == 1         # failed starts never win
    assert gicp.pick_start([r(-1, 99, 0.0)]) is None and gicp.pick_start([]) is None
    assert gicp.pick_start([r(0, 0, 0.0), r(0, 0, 0.0)]) == 0


# ---- the preconditions of the GPU tests, asserted with the oracle ----

@pytest.mark.parametrize("name", B.FIXTURES)
def test_fixture_steps_keep_clear_of_the_tolerance(name):
    """Stop-rule parity between two summation orders needs |delta loss| away from `tolerance` at the stopping
    iteration (below) and at the one before (above): at least 10 % on every convergent fixture.  Measured: the
    tightest are robot_p1_r90 (0.885 x tolerance at the stop) and robot_p0_r360 (1.28 x the iteration before)."""
    src, tgt, kw = B.fixture(name)
    at, stop, before = B.loss_steps(src, tgt, **kw)
    print(f"{name}: stops at {at}, |dloss| {stop / kw['tolerance']:.3g} x tol, before {before / kw['tolerance']:.3g} x tol")
    assert 1 <= at < kw["max_iterations"]
    assert stop <= 0.9 * kw["tolerance"] and before >= 1.1 * kw["tolerance"]


def test_room_pair_preconditions():
    """The small 3-D pair converges at iteration 8 with its steps 24 x above and 2.9 x below the tolerance, and
    most of its target neighbourhoods are full (k = 20 within d_n)."""
    src, tgt, _ = B.room_pair()
    assert src.shape == (1500, 3) and tgt.shape == (1400, 3)
    kw = dict(max_iterations=100, tolerance=1e-6, **B.P3)
    at, stop, before = B.loss_steps(src, tgt, **kw)
    print(f"room pair: stops at {at}, |dloss| {stop / 1e-6:.3g} x tol, before {before / 1e-6:.3g} x tol")
    assert at == B.ROOM_ITERATIONS and stop <= 0.9e-6 and before >= 1.1e-6
    _, cnt = O.covariances(tgt, B.P3["max_distance_nearest_neighbors"], faithful=False)
    assert np.mean(cnt == O.default_k(3)) >= 0.8


@pytest.mark.parametrize("dim", [2, 3])
def test_covariance_clouds_leave_the_oracle_within_two_percent(dim):
    """check_covariances' entrywise criterion leaves out the surface points whose eigen-gap is below 1e-2, at most
    2 % of a cloud: on the clouds the GPU test uses, the oracle's own neighbourhoods leave out no more."""
    d_n = 1.0
    clouds = [B.cov_cloud(dim, n) for n in B.COV_SIZES] + ([H.planar_lattice()] if dim == 3 else [])
    for pts in clouds:
        rep = B.oracle_cov_report(pts, d_n)
        surf = rep["surface"]
        left = int(np.sum(surf & (rep["gap"] < 1e-2)))
        print(f"dim {dim} n {len(pts)}: surface {int(surf.sum())}, small gap {left}")
        assert rep["count_ok"] and left <= 0.02 * len(pts), (len(pts), left)
    assert any(B.oracle_cov_report(c, d_n)["surface"].any() for c in clouds[2:])


@pytest.mark.parametrize("name", sorted(B.PCL_CASES))
def test_pcl_cases_stop_clear_of_their_epsilon(name):
    """The PCL-rule cases of the GPU stop-rule test end on GICP_STOP_TRANSFORM at the same iteration for half and
    for twice their transformation_epsilon: the increment is a factor of two clear of the threshold on both sides."""
    src, tgt, kw = B.pcl_case(name)
    eps, at = B.PCL_CASES[name]
    for f in (0.5, 1.0, 2.0):
        k = dict(kw, transformation_epsilon=f * eps)
        _, rec = O.gicp(src, tgt, inner="gn", source_cov="rotate", record=True, **k)
        assert rec["converged_at"] == at and rec["stop_reason"] == "transform", (f, rec["converged_at"], rec["stop_reason"])
