"""The top-k reference tests/topk_ref.py on its own, without a GPU: the selection against NumPy's stable argsort,
gicp._merge_top against the merge restated there and against the top-k of the whole, and the closed-form
determinant's exact values on W = w I."""
import numpy as np
import pytest

import topk_ref as TR

gicp = pytest.importorskip("gicp")

KS = range(1, 17)


def _data(kind, n, rng):
    if kind == "random":
        return rng.random(n)
    if kind == "equal":
        return np.full(n, 0.125)
    return rng.integers(0, 3, n) / 8.0                       # three values: ties inside and across the last k


@pytest.mark.parametrize("kind", ["random", "equal", "few_values"])
@pytest.mark.parametrize("n", [1, 5, 16, 17])
def test_top_reference_is_the_stable_argsort(kind, n):
    rng = np.random.default_rng(100 * n + len(kind))
    det = _data(kind, n, rng)
    index = rng.integers(-1, 50, n)
    for k in KS:
        src, tgt, dv = TR.top_reference(det, index, k)
        want = np.argsort(det, kind="stable")[-k:]
        pad = k - len(want)
        assert pad == max(0, k - n)
        assert src.dtype == np.int64 and tgt.dtype == np.int64 and dv.dtype == np.float64
        assert src.shape == tgt.shape == dv.shape == (k,)
        assert np.all(src[:pad] == -1) and np.all(tgt[:pad] == -1) and np.all(dv[:pad] == 0.0)   # pads first
        assert np.array_equal(src[pad:], want)
        assert np.array_equal(tgt[pad:], index[want]) and np.array_equal(dv[pad:], det[want])
        if kind == "equal":                                   # decided by the row alone: the last k rows, in order
            assert np.array_equal(src[pad:], np.arange(n)[-k:])


def _split(det, index, owner, nranks, k):
    """Each rank's top-k over its own rows, as source indices of the whole (what a shard returns)."""
    rows = []
    for r in range(nranks):
        mine = np.nonzero(owner == r)[0]
        s, t, v = TR.top_reference(det[mine], index[mine], k)
        rows.append((np.where(s >= 0, mine[np.maximum(s, 0)], -1) if len(mine) else s, t, v))
    return rows


@pytest.mark.parametrize("kind", ["random", "equal", "few_values"])
@pytest.mark.parametrize("nranks,n", [(1, 40), (3, 40), (7, 40), (7, 9), (3, 2)])
def test_merge_top_is_the_top_of_the_whole(kind, nranks, n):
    """Ranks of uneven size, some empty or smaller than k (their rows carry pads), dets tied across ranks."""
    rng = np.random.default_rng(7 * nranks + n + len(kind))
    det = _data(kind, n, rng)
    index = rng.integers(-1, 50, n)
    owner = rng.integers(0, max(1, nranks - 1), n)            # (the last rank of several owns nothing)
    for k in KS:
        rows = _split(det, index, owner, nranks, k)
        if nranks > 1:
            assert np.all(rows[-1][0] == -1)
        if kind != "random" and nranks > 1 and n >= 9:
            heads = [r[2][-1] for r in rows if r[0][-1] >= 0]
            assert len(heads) > 1 and len(set(heads)) < len(heads)        # a det tied across ranks
        got = gicp._merge_top(rows, k)
        ref = TR.merge_reference(rows, k)
        whole = TR.top_reference(det, index, k)
        keep = whole[0] >= 0
        for a, b, c in zip(got, ref, whole):
            assert a.dtype == b.dtype
            assert np.array_equal(a, b)
            assert np.array_equal(a, c[keep])                 # the merge drops the pads
        assert len(got[0]) == min(k, n)


def test_merge_drops_pads_wherever_they_stand():
    rows = [(np.array([-1, -1, 4]), np.array([-1, -1, 9]), np.array([0.0, 0.0, 0.5])),
            (np.array([-1, -1, -1]), np.array([-1, -1, -1]), np.zeros(3)),
            (np.array([2, 7, 3]), np.array([-1, 5, 6]), np.array([0.0, 0.5, 1.0]))]
    for k, want in ((1, [3]), (2, [7, 3]), (3, [4, 7, 3]), (4, [2, 4, 7, 3]), (16, [2, 4, 7, 3])):
        for fn in (gicp._merge_top, TR.merge_reference):
            s, t, v = fn(rows, k)
            assert list(s) == want
            assert list(t) == [{2: -1, 4: 9, 7: 5, 3: 6}[i] for i in want]
            assert list(v) == [{2: 0.0, 4: 0.5, 7: 0.5, 3: 1.0}[i] for i in want]


@pytest.mark.parametrize("d", [2, 3])
def test_det_closed_form_is_exact_on_scaled_identities(d):
    ws = np.array([1.0, 0.5, 0.25, 0.0])
    W = ws[:, None, None] * np.eye(d)
    assert np.array_equal(TR.det_closed_form(W), ws ** d)
    assert list(TR.det_closed_form(W)) == ([1.0, 0.25, 0.0625, 0.0] if d == 2 else [1.0, 0.125, 0.015625, 0.0])
    assert not np.any(np.signbit(TR.det_closed_form(W)))


@pytest.mark.parametrize("d", [2, 3])
def test_det_closed_form_is_the_determinant(d):
    """Against np.linalg.det on well-conditioned matrices, to the 1e-12 that the GPU test allows the kernel."""
    rng = np.random.default_rng(d)
    A = rng.normal(size=(200, d, d))
    W = A @ np.swapaxes(A, 1, 2) + np.eye(d)
    np.testing.assert_allclose(TR.det_closed_form(W), np.linalg.det(W), rtol=1e-12)
