"""NumPy restatement of the top-k of det(W) (include/gicp_hip.h gicp_top_weights, gicp_trace.top_*): the
determinant as the kernel's cofactor expansion, the selection as the last k of a stable argsort, and the merge
of the ranks' rows by (det, source index).  Nothing here touches the engine; test_topk_ref_cpu.py checks these
helpers on their own."""
import numpy as np


def det_closed_form(W):
    """det of W [n, d, d], d = 2 or 3: the cofactor expansion along the first row, elementwise in fp64, term by
    term as k_corr writes it.  (np.linalg.det goes through an LU and exp/log of the pivots and is not exact:
    det(0.5 I_3) != 0.125 there.)  For W = w I with w a power of two every product is exact and every other
    term is 0, so the value is w^d in any evaluation order, fused or not."""
    W = np.asarray(W, dtype=np.float64)
    d = W.shape[-1]
    assert W.ndim == 3 and W.shape[1] == d and d in (2, 3), W.shape
    if d == 2:
        return W[:, 0, 0] * W[:, 1, 1] - W[:, 0, 1] * W[:, 1, 0]
    return (W[:, 0, 0] * (W[:, 1, 1] * W[:, 2, 2] - W[:, 1, 2] * W[:, 2, 1])
            - W[:, 0, 1] * (W[:, 1, 0] * W[:, 2, 2] - W[:, 1, 2] * W[:, 2, 0])
            + W[:, 0, 2] * (W[:, 1, 0] * W[:, 2, 1] - W[:, 1, 1] * W[:, 2, 0]))


def top_reference(det, index, k):
    """(src[k], tgt[k], det[k]): the last k rows of the stable ascending argsort of det (equal dets: the larger
    original row last), with tgt = index[src].  Fewer than k rows: the pads -1 / -1 / 0 come first."""
    det = np.asarray(det, dtype=np.float64)
    index = np.asarray(index, dtype=np.int64)
    n = len(det)
    assert index.shape == (n,) and k >= 1
    src = np.lexsort((np.arange(n), det))[-k:].astype(np.int64)
    pad = k - len(src)
    return (np.concatenate([np.full(pad, -1, dtype=np.int64), src]),
            np.concatenate([np.full(pad, -1, dtype=np.int64), index[src]]),
            np.concatenate([np.zeros(pad), det[src]]))


def merge_reference(rows, k):
    """The ranks' rows [(src, tgt, det), ...] merged: pads (src < 0) dropped, the k largest by (det, source
    index), ascending.  Fewer than k rows in all: only those, no pads."""
    src = np.concatenate([np.asarray(r[0], dtype=np.int64) for r in rows])
    tgt = np.concatenate([np.asarray(r[1], dtype=np.int64) for r in rows])
    det = np.concatenate([np.asarray(r[2], dtype=np.float64) for r in rows])
    keep = [i for i in range(len(src)) if src[i] >= 0]
    keep.sort(key=lambda i: (det[i], src[i]))
    keep = np.asarray(keep[-k:], dtype=np.int64)
    return src[keep], tgt[keep], det[keep]
