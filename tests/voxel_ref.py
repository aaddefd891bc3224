"""NumPy restatement of the voxel-grid filter (include/gicp_hip.h) — the tests' yardstick.

Absolute grid: the cell of a point is np.floor(x / leaf) per axis.  One centroid per occupied cell, the
cells in ascending lexicographic order (np.unique(axis=0)), cells with fewer than min_points points dropped.
"""
import numpy as np


def voxel_ref(points, leaf, min_points=1):
    """(centroids [M, d], counts [M] int64, cells [M, d]) of the kept voxels, in np.unique's order."""
    x = np.asarray(points, dtype=np.float64)
    cells = np.floor(x / leaf)
    uniq, inv, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    sums = np.zeros_like(uniq)
    np.add.at(sums, inv, x)
    cent = sums / counts[:, None]
    keep = counts >= min_points
    return cent[keep], counts[keep], uniq[keep]


def voxel_abs_max(points, leaf, min_points=1):
    """max |x_a| over each kept voxel's points, per axis ([M, d]): the scale of the centroid error bound."""
    x = np.asarray(points, dtype=np.float64)
    uniq, inv, counts = np.unique(np.floor(x / leaf), axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    amax = np.zeros_like(uniq)
    np.maximum.at(amax, inv, np.abs(x))
    return amax[counts >= min_points]


def voxel_loop(points, leaf, min_points=1):
    """The same filter as a plain dict-of-lists loop (checks voxel_ref itself)."""
    import math
    vox = {}
    for p in np.asarray(points, dtype=np.float64):
        vox.setdefault(tuple(math.floor(v / leaf) for v in p), []).append(p)
    cent, counts, cells = [], [], []
    for c in sorted(vox):
        pts = vox[c]
        if len(pts) < min_points:
            continue
        s = np.zeros(len(c))
        for p in pts:
            s = s + p
        cent.append(s / len(pts))
        counts.append(len(pts))
        cells.append(c)
    return np.array(cent), np.array(counts, dtype=np.int64), np.array(cells, dtype=np.float64)
