"""NumPy restatement of the local voxel map (include/gicp_hip.h "local voxel map") -- the
tests' yardstick, written from the stated semantics, not from the kernels.

A map has a dimension, a leaf and a half-width in cells R = ceil(max_range / leaf).  Its voxels are cells of the
absolute grid floor(x / leaf); each holds the fp64 sums of the coordinates of every point merged into it and
their number.  insert(points, T), T = sensor -> world:
  1. every point moves to the world frame as ((R_a0 x + R_a1 y) + R_a2 z) + t_a, each product and sum rounded
     on its own (the z term dropped in 2-D);
  2. the window becomes the cube |cell_a - c_a| <= R around c = floor(t / leaf): voxels outside it are
     forgotten, new points outside it discarded;
  3. the new points are merged: stored sum first, then the voxel's new points in row order;
  4. rows are kept in ascending lexicographic order of the cells.
"""
import math

import numpy as np


def transform(points, T):
    """The scan in the world frame, in the stated operation order (NumPy rounds every product and sum)."""
    x = np.asarray(points, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    d = T.shape[0] - 1
    R, t = T[:d, :d], T[:d, d]
    w = np.empty((len(x), d))
    for a in range(d):
        acc = R[a, 0] * x[:, 0] + R[a, 1] * x[:, 1]
        if d == 3:
            acc = acc + R[a, 2] * x[:, 2]
        w[:, a] = acc + t[a]
    return w


class MapRef:
    """Vectorised restatement.  Rows: cells int64 [M, d], sums [M, d], counts int64 [M], and amax [M, d], the
    largest |coordinate| of the world-frame points merged into the voxel since it was last (re)created (the
    scale of the centroids' error bound)."""

    def __init__(self, dim, leaf, max_range):
        self.dim, self.leaf = int(dim), float(leaf)
        self.R = int(math.ceil(max_range / leaf))
        self.cells = np.zeros((0, dim), dtype=np.int64)
        self.sums = np.zeros((0, dim))
        self.counts = np.zeros(0, dtype=np.int64)
        self.amax = np.zeros((0, dim))

    def insert(self, points, T):
        T = np.asarray(T, dtype=np.float64)
        d = self.dim
        w = transform(points, T)
        c = np.floor(T[:d, d] / self.leaf).astype(np.int64)
        pc = np.floor(w / self.leaf).astype(np.int64)
        pin = np.all(np.abs(pc - c) <= self.R, axis=1)
        rin = np.all(np.abs(self.cells - c) <= self.R, axis=1)
        w, pc = w[pin], pc[pin]
        cells = np.concatenate([self.cells[rin], pc])
        uniq, inv = np.unique(cells, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        m = int(rin.sum())
        sums = np.zeros((len(uniq), d))
        counts = np.zeros(len(uniq), dtype=np.int64)
        amax = np.zeros((len(uniq), d))
        np.add.at(sums, inv, np.concatenate([self.sums[rin], w]))          # (in index order: stored sum first)
        np.add.at(counts, inv, np.concatenate([self.counts[rin], np.ones(len(w), dtype=np.int64)]))
        np.maximum.at(amax, inv, np.concatenate([self.amax[rin], np.abs(w)]))
        self.cells, self.sums, self.counts, self.amax = uniq, sums, counts, amax
        return self

    def get(self, min_points=1):
        """(cells, centroids, counts, amax) of the voxels holding >= min_points points, in key order."""
        k = self.counts >= min_points
        return self.cells[k], self.sums[k] / self.counts[k][:, None], self.counts[k], self.amax[k]

    def __len__(self):
        return len(self.cells)


class MapLoop:
    """The same map as a plain dict and Python floats (checks MapRef itself)."""

    def __init__(self, dim, leaf, max_range):
        self.dim, self.leaf = int(dim), float(leaf)
        self.R = int(math.ceil(max_range / leaf))
        self.vox = {}   # cell -> [sums, count]

    def insert(self, points, T):
        d = self.dim
        T = np.asarray(T, dtype=np.float64)
        c = [math.floor(float(T[a, d]) / self.leaf) for a in range(d)]
        inside = lambda cell: all(abs(cell[a] - c[a]) <= self.R for a in range(d))  # noqa: E731
        self.vox = {cell: v for cell, v in self.vox.items() if inside(cell)}
        for p in np.asarray(points, dtype=np.float64):
            w = []
            for a in range(d):
                acc = float(T[a, 0]) * float(p[0]) + float(T[a, 1]) * float(p[1])
                if d == 3:
                    acc = acc + float(T[a, 2]) * float(p[2])
                w.append(acc + float(T[a, d]))
            cell = tuple(math.floor(v / self.leaf) for v in w)
            if not inside(cell):
                continue
            row = self.vox.setdefault(cell, [[0.0] * d, 0])
            row[0] = [s + v for s, v in zip(row[0], w)]
            row[1] += 1
        return self

    def get(self, min_points=1):
        keys = [k for k in sorted(self.vox) if self.vox[k][1] >= min_points]
        cells = np.array(keys, dtype=np.int64).reshape(len(keys), self.dim)
        counts = np.array([self.vox[k][1] for k in keys], dtype=np.int64)
        cent = np.array([[s / self.vox[k][1] for s in self.vox[k][0]] for k in keys]).reshape(len(keys), self.dim)
        return cells, cent, counts
