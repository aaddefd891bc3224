"""Reference of the input filters in NumPy, and the clouds the CPU and GPU tests share.

scipy's cKDTree only PROPOSES candidate pairs, within radius (1 + 1e-6); every decision is the fp64 expression of
include/gicp_hip.h evaluated in NumPy operation for operation -- d2 = ((dx*dx + dy*dy) + dz*dz) against the squared
bound, each product and sum rounded on its own -- so the mask and the counts are exact, not approximate."""
import functools

import numpy as np
from scipy.spatial import cKDTree


def d2(a, b):
    """((dx*dx + dy*dy) + dz*dz) of rows a and b (broadcast), the z term dropped in 2-D."""
    dx = a[..., 0] - b[..., 0]
    dy = a[..., 1] - b[..., 1]
    s = dx * dx + dy * dy
    if a.shape[-1] == 3:
        dz = a[..., 2] - b[..., 2]
        s = s + dz * dz
    return s


def filter_ref(points, center=None, min_range=0.0, max_range=0.0, radius=0.0, min_neighbors=1):
    """(keep mask [N] bool, counts [N] int32): the crop, then radius outlier removal among its survivors.  counts:
    per input row the exact number of other survivors within `radius`, -1 where the crop removed the row, 0 for
    every kept row when radius is 0."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
    n, d = p.shape
    c = np.zeros(d) if center is None else np.asarray(center, dtype=np.float64)[:d]
    crop = np.ones(n, dtype=bool)
    if min_range > 0 or max_range > 0:
        dd = d2(p, c[None, :])
        if min_range > 0:
            crop &= dd >= np.float64(min_range) * np.float64(min_range)
        if max_range > 0:
            crop &= dd <= np.float64(max_range) * np.float64(max_range)
    counts = np.where(crop, 0, -1).astype(np.int32)
    keep = crop.copy()
    if radius > 0:
        rows = np.flatnonzero(crop)
        q = p[rows]
        cnt = np.zeros(len(rows), dtype=np.int64)
        if len(rows) > 1:
            pairs = cKDTree(q).query_pairs(radius * (1.0 + 1e-6), output_type="ndarray")
            near = d2(q[pairs[:, 0]], q[pairs[:, 1]]) <= np.float64(radius) * np.float64(radius)
            cnt = np.bincount(pairs[near].ravel(), minlength=len(rows))
        counts[rows] = cnt
        keep[rows] = cnt >= min_neighbors
    return keep, counts


def min_margin(points, radius, crop=None):
    """The smallest |d2 - r^2| / r^2 over all candidate pairs of `points` (rows `crop` only): how far the nearest
    decision is from its bound."""
    p = np.asarray(points, dtype=np.float64)
    q = p if crop is None else p[crop]
    pairs = cKDTree(q).query_pairs(radius * 1.5, output_type="ndarray")
    if not len(pairs):
        return np.inf
    r2 = radius * radius
    return float(np.min(np.abs(d2(q[pairs[:, 0]], q[pairs[:, 1]]) - r2)) / r2)


# ---- the clouds of the one-shot tests (tests/test_filter_cpu.py, tests/test_gpu_filter.py) ----

SIZES = (63, 64, 65, 255, 256, 257)
# rocPRIM's scan and sort work in blocks of a few thousand items and switch algorithms on the size; the project's
# own kernels have one path (one lane per row, no grid stride).  One size below and above each plausible block
# edge
BLOCK_EDGES = (1023, 1025, 4095, 4097, 16383, 16385, 65535, 65537)


def _lattice(dim):
    g = np.arange(-12, 13) * 0.25
    pts = np.stack(np.meshgrid(*([g] * dim), indexing="ij"), -1).reshape(-1, dim)
    return pts[np.random.default_rng(5).permutation(len(pts))]


def _cloud(n, dim, seed):
    return np.random.default_rng(seed).uniform(-4.0, 4.0, (n, dim))


def _dense_cell(dim):
    rng = np.random.default_rng(11)
    dense = rng.uniform(10.05, 10.95, (5000, dim))       # inside one cell of edge 1 (1 + 2^-16) and of edge 1
    sparse = rng.uniform(-20.0, 20.0, (300, dim))
    pts = np.concatenate([dense, sparse])
    return pts[rng.permutation(len(pts))]


def _duplicates(dim):
    rng = np.random.default_rng(13)
    base = rng.uniform(-50.0, 50.0, (200, dim))
    pts = np.concatenate([base, base[:120], base[:60], base[:60]])   # rows 1, 2 or 4 times
    return pts[rng.permutation(len(pts))]


def _key_runs(dim):
    """8 cells of edge 1 per axis (3 key bits each, all used; the corner points fix the grid).  For every axis and
    both of its ends: a cluster A across the end cell and its inner neighbour, and a cluster B in the cell whose
    key is A's end cell moved one step further along that axis with the carry taken -- next to A in key order (for
    the last axis: the lowest cell of the next row), far from it in space.  A run of keys that is not clipped at
    the axis end reaches B, one that wraps below 0 loses A's own cells."""
    rng = np.random.default_rng(19)
    out = [np.full((1, dim), 0.01), np.full((1, dim), 7.99)]
    for a in range(dim):
        for end in (0, 7):
            cell = np.full(dim, 3)
            cell[a] = end
            inner = cell.copy()
            inner[a] += 1 if end == 0 else -1
            out.append(cell + 0.5 + rng.uniform(-0.3, 0.3, (5, dim)))
            out.append(inner + 0.5 + rng.uniform(-0.3, 0.3, (3, dim)))
            key = 0
            for b in range(dim):
                key = key * 8 + int(cell[b])
            key += (1 if end == 7 else -1) * 8 ** (dim - 1 - a)
            if 0 <= key < 8 ** dim:
                bcell = np.array([(key // 8 ** (dim - 1 - b)) % 8 for b in range(dim)])
                out.append(bcell + 0.5 + rng.uniform(-0.3, 0.3, (4, dim)))
    pts = np.concatenate(out)
    return pts[rng.permutation(len(pts))]


WIDEST_LOW = {3: (-1234567, -7, -2000001), 2: (-1234567891, -3)}     # lowest cells: negative, no powers of two


def widest(dim, extra=0):
    """About 3000 points at cell + 0.5 of the grid of edge 1.0 (exact in fp64) whose cells span exactly 2^21 (3-D)
    or 2^31 (2-D) cells on every axis, as test_gpu_voxel.py's widest cloud: both corner cells, a cell next to each
    corner, 70 points in one cell, the rest scattered.  extra = 1: one more point, one cell past the highest on
    axis 0 -- the first span that is refused."""
    rng = np.random.default_rng(17)
    span = 2 ** 21 if dim == 3 else 2 ** 31
    lo = np.array(WIDEST_LOW[dim], dtype=np.int64)
    hi = lo + span - 1
    cells = rng.integers(0, span, (2900, dim)) + lo
    one = lo + span // 3
    step = np.eye(dim, dtype=np.int64)
    cells = np.concatenate([cells, lo[None], hi[None], lo + step, hi - step, np.tile(one, (70, 1))])
    if extra:
        cells = np.concatenate([cells, (hi + extra * step[0])[None]])
    cells = cells[rng.permutation(len(cells))]
    return cells.astype(np.float64) + 0.5


@functools.lru_cache(maxsize=None)
def cases(dim):
    """{name: (points, filter keywords)}: the one-shot cases of the issue, read only."""
    out = {
        "one_row": (np.full((1, dim), 0.75), dict(max_range=2.0)),
        "two_coincident": (np.full((2, dim), -1.5), dict(radius=0.5, min_neighbors=1)),
        "lattice_r025": (_lattice(dim), dict(radius=0.25, min_neighbors=2 * dim)),
        "lattice_r05": (_lattice(dim), dict(radius=0.5, min_neighbors=12 if dim == 2 else 32)),
        # 3-4-5 triangles times 0.25: lattice points exactly on min_range 1.25 and on max_range 2.5
        "lattice_345": (_lattice(dim), dict(min_range=1.25, max_range=2.5)),
        "lattice_345_ror": (_lattice(dim), dict(min_range=1.25, max_range=2.5, radius=0.25, min_neighbors=2 * dim - 1)),
        "lattice_centre": (_lattice(dim), dict(center=(0.25, -0.5, 0.75)[:dim], min_range=0.75, max_range=1.25)),
        "dense_cell": (_dense_cell(dim), dict(radius=1.0, min_neighbors=5)),
        "duplicates": (_duplicates(dim), dict(radius=1e-3, min_neighbors=2)),
        "key_runs": (_key_runs(dim), dict(radius=1.0, min_neighbors=3)),
        "widest": (widest(dim), dict(radius=1.0, min_neighbors=1)),
    }
    for n in SIZES + BLOCK_EDGES:
        # (the box grows with n, so that the share of kept rows stays away from 0 and 1)
        scale = (n / 64.0) ** (1.0 / dim)
        out[f"n{n}"] = (_cloud(n, dim, n) * scale, dict(max_range=3.8 * scale, min_range=0.5, radius=1.2 if dim == 3 else 0.5,
                                                        min_neighbors=1))
    for pts, _ in out.values():
        pts.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(dim, name):
    """(points, keywords, keep mask, counts) of a case: computed once, shared, read only."""
    pts, kw = cases(dim)[name]
    keep, counts = filter_ref(pts, **kw)
    keep.setflags(write=False)
    counts.setflags(write=False)
    return pts, kw, keep, counts


def check_against_reference(fn, dim, name):
    """fn (gicp.filter_points or gicp.filter_points_host) on one case: mask, index list, counts and kept rows bit
    for bit; the early-exit call (no counts) keeps the same rows."""
    pts, kw, keep, counts = reference(dim, name)
    rows, idx, cnt = fn(pts, return_index=True, return_counts=True, **kw)
    assert idx.dtype == np.int64 and cnt.dtype == np.int32 and cnt.shape == (len(pts),)
    assert np.array_equal(idx, np.flatnonzero(keep)), (name, len(idx), int(keep.sum()))
    assert np.array_equal(cnt, counts), (name, int(np.sum(cnt != counts)))
    assert rows.tobytes() == pts[keep].tobytes()
    early = fn(pts, **kw)
    assert early.tobytes() == rows.tobytes()
    return keep, counts
