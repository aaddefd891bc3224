"""Inputs of tests/test_gpu_stats_epilogue.py, shared with scripts/make_stats_epilogue_golden.py (which
records the statistics of every case as raw 64-bit words), and the one engine call sequence both use.

Two families of cases exercise k_corr's statistics epilogue (the transpose of a wave's 64 points through LDS,
the 16x16 fp64 MFMA product and its mapping onto the statistics vector):

  * fill: a tight source cluster of n points in front of a ~2k-point target, n either side of every
    multiple of 16 up to 64, and 300;
  * pattern: source tiles of exactly 64 points of which a chosen set of lanes is accepted.

How the pattern source gets 64-point tiles whose lane order is known.  A cloud is sorted by Morton code
(stable radix sort) and cut into tiles inside 16 equal index segments, never across one.  The source is 16
groups of 64 points; every coordinate increases strictly along the whole cloud, so the Morton code (an
interleave of per-coordinate monotone grid indices) never decreases and the sorted order is the input
order.  The 16 groups share their increments, so their extents agree to a grid cell: each segment of 64
is one tile, lane l of tile c being input point 64 c + l.  The test checks the tile count on the device
(16 source tiles walk on a cold pass)."""
import numpy as np

import edge_ref as E
from oracle import gicp_oracle as O

FILL_N = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 300)
FILL_D_C = 0.5
FILL_D_N = 1.0

GROUPS, TILE = 16, 64
PAT_D_C = 0.02
PAT_D_N = 0.5
PATTERNS = {
    "none": [],
    "lane0": [0],
    "lane63": [63],
    "group4": list(range(20, 24)),
    "group16": list(range(32, 48)),
    "low32": list(range(0, 32)),
    "high32": list(range(32, 64)),
    "alternating": list(range(0, 64, 2)),
}
MODELS = ("point_to_point", "point_to_plane")


def _turn(dim, deg):
    if dim == 2:
        return O.rot2(np.deg2rad(deg))
    return O.so3_exp(np.deg2rad(deg) * np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5]))


def fill_case(dim, n):
    """(source [n, dim], target [2000, dim], two poses): the source is the n target points nearest the
    target's centroid, moved by 4 mm of noise."""
    rng = np.random.default_rng([7, dim, n])
    _, tgt = E.dense_patch(dim, 4, 2000, seed=3)
    c = tgt.mean(axis=0)
    near = np.argsort(np.linalg.norm(tgt - c, axis=1), kind="stable")[:n]
    src = tgt[near] + rng.normal(0, 0.004, (n, dim))
    t = [0.02, -0.01, 0.015][:dim]
    return src, tgt, [np.eye(dim + 1), E.pose_about(src.mean(axis=0), _turn(dim, 1.5), t)]


def pattern_source(dim):
    """16 groups of 64 points, every coordinate strictly increasing: steps of 0.05 .. 0.10 per coordinate
    inside a group (the same steps in every group), groups 8 apart."""
    rng = np.random.default_rng([11, dim])
    steps = rng.uniform(0.05, 0.10, (TILE, dim))
    steps[0] = 0.0
    group = np.cumsum(steps, axis=0)
    return np.concatenate([group + 8.0 * c for c in range(GROUPS)])


def pattern_case(dim, name):
    """(source, target, pose, accepted mask over the source in input = sorted order).  The target is the
    moved source's chosen lanes, 3 mm off: every other lane is at least 0.05 sqrt(dim) - 0.003 > d_c from
    any target.  With no lane chosen the target is one point per group, 1 off in every coordinate."""
    src = pattern_source(dim)
    T = E.pose_about(src.mean(axis=0), _turn(dim, 0.7), [0.3, -0.2, 0.1][:dim])
    lanes = np.array(PATTERNS[name], dtype=np.int64)
    mask = np.zeros(len(src), dtype=bool)
    moved = O.apply_transformation(src, T)
    if len(lanes):
        chosen = (np.arange(GROUPS)[:, None] * TILE + lanes[None, :]).ravel()
        mask[chosen] = True
        off = np.array([0.003, -0.001, 0.002][:dim]) * (0.003 / np.linalg.norm([0.003, -0.001, 0.002][:dim]))
        tgt = moved[chosen] + off
    else:
        tgt = moved[::TILE] - 1.0
    return src, tgt, T, mask


def engine_pass(gicp, eng, src, tgt, T, d_c, d_n, model="plane_to_plane"):
    """Both clouds set afresh (a cold cache), then one pass at T with the per-point outputs:
    (statistics, debug dict, pass_info)."""
    p = gicp.default_params(src.shape[1], max_distance_correspondence=d_c, max_distance_nearest_neighbors=d_n,
                            cov_model=gicp._lib.COV_MODELS[model])
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    st, dbg = eng.iterate(T, debug=True)
    return st, dbg, eng.pass_info()


def all_cases():
    """(key in the golden file, source, target, pose, d_c, d_n, covariance model) of every case."""
    for d in (2, 3):
        for n in FILL_N:
            src, tgt, poses = fill_case(d, n)
            for k, T in enumerate(poses):
                yield f"fill_{d}d_n{n}_p{k}", src, tgt, T, FILL_D_C, FILL_D_N, "plane_to_plane"
    for d in (2, 3):
        for name in PATTERNS:
            src, tgt, T, _ = pattern_case(d, name)
            yield f"pattern_{d}d_{name}", src, tgt, T, PAT_D_C, PAT_D_N, "plane_to_plane"
    src, tgt, poses = fill_case(3, 300)
    for m in MODELS:
        yield f"model_{m}", src, tgt, poses[1], FILL_D_C, FILL_D_N, m


def case_keys():
    """Every case's key in the golden file, in a fixed order."""
    keys = [f"fill_{d}d_n{n}_p{k}" for d in (2, 3) for n in FILL_N for k in (0, 1)]
    keys += [f"pattern_{d}d_{name}" for d in (2, 3) for name in PATTERNS]
    keys += [f"model_{m}" for m in MODELS]
    return keys
