"""Inputs of tests/test_gpu_point_record.py, shared with scripts/make_point_record_golden.py (which records what the
build before the 48-byte point records gave, as raw words), and the engine call sequences both use.

A cloud's points live on the device as records (x, y, z, m0, m1, m2) of the covariance C = a I - m m^T; `a` is not
stored (the cloud's epsilon, or 1 for an isolated point, which the record marks).  The cases:

  * decode: 2000-point clouds with at least 50 isolated points each (isolated source points on the target's surface,
    isolated target points on the source's, and isolated pairs far from both), the source built with epsilon 1e-3
    and the target with 4e-3, ratio at its default and at 1 (m = 0 for every surface point), every covariance model;
  * shard: a 6000-point pair of the same construction, the source built as shard 0 and as shard 1 of 2;
  * offset: clouds 1e5 from the origin at 5 cm spacing, source clusters of 1, 2, 17, 63 and 64 points and a source
    of sixteen full 64-point tiles, three poses in a row on one cache (the walk, the certificates and the graph
    descent run in turn);
  * boundary: clouds of 1 .. 65 points a side (records that straddle 128-byte lines, the allocation's last record).

Large per-point arrays are recorded as one 32-bit checksum per row (position-weighted wrap-around sum of the
row's 64-bit words, folded) and a SHA-256 of the whole array: equal bits give equal digests, and a differing row is
named."""
import hashlib

import numpy as np

import edge_ref as E
from oracle import gicp_oracle as O

EPS_SRC, EPS_TGT = 1e-3, 4e-3
MODELS = ("plane_to_plane", "point_to_point", "point_to_plane")
RATIOS = {"r0": None, "r1": 1.0}          # None: the default ratio
DEC_N, DEC_D_C, DEC_D_N = 2000, 0.3, 0.4
SHARD_N = 6000
OFF_T = np.array([1e5, -3e4, 7e3])
OFF_SPACING, OFF_D_C, OFF_D_N = 0.05, 0.1, 0.25
OFF_FILLS = (1, 2, 17, 63, 64)
BND_N = (1, 2, 3, 7, 8, 9, 65)
BND_D_C, BND_D_N = 0.5, 50.0
SPACING = 0.12


def params(gicp, dim, eps, ratio, d_c, d_n, model="plane_to_plane"):
    kw = dict(max_distance_correspondence=d_c, max_distance_nearest_neighbors=d_n, epsilon=eps,
              cov_model=gicp._lib.COV_MODELS[model])
    if ratio is not None:
        kw["ratio"] = ratio
    return gicp.default_params(dim, **kw)


def ratio_value(ratio):
    return O.RATIO if ratio is None else ratio


# ----------------------------------------------------------------------------- geometry
def _height(u, v):
    return 0.05 * np.sin(u * 1.3) + 0.04 * np.cos(v * 0.9)


def _frame(d, n, spacing):
    """(side, rows) of an n-point patch: in 3-D a square of side `side`, in 2-D `rows` rows 2 apart, `side` long."""
    if d == 3:
        return spacing * n ** 0.5, 1
    rows = max(1, int(round((spacing * n / 2.0) ** 0.5)))
    return spacing * n / rows, rows


def _on_surface(d, u, v):
    """Points of the surface at (u, v): v is the second coordinate in 3-D and the row number in 2-D."""
    if d == 3:
        return np.stack([u, v, _height(u, v)], axis=1)
    return np.stack([u, 2.0 * v + 0.05 * np.sin(u * 1.3)], axis=1)


def _patch(d, n, rng, side, rows, noise=0.004):
    u = rng.uniform(0, side, n)
    v = rng.uniform(0, side, n) if d == 3 else rng.integers(0, rows, n).astype(np.float64)
    return _on_surface(d, u, v) + rng.normal(0, noise, (n, d))


def isolated_pair(d, n, seed=0):
    """(source, target, isolated source rows, isolated target rows), n points each.  Both clouds sample one
    surface, the source moved 0.45 of its length along the first axis: the far 0.45 of the target has no source
    near it and carries the source's first isolated points (spaced 0.6: farther than DEC_D_N from every other source
    point, within DEC_D_C of the target's surface points), likewise the target's on the source's far end; 30 more
    isolated points of each cloud lie in pairs, 0.5 apart, on a line far from both."""
    rng = np.random.default_rng([23, d, n, seed])
    side, rows = _frame(d, n, SPACING)
    shift = 0.45 * side

    def grid(u0):
        us = u0 + 0.6 * np.arange(3)
        vs = 0.3 + 0.6 * np.arange(8) if d == 3 else np.arange(min(rows, 8), dtype=np.float64)
        uu, vv = np.meshgrid(us, vs, indexing="ij")
        return uu.ravel(), vv.ravel()

    su, sv = grid(0.3)                                  # source rows on the target's own end
    tu, tv = grid(side + 0.6)                           # target rows on the source's far end (in the target's frame)
    iso_s = _on_surface(d, su, sv) + rng.normal(0, 0.004, (len(su), d))
    iso_t = _on_surface(d, tu - shift, tv) + rng.normal(0, 0.004, (len(tu), d))
    iso_t[:, 0] += shift
    line = np.zeros((30, d))
    line[:, 0] = 2.0 * side + 3.0 + 0.5 * np.arange(30)
    line[:, 1] = -10.0
    pair_s = line + np.array([0.05, -0.03, 0.02][:d])
    n_patch_s = n - len(iso_s) - 30
    n_patch_t = n - len(iso_t) - 30
    ps = _patch(d, n_patch_s, rng, side, rows)
    ps[:, 0] += shift
    pt = _patch(d, n_patch_t, rng, side, rows)
    src = np.concatenate([ps, iso_s, pair_s])
    tgt = np.concatenate([pt, iso_t, line])
    order_s, order_t = rng.permutation(n), rng.permutation(n)     # isolated rows anywhere in the input order
    is_iso_s = np.zeros(n, dtype=bool)
    is_iso_s[n_patch_s:] = True
    is_iso_t = np.zeros(n, dtype=bool)
    is_iso_t[n_patch_t:] = True
    return src[order_s], tgt[order_t], is_iso_s[order_s], is_iso_t[order_t]


def decode_pose(d, src):
    R = O.rot2(np.deg2rad(0.2)) if d == 2 else O.so3_exp(np.deg2rad(0.2) * np.array([0.2, -0.3, 0.93]))
    return E.pose_about(src.mean(axis=0), R, [0.01, -0.015, 0.005][:d])


def offset_case(d, n):
    """(source [n, d], target [2000, d], three poses): a 2000-point target at 5 cm spacing, 1e5 from the origin; the
    source is the n target points nearest its centroid, 2 mm of noise; the poses: the identity (a cold cache: every
    tile walks), 0.04 mm away (the walk's certificates hold), then 1.5 degrees and centimetres away (the graph descent)."""
    rng = np.random.default_rng([29, d, n])
    side, rows = _frame(d, 2000, OFF_SPACING)
    u = rng.uniform(0, side, 2000)
    if d == 3:
        v = rng.uniform(0, side, 2000)
        tgt = np.stack([u, v, 0.4 * _height(u / 0.4, v / 0.4)], axis=1)
    else:
        r = rng.integers(0, rows, 2000)
        tgt = np.stack([u, 0.8 * r + 0.02 * np.sin(u * 3.0)], axis=1)
    tgt = tgt + rng.normal(0, 0.002, tgt.shape) + OFF_T[:d]
    c = tgt.mean(axis=0)
    near = np.argsort(np.linalg.norm(tgt - c, axis=1), kind="stable")[:n]
    src = tgt[near] + rng.normal(0, 0.002, (n, d))
    return src, tgt, _moving_poses(d, src.mean(axis=0))


def _moving_poses(d, centre, last_turn=1.5):
    def turn(deg):
        if d == 2:
            return O.rot2(np.deg2rad(deg))
        return O.so3_exp(np.deg2rad(deg) * np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5]))

    # (a walk certifies its nearest against a runner-up gap of at most kappa = 0.002 d_c = 0.2 mm: the second pose moves
    # every point by 0.04 mm, less than half of it)
    return [np.eye(d + 1), E.rigid(d, None, [3e-5, -2e-5, 1e-5][:d]),
            E.pose_about(centre, turn(last_turn), [0.03, -0.02, 0.015][:d])]


FULL_GROUPS, FULL_TILE = 16, 64


def full_tile_case(d):
    """(source [1024, d], target, three poses): source tiles of exactly 64 points, 1e5 from the origin.  The source is
    16 groups of 64 points whose every coordinate increases strictly along the cloud (steps of 5 to 10 cm inside a
    group, the same in every group, groups 8 apart), so the sorted order is the input order and each group is one
    tile (stats_epilogue_cases.py explains why); the target is the source, shuffled, 2 mm of noise."""
    rng = np.random.default_rng([37, d])
    steps = rng.uniform(0.05, 0.10, (FULL_TILE, d))
    steps[0] = 0.0
    group = np.cumsum(steps, axis=0)
    src = np.concatenate([group + 8.0 * c for c in range(FULL_GROUPS)]) + OFF_T[:d]
    tgt = (src + rng.normal(0, 0.002, src.shape))[rng.permutation(len(src))]
    return src, tgt, _moving_poses(d, src.mean(axis=0), last_turn=0.02)   # (the cloud is 130 long)


def offset_cases():
    """(key, source, target, poses) of every moving sequence."""
    for d in (3, 2):
        for n in OFF_FILLS:
            yield (f"offset_{d}d_n{n}",) + offset_case(d, n)
        yield (f"offset_{d}d_full",) + full_tile_case(d)


def boundary_case(d, n):
    """(source, target, pose), n points a side: a patch of side 1 (2-D: up to two rows), the source the target's
    points with 4 mm of noise."""
    rng = np.random.default_rng([31, d, n])
    tgt = _patch(d, n, rng, 1.0, 2)
    src = tgt + rng.normal(0, 0.004, (n, d))
    return src, tgt, E.rigid(d, None, [0.01, -0.02, 0.015][:d])


# ----------------------------------------------------------------------------- engine call sequences
def engine_pass(gicp, eng, src, tgt, T, p_src, p_tgt, shard=0, nshards=1):
    """Both clouds set afresh (a cold cache), then one pass at T with the per-point outputs."""
    eng.set_target(tgt, p_tgt)
    eng.set_source(src, p_src, shard=shard, nshards=nshards)
    return eng.iterate(T, debug=True)


def moving_sequence(gicp, eng, src, tgt, poses, p):
    """Both clouds set afresh, then one pass per pose on the warming cache: [(statistics, debug, pass_info)]."""
    eng.set_target(tgt, p)
    eng.set_source(src, p)
    out = []
    for T in poses:
        st, dbg = eng.iterate(T, debug=True)
        out.append((st, dbg, eng.pass_info()))
    return out


INFO_KEYS = ("ambiguous", "pairs", "list_rebuilds", "sum_sq", "graph_proved", "walked_tiles")


def info_words(info):
    return words(np.array([info[k] for k in INFO_KEYS], dtype=np.float64))


# ----------------------------------------------------------------------------- raw words and digests
def words(a):
    """The array's 64-bit words (float64 and int64 alike)."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 8
    return a.view(np.uint64).reshape(a.shape).copy()


def row_sums(a):
    """One 32-bit checksum per row of a [n, ...] array of 64-bit words: sum over the row of word k times the k-th odd
    constant, modulo 2^64, the two halves added."""
    w = words(a).reshape(len(a), -1)
    k = (2 * np.arange(w.shape[1], dtype=np.uint64) + 1) * np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        s = (w * k[None, :]).sum(axis=1, dtype=np.uint64)
    return ((s >> np.uint64(32)) + (s & np.uint64(0xFFFFFFFF))).astype(np.uint32)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def digest(rec, key, a):
    rec[key + ".rows"] = row_sums(a)
    rec[key + ".sha"] = sha(a)


# ----------------------------------------------------------------------------- what the golden file holds
def decode_cases():
    for d in (2, 3):
        for rk, ratio in RATIOS.items():
            for model in MODELS:
                yield f"decode_{d}d_{rk}_{model}", d, ratio, model


def record_all(gicp, eng, log=print):
    """Every golden entry of the build `eng` runs on: {key: array}."""
    rec = {}
    for key, d, ratio, model in decode_cases():
        src, tgt, _, _ = isolated_pair(d, DEC_N)
        ps = params(gicp, d, EPS_SRC, ratio, DEC_D_C, DEC_D_N, model)
        pt = params(gicp, d, EPS_TGT, ratio, DEC_D_C, DEC_D_N, model)
        st, dbg = engine_pass(gicp, eng, src, tgt, decode_pose(d, src), ps, pt)
        rec[key + ".stats"] = words(st)
        rec[key + ".index"] = dbg["index"].astype(np.int32)
        digest(rec, key + ".weight", dbg["weight"])
        if model == MODELS[0]:
            ck = f"decode_{d}d_{'r0' if ratio is None else 'r1'}"
            digest(rec, ck + ".cov_source", eng.covariances("source"))
            digest(rec, ck + ".cov_target", eng.covariances("target"))
        log(f"{key}: accepted {int(np.sum(dbg['index'] >= 0))} of {len(src)}")
    for d in (2, 3):
        src, tgt, _, _ = isolated_pair(d, SHARD_N)
        ps = params(gicp, d, EPS_SRC, None, DEC_D_C, DEC_D_N)
        pt = params(gicp, d, EPS_TGT, None, DEC_D_C, DEC_D_N)
        T = decode_pose(d, src)
        parts = [engine_pass(gicp, eng, src, tgt, T, ps, pt, shard=r, nshards=2)[0] for r in (0, 1)]
        rec[f"shard_{d}d.stats_sum"] = words(parts[0] + parts[1])
        log(f"shard_{d}d: counts {parts[0][-1]:.0f} + {parts[1][-1]:.0f}")
    for key, src, tgt, poses in offset_cases():
        p = params(gicp, src.shape[1], EPS_SRC, None, OFF_D_C, OFF_D_N)
        for k, (st, dbg, info) in enumerate(moving_sequence(gicp, eng, src, tgt, poses, p)):
            rec[f"{key}_p{k}.stats"] = words(st)
            rec[f"{key}_p{k}.info"] = info_words(info)
            log(f"{key}_p{k}: accepted {int(np.sum(dbg['index'] >= 0))} of {len(src)}, "
                + ", ".join(f"{a} {b:g}" for a, b in info.items()))
    return rec
