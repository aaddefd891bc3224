"""Clouds of uneven density and outlier-stretched extent, and their CPU preconditions' helpers (no GPU
import; test_density_ref_cpu.py checks every property the GPU tests of test_gpu_density.py rely on).

Three regimes the uniformly sampled fixtures never reach:

  collapsed Morton grid   a handful of far returns stretches the extent until the whole core shares one grid
                          cell of a build (10 bits per axis in 3-D, 16 in 2-D): tiles become runs of 64 points
                          in original order, every tile's box is the core, every candidate list overflows;
  rho-dominated margin    a sparse halo gives tiles kilometres wide, so the screen's margin in the dense core
                          comes from the largest tile radius, not from d_c;
  range-dependent density a spinning-LiDAR frame: neighbour spacing from centimetres to most of a metre,
                          neighbourhoods cut by d_n and by k in one cloud, collinear far rings.

Every fixture is built from gicp.synthetic with fixed seeds and its rows are shuffled by a fixed permutation,
so that original order is unrelated to position."""
import functools

import numpy as np

import edge_ref as E
from gicp import synthetic as S
from oracle import gicp_oracle as O

OFFSET = np.array([451234.5, 5402187.25, 123.0])        # test_large_coordinate_offsets' map-frame offset
N_FAR = 12
FAR_3D = 1e5                                            # half-width of the far points' cube, m
FAR_2D = 2.0 ** 27                                      # ... px
HALO = 1e4

FIXTURES = ("stretched_3d", "offset_origin_3d", "halo_3d", "lidar_small", "stretched_2d")
COLLAPSED = ("stretched_3d", "offset_origin_3d", "stretched_2d")

# Points of each cloud that the entrywise covariance comparison leaves out: a surface exists and the relative
# eigen-gap of the ORACLE's neighbourhood is below 1e-2 (E.covariance_report on the oracle's own output: a
# figure of the cloud and the oracle alone, as LEFT_OUT_ROOM_D_N_1 of test_gpu_history.py).
# test_density_ref_cpu.py asserts these counts exactly.
LEFT_OUT = {
    ("stretched_3d", "source"): 141, ("stretched_3d", "target"): 160,
    ("offset_origin_3d", "source"): 141, ("offset_origin_3d", "target"): 160,
    ("halo_3d", "source"): 197, ("halo_3d", "target"): 194,
    ("lidar_small", "source"): 1238, ("lidar_small", "target"): 1235,
    ("stretched_2d", "source"): 0, ("stretched_2d", "target"): 0,
}


def max_left_out(name, which):
    """LEFT_OUT as the share check_covariances takes (half a point above the count: no rounding at the edge)."""
    return (LEFT_OUT[name, which] + 0.5) / len(fixture(name)[which])


def _far(seed, dim, half, low_extra):
    """N_FAR points uniform in the +-half cube; the first sits at -(half + low_extra) on every axis and the
    second at +half, so the extent, and with it the grid, is fixed by these two."""
    far = np.random.default_rng(seed).uniform(-half, half, (N_FAR, dim))
    far[0] = -(half + low_extra)
    far[1] = half
    return far


def _mix(core, extra, seed):
    """core and extra in one cloud, rows shuffled by a fixed permutation: (points, mask of the core rows)."""
    pts = np.concatenate([core, extra])
    is_core = np.arange(len(pts)) < len(core)
    perm = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), is_core[perm]


def _fixture(name):
    if name in ("stretched_3d", "offset_origin_3d", "halo_3d"):
        src, tgt, _ = S.scene_pair_3d(8000)
        dim, d_c, d_n, scale = 3, 0.5, 1.0, 1.0
        if name == "stretched_3d":
            # the room, 40 m wide, lies 100040 .. 100080 m above the lowest corner: inside cell 512 of the
            # 1024 cells of 195.4 m, not across a boundary
            xs, xt = _far(101, 3, FAR_3D, 60.0), _far(102, 3, FAR_3D, 60.0)
        elif name == "offset_origin_3d":
            src, tgt = src + OFFSET, tgt + OFFSET
            xs = np.random.default_rng(103).uniform(-0.5, 0.5, (N_FAR, 3))     # invalid returns: (0, 0, 0) and about
            xt = np.random.default_rng(104).uniform(-0.5, 0.5, (N_FAR, 3))
        else:
            src, tgt = src[:6000], tgt[:6000]
            # (the seeds are chosen so that the grid, whose origin is the halo's lowest point, cuts the room into
            # few cells: the fullest cell must hold 1000 points, test_density_ref_cpu.py)
            xs = np.random.default_rng(135).uniform(-HALO, HALO, (2000, 3))
            xt = np.random.default_rng(136).uniform(-HALO, HALO, (2000, 3))
    elif name == "stretched_2d":
        # (a motion of 0.04 rad and (8, -6) px between the clouds: with the generator's default 0.02 rad and
        # (2, -1) px 98.5 % of the source is accepted at d_c = 20 along the whole sequence, above the 95 % the
        # preconditions allow; with this one 74 .. 86 %)
        src, tgt, _ = S.segment_scene_2d(6000, theta=0.04, t=(8.0, -6.0))
        dim, d_c, d_n, scale = 2, 20.0, 25.0, 40.0
        # the 1000 px scene lies 2^27 + 3000 .. 2^27 + 4000 px above the lowest corner: inside cell 32768 of the
        # 65536 cells of 4096.05 px
        xs, xt = _far(107, 2, FAR_2D, 3000.0), _far(108, 2, FAR_2D, 3000.0)
    elif name == "lidar_small":
        frames = [f for f, _ in S.lidar_stream(3, beams=32, azimuths=250)]
        src, tgt = frames[1], frames[2]
        dim, d_c, d_n, scale = 3, 0.5, 1.0, 1.0
        xs = xt = np.zeros((0, 3))
    else:
        raise KeyError(name)
    seed = 200 + 2 * FIXTURES.index(name)
    source, core_s = _mix(src, xs, seed)
    target, core_t = _mix(tgt, xt, seed + 1)
    out = dict(name=name, dim=dim, d_c=d_c, d_n=d_n, step_scale=scale, source=source, target=target,
               core_source=core_s, core_target=core_t, bits=10 if dim == 3 else 16)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dict(name, dim, d_c, d_n, step_scale, bits, source, target, core_source, core_target): the clouds (read
    only), the masks of their core rows (the room, the scene, the frame; the rest are the far points, the points
    about the origin or the halo), and the parameters the tests run them with."""
    return _fixture(name)


def core_only(name):
    """(source, target) without the far points or the halo, rows in the fixture's order: the sibling the regime
    conditions compare with."""
    f = fixture(name)
    return (np.ascontiguousarray(f["source"][f["core_source"]]),
            np.ascontiguousarray(f["target"][f["core_target"]]))


def params_kw(f):
    return dict(max_distance_correspondence=f["d_c"], max_distance_nearest_neighbors=f["d_n"])


def grid_cells(points, bits):
    """The quantisation of a cloud build (begin_build / build_core), restated: lo the per-axis minimum, ext the
    largest extent of any axis times (1 + 1e-9) plus 1e-12 (1 + |min_x|), cell of a point per axis
    floor(clip((p - lo) 2^bits / ext, 0, 2^bits - 1)).  Returns int64 [n, d]."""
    p = np.asarray(points, dtype=np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = np.max(hi - lo) * (1.0 + 1e-9) + 1e-12 * (1.0 + abs(lo[0]))
    q = (p - lo) * (2.0 ** bits / ext)
    return np.floor(np.clip(q, 0.0, 2.0 ** bits - 1.0)).astype(np.int64)


STEPS = (0.0, 0.002, 0.01, 0.03, 0.08, 0.15, 0.01, 0.001)


def moving_poses(f):
    """The 8 poses of test_graph_descent_along_a_moving_pose (steps of millimetres to 15 cm with a turn of 0.2 rad
    per metre about a changing axis, then back), applied about the centroid of the source's core; the
    translations times step_scale (px in 2-D)."""
    d = f["dim"]
    centre = f["source"][f["core_source"]].mean(axis=0)
    out = []
    for k, step in enumerate(STEPS):
        if d == 3:
            R = S.axis_angle([1.0, 0.5 * k, -0.3], step * 0.2)
            t = np.array([step, -0.5 * step, 0.25 * step])
        else:
            R = O.rot2(step * 0.2)
            t = np.array([step, -0.5 * step])
        out.append(E.pose_about(centre, R, t * f["step_scale"]))
    return out
