"""Inputs shared by the batched-registration tests (test_batch_cpu.py checks their preconditions with the oracle,
test_gpu_batch.py runs them on the GPU): the convergent 2-D fixtures, the small 3-D room pair, the covariance
clouds of every size, and the oracle's |delta loss| around the stopping iteration."""
import functools

import numpy as np

import edge_ref as E
from golden_util import kwargs, load
from oracle import gicp_oracle as O

# the eleven fixtures of the reference's demos whose run converges (bench_small.py PAIRS)
FIXTURES = ["robot_p0_r360", "robot_p1_r360", "robot_p2_r360", "robot_p0_r90", "robot_p1_r90", "robot_p2_r90",
            "vis_s0", "vis_s1", "vis_s2", "vis_s3", "vis_s5"]
P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)   # (gpu_helpers.P3)
COV_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2048)    # the last: gicp_batch_max_points
ROOM_ITERATIONS = 8                                    # the iteration the room pair converges at


@functools.lru_cache(maxsize=None)
def fixture(name):
    fx = load(name)
    return np.ascontiguousarray(fx["source"], dtype=np.float64), np.ascontiguousarray(fx["target"], dtype=np.float64), kwargs(fx)


@functools.lru_cache(maxsize=None)
def room_pair():
    """The small 3-D pair: 1500 / 1400 points of a 6 x 6 x 3 m room (seed pinned: other seeds of so small a room
    can raise in the generator)."""
    from gicp import synthetic as S
    src, tgt, Tgt = S.scene_pair_3d(1500, 1400, scene=S.room_scene(seed=1, size=(6, 6, 3), n_boxes=3, n_spheres=2))
    return src, tgt, Tgt


@functools.lru_cache(maxsize=None)
def cov_cloud(dim, n):
    """The covariance cloud of n rows: 3-D the first n of 2048 points of the small room, 2-D the first n of a
    dense patch of 2048 (edge_ref.dense_patch: gently curved rows)."""
    if dim == 3:
        from gicp import synthetic as S
        pts = S.scene_pair_3d(2048, 2048, scene=S.room_scene(seed=1, size=(6, 6, 3), n_boxes=3, n_spheres=2))[0]
    else:
        pts = E.dense_patch(2, 2048, 2048, seed=5)[0]
    return np.ascontiguousarray(pts[:n])


def oracle_cov_report(pts, d_n):
    """edge_ref.covariance_report of the oracle's own covariances: how many points the entrywise criterion must
    leave out (surface points whose eigen-gap is below 1e-2) whatever computes them."""
    C, cnt = O.covariances(pts, d_n, faithful=False)
    return E.covariance_report(pts, d_n, O.default_k(pts.shape[1]), O.EPSILON, O.RATIO, pts.shape[1], C, cnt)


def loss_steps(src, tgt, **kw):
    """The oracle's loop with the batch's semantics (exact inner solve, rotated source covariances): the
    iteration it stops at, |delta loss| there and at the iteration before (inf at iteration 0)."""
    _, rec = O.gicp(src, tgt, inner="gn", source_cov="rotate", record=True, **kw)
    loss = [r["loss"] for r in rec["iterations"]]
    at = rec["converged_at"]
    step = [np.inf] + [abs(a - b) for a, b in zip(loss[:-1], loss[1:])]
    return at, step[at] if at >= 0 else None, step[at - 1] if at >= 1 else np.inf


# the PCL-rule cases (transformation_epsilon with the loss rule off): where the oracle stops, the same for half and
# for twice the epsilon (test_batch_cpu.py)
PCL_CASES = {"room": (1e-10, 8), "vis_s0": (1e-6, 13)}


def pcl_case(name):
    """(source, target, keyword arguments) of a PCL-rule case."""
    if name == "room":
        src, tgt, _ = room_pair()
        kw = dict(max_iterations=30, **P3)
    else:
        src, tgt, kw = fixture(name)
        kw = dict(kw)
    kw.update(tolerance=0.0, transformation_epsilon=PCL_CASES[name][0])
    return src, tgt, kw
