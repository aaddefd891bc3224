"""Batched registration: problems per second of gicp_batch_align against the same problems run one
after another through Engine.set_target / set_source / align on the same GPU in the same process -- the code path a
caller had before there was a batch.

    python bench_batch.py [--reps 5] [--warmup 2]

Workloads:
  fixtures_2d   B in {1, 16, 256, 1024} problems cycled over the eleven convergent 2-D scan pairs of the reference's
                demos (tests/golden/*.npz, 33-203 points), each from the identity with its fixture's own parameters.
                One gicp_params serves a batch, so a batch here is two gicp_batch_align calls, one per parameter
                set (the robot pairs, the static demo's pairs); both are inside the timed region.
  r360          B = 256 problems cycled over the three 360-ray robot pairs (131-203 points): one call.
  room_3d       B in {16, 256} starts (yaw and shift perturbed) of one 3-D pair of 1500 / 1400 points: one call.
Whole calls are timed on the host (uploads, launches, the synchronisation, results), median of --reps after
--warmup.  The sequential loop is timed the same way; `sequential_align_ms` is the part of it spent inside
Engine.align alone (what remains when the clouds are already resident).  Every batch result is checked against
its sequential twin (iterations and correspondences equal).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "generalized-icp_amd"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

PAIRS = ["robot_p0_r360", "robot_p1_r360", "robot_p2_r360", "robot_p0_r90", "robot_p1_r90", "robot_p2_r90",
         "vis_s0", "vis_s1", "vis_s2", "vis_s3", "vis_s5"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import gicp
    from gicp import synthetic as S
    from golden_util import kwargs, load

    eng = gicp.Engine(0)
    seq = gicp.Engine(0)
    fx = {}
    for name in PAIRS:
        f = load(name)
        fx[name] = (np.ascontiguousarray(f["source"], dtype=np.float64), np.ascontiguousarray(f["target"], dtype=np.float64),
                    kwargs(f))

    def fixture_groups(names, B):
        """The B problems cycled over `names`, grouped by parameter set: [(params, clouds, pairs, T0)]."""
        groups = {}
        for b in range(B):
            src, tgt, kw = fx[names[b % len(names)]]
            g = groups.setdefault(tuple(sorted(kw.items())), dict(kw=kw, clouds=[], slot={}, pairs=[]))
            nm = names[b % len(names)]
            if nm not in g["slot"]:
                g["slot"][nm] = len(g["clouds"])
                g["clouds"] += [src, tgt]
            g["pairs"].append((g["slot"][nm], g["slot"][nm] + 1))
        return [(gicp.default_params(2, **g["kw"]), g["clouds"], g["pairs"], None) for g in groups.values()]

    def room_groups(B):
        src, tgt, _ = S.scene_pair_3d(1500, 1400, scene=S.room_scene(seed=1, size=(6, 6, 3), n_boxes=3, n_spheres=2))
        rng = np.random.default_rng(3)
        T0 = np.tile(np.eye(4), (B, 1, 1))
        for b in range(B):
            T0[b, :3, :3] = S.axis_angle([0.0, 0.0, 1.0], np.deg2rad(rng.uniform(-1.5, 1.5)))
            T0[b, :3, 3] = rng.uniform(-0.03, 0.03, 3)
        p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
        return [(p, [src, tgt], [(0, 1)] * B, T0)]

    def run_batch(groups):
        out = []
        for p, clouds, pairs, T0 in groups:
            out += eng.align_batch(clouds, pairs, T0, p)[1]
        return out

    def run_sequential(groups):
        out, t_align = [], 0.0
        for p, clouds, pairs, T0 in groups:
            for b, (s, t) in enumerate(pairs):
                seq.set_target(clouds[t], p)
                seq.set_source(clouds[s], p)
                t0 = time.perf_counter()
                out.append(seq.align(None if T0 is None else T0[b], p)[1])
                t_align += time.perf_counter() - t0
        return out, t_align * 1e3

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        walls, last = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            last = fn()
            walls.append((time.perf_counter() - t0) * 1e3)
        return walls, last

    rows = []
    work = [("fixtures_2d", B, fixture_groups(PAIRS, B)) for B in (1, 16, 256, 1024)]
    work.append(("r360", 256, fixture_groups(PAIRS[:3], 256)))
    work += [("room_3d", B, room_groups(B)) for B in (16, 256)]
    for name, B, groups in work:
        wb, rb = timed(lambda: run_batch(groups))
        ws, (rs, _) = timed(lambda: run_sequential(groups))
        al = [run_sequential(groups)[1] for _ in range(max(1, a.reps // 2))]
        same = all(x["iterations"] == y["iterations"] and x["correspondences"] == y["correspondences"] for x, y in zip(rb, rs))
        mb, ms = statistics.median(wb), statistics.median(ws)
        rows.append({"workload": name, "problems": B, "calls_per_batch": len(groups),
                     "points": sorted({len(c) for g in groups for c in g[1]}),
                     "iterations_mean": round(float(np.mean([r["iterations"] for r in rb])), 2),
                     "batch_ms": round(mb, 3), "batch_ms_min_max": [round(min(wb), 3), round(max(wb), 3)],
                     "batch_problems_per_s": round(B / mb * 1e3, 1),
                     "sequential_ms": round(ms, 3), "sequential_ms_min_max": [round(min(ws), 3), round(max(ws), 3)],
                     "sequential_problems_per_s": round(B / ms * 1e3, 1),
                     "sequential_align_ms": round(statistics.median(al), 3),
                     "speedup": round(ms / mb, 2), "speedup_over_align_alone": round(statistics.median(al) / mb, 2),
                     "results_match_sequential": bool(same)})
    eng.close()
    seq.close()
    print(json.dumps({"metric": "batched registration: problems per second, one launch against sequential calls",
                      "unit": "problems/s", "higher_is_better": True, "reps": a.reps, "warmup": a.warmup,
                      "max_points": gicp.batch_max_points(3), "workloads": rows,
                      "note": "host wall time of whole calls, median; sequential = Engine.set_target + set_source + "
                              "align per problem on the same GPU in the same process"}))


if __name__ == "__main__":
    main()
