"""C5 (BASELINE.json configs[4]): scan-to-scan odometry over a synthetic spinning-LiDAR stream
(64 x 1563 rays ~ 100k points per frame) through the C2 room, one MI355X.

    python bench_odometry.py [--frames 1000] [--max-iterations 30] [--fixed]
    python bench_odometry.py --map-voxel 0.4 --map-range 30     # the same stream, scan-to-map
    python bench_odometry.py --skew [--deskew]                  # sweeps measured while the sensor moves (§3m)

Prints one JSON line: GICP iterations/sec over the registration loops, frames/sec end to end
(upload + index + covariances + registration per frame), setup per frame, and the trajectory
error against the generating poses.  Scans are generated before the timed stream (on the GPU
through torch when available — data plumbing, not the measured path)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "generalized-icp_amd"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1563)
    ap.add_argument("--max-iterations", type=int, default=30)
    ap.add_argument("--fixed", action="store_true", help="fixed iterations (convergence disabled)")
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--sync", action="store_true", help="build each scan when needed (no staged double buffer)")
    ap.add_argument("--kernel-times", action="store_true", help="keep the library's sampled per-launch HIP events")
    ap.add_argument("--copy", action="store_true",
                    help="staged scans copied by the library before stage_target returns (the default for callers "
                         "that refill their buffer); without it the bench, which holds every frame untouched in "
                         "memory, lends them (GICP_STAGE_BORROW: no copy on the calling thread)")
    ap.add_argument("--voxel-size", type=float, default=None,
                    help="voxel-filter every scan on the device before it is indexed (metres; default: off)")
    ap.add_argument("--map-voxel", type=float, default=None,
                    help="scan-to-map mode: every scan is registered against a local voxel map of this leaf (metres) "
                         "and merged into it (needs --map-range; default: scan-to-scan)")
    ap.add_argument("--map-range", type=float, default=None, help="reach of the local map from the sensor (metres)")
    ap.add_argument("--map-min-points", type=int, default=1, help="voxels with fewer points are not registered against")
    ap.add_argument("--skew", action="store_true",
                    help="every ray is cast from the pose the sensor has at its stamp (synthetic.lidar_stream_skewed, "
                         "generated with NumPy); poses are compared at mid-sweep")
    ap.add_argument("--deskew", action="store_true",
                    help="de-skew every scan on the device as part of its build (Odometry(deskew=True); needs --skew)")
    ap.add_argument("--report", action="store_true",
                    help="evaluate every registration on the device (Odometry(report=...)): thresholds d_c / 4, d_c / 2, "
                         "d_c and the quantiles 0.5 and 0.9")
    a = ap.parse_args()
    if a.deskew and not a.skew:
        ap.error("--deskew needs --skew (the plain stream carries no stamps)")
    if (a.map_voxel is None) != (a.map_range is None):
        ap.error("--map-voxel and --map-range go together")
    from gicp import synthetic as S
    from gicp.odometry import Odometry
    xp, dev = None, None
    try:
        import torch
        if torch.cuda.is_available():
            xp, dev = torch, "cuda"
    except ImportError:
        pass
    t0 = time.perf_counter()
    if a.skew:
        frames = list(S.lidar_stream_skewed(a.frames, a.beams, a.azimuths))
        if not a.deskew:   # the skewed points as they are: the stamps are dropped
            frames = [(np.ascontiguousarray(f[:, :3]), P) for f, P in frames]
    else:
        frames = list(S.lidar_stream(a.frames, a.beams, a.azimuths, xp=xp, device=dev))
    gen_s = time.perf_counter() - t0
    kw = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
    dc = kw["max_distance_correspondence"]
    import gicp
    p = gicp.default_params(3, max_iterations=a.max_iterations, tolerance=a.tolerance,
                            fixed_iterations=1 if a.fixed else 0, **kw)
    if not a.kernel_times:
        # no per-launch HIP event pairs (a diagnostic the line does not report: each pair is queue work between
        # two launches); --kernel-times keeps the library default (every 8th launch timed)
        p.timing_stride = -1
    odo = Odometry(3, params=p, borrow=not a.copy, voxel_size=a.voxel_size, map_voxel_size=a.map_voxel,
                   map_range=a.map_range, map_min_points=a.map_min_points, deskew=a.deskew,
                   report=dict(thresholds=[dc / 4, dc / 2, dc], quantiles=[0.5, 0.9]) if a.report else None)
    # warm-up on the first two frames (library init, allocation), then restart the stream
    odo.step(frames[0][0])
    odo.step(frames[1][0], frames[2][0])
    odo.step(frames[2][0])
    odo.reset()   # same device context and buffers, fresh stream
    t1 = time.perf_counter()
    scans = [f for f, _ in frames]
    stream = (odo.step(s) for s in scans) if a.sync else odo.run(scans)
    results = list(stream)        # the timed stream (the accuracy is evaluated below)
    Ts = [T for T, _ in results]
    final_pose = odo.pose         # inside the timed region: flushes the per-frame pose compositions
    wall = time.perf_counter() - t1
    errs = []
    for k, T in enumerate(Ts):
        if T is not None:
            Ttrue = np.linalg.inv(frames[k][1]) @ frames[k - 1][1]
            errs.append((S.rotation_angle_error(T, Ttrue), S.translation_error(T, Ttrue)))
    P0 = frames[0][1]
    est_end = P0 @ final_pose
    true_end = frames[-1][1]
    errs = np.asarray(errs)
    it = odo.timing["iterations"]
    line = {
        "metric": "GICP iterations/sec, scan-to-scan odometry stream (C5)",
        "value": it / odo.timing["align_s"],
        "unit": "it/s",
        "n_gpus": 1,
        "frames": a.frames,
        "frames_per_s": (a.frames - 1) / wall,
        "iterations_total": it,
        "iterations_per_frame": it / max(1, a.frames - 1),
        "setup_ms_per_frame": odo.timing["setup_s"] * 1e3 / a.frames,
        "align_ms_per_frame": odo.timing["align_s"] * 1e3 / max(1, a.frames - 1),
        "higher_is_better": True,
        "dtype": "f32-screen+f64",
        "data": f"synthetic spinning LiDAR, {a.beams}x{a.azimuths} rays, C2 room (generated in {gen_s:.1f} s, "
                f"{'torch/' + dev if xp else 'numpy'})",
        "pipeline": "synchronous builds" if a.sync else
        ("coming scans staged on their own streams during the registrations before them, " +
         ("copied by the library (stage_target copy)" if a.copy else "lent to the library (GICP_STAGE_BORROW)")),
        "accuracy": "model-limited: per-frame error is the reference's covariance model's (the GPU equals the "
                    "oracle per frame), see frame_error",
        "config": {"workload": f"c5_lidar_{a.frames}f", "points_per_frame": int(np.mean([len(f[0]) for f in frames])),
                   "trajectory": "0.5 m and 0.5 deg yaw per frame (+-10 %), SURVEY.md 8(d)",
                   "max_iterations": a.max_iterations, "fixed_iterations": bool(a.fixed), **kw},
        "frame_error": {"rot_rad_median": float(np.median(errs[:, 0])), "rot_rad_max": float(errs[:, 0].max()),
                        "trans_median": float(np.median(errs[:, 1])), "trans_max": float(errs[:, 1].max()),
                        "note": "model-limited: the reference's covariance model (eps (I - n n^T) + 0.1 eps n n^T, "
                                "SURVEY.md 8.A) under-registers the yaw step on these scans; the GPU equals the "
                                "oracle frame by frame (tests/test_odometry.py::test_full_size_stream_per_frame_vs_oracle)"},
        "drift": {"trans": float(np.linalg.norm(est_end[:3, 3] - true_end[:3, 3])),
                  "rot_rad": S.rotation_angle_error(est_end, true_end),
                  "path_length": float(sum(np.linalg.norm(frames[k][1][:3, 3] - frames[k - 1][1][:3, 3])
                                           for k in range(1, len(frames))))},
    }
    if a.skew:
        est = [P0 @ P for P in odo.poses]
        pos_err = [float(np.linalg.norm(E[:3, 3] - f[1][:3, 3])) for E, f in zip(est, frames)]
        line["data"] = f"synthetic spinning LiDAR, {a.beams}x{a.azimuths} rays, C2 room, every ray cast from the pose at " \
                       f"its stamp (generated in {gen_s:.1f} s, numpy)"
        line["skew"] = {"deskew": bool(a.deskew), "pose_reference_stamp": 0.5,
                        "pose_error_final": pos_err[-1], "pose_error_median": float(np.median(pos_err[1:])),
                        "pose_error_max": float(np.max(pos_err))}
    if a.report:
        reps = [r["report"] for _, r in results if r is not None]
        line["report"] = {"ms_per_frame": odo.timing["report_s"] * 1e3 / max(1, a.frames - 1),
                          "share_of_frame": odo.timing["report_s"] / wall,
                          "thresholds": [dc / 4, dc / 2, dc],
                          "fitness_median": np.median([r["fitness"] for r in reps], axis=0).tolist(),
                          "inlier_rmse_median": np.median([r["inlier_rmse"] for r in reps], axis=0).tolist(),
                          "dist_q50_median": float(np.median([r["dist_q"][0.5] for r in reps])),
                          "dist_q90_median": float(np.median([r["dist_q"][0.9] for r in reps])),
                          "eig_min_median": float(np.median([r["eig"][0] for r in reps]))}
    if a.voxel_size is not None:
        line["voxel"] = {"voxel_size": a.voxel_size, "points_last_frame": odo.eng.cloud_size("source" if a.map_voxel else "target")}
    if a.map_voxel is not None:
        tm, nf = odo.timing, a.frames
        line["metric"] = "GICP iterations/sec, scan-to-map odometry stream (C5)"
        line["pipeline"] = "scan-to-map: source build, align against the map, insert, synchronous target rebuild"
        line["map"] = {"voxel_size": a.map_voxel, "range": a.map_range, "min_points": a.map_min_points,
                       "voxels_last_frame": odo.eng.map_size(), "target_points_last_frame": odo.eng.cloud_size("target"),
                       "source_build_ms_per_frame": tm["setup_s"] * 1e3 / nf,
                       "align_ms_per_frame": tm["align_s"] * 1e3 / max(1, nf - 1),
                       "insert_ms_per_frame": tm["map_insert_s"] * 1e3 / nf,
                       "target_rebuild_ms_per_frame": tm["map_target_s"] * 1e3 / nf}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
