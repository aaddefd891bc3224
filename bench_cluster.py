"""Euclidean cluster extraction: the one-shot and the stage fused into a cloud build, beside the host
function and the route a caller had before it -- scipy's cKDTree.query_pairs plus connected_components.

    python bench_cluster.py [--room 1000000] [--room-radius 0.2] [--lidar-radius 0.5] [--min-size 10] [--reps 9]
                            [--warmup 2] [--host-reps 1] [--no-scipy] [--out profiles/cluster/bench.json]

Two clouds: the 3-D room of bench.py at --room rows, and one 64 x 1563 LiDAR frame of the synthetic stream.  Per cloud:
  one_shot_ms   gicp.cluster_points with labels, sizes and the kept index: upload, the stage, the copies back; host
                wall time, median of --reps after --warmup
  stage_ms      the stream-synchronised time of the stage inside Engine.set_target, from the build's own phase log
                (GICP_VERBOSE=1: every phase ends with a stream synchronisation), phase "cluster": keys, sort, gather,
                the edge pass, roots, scan, labels, compaction, the result words; median of --reps builds
  build_ms      the whole verbose build with the stage, and without it (the other phases are synchronised too, so both
                are slower than a plain build: they are there for the stage's added time, not as a frame time)
  host_ms       gicp.cluster_points_host, the library's union-find on the CPU; median of --host-reps
  scipy_ms      cKDTree(points).query_pairs(radius) + scipy.sparse.csgraph.connected_components, the tree built inside
                the timed region; median of --host-reps
  rounds        passes over the edges: 1 by construction (one lock-free pass, no "changed" word)
The numbers of clusters and of kept rows of every route are recorded, and whether device and host labels are the same
array; nothing is asserted.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "generalized-icp_amd"), ROOT]
os.environ["GICP_VERBOSE"] = "1"

import numpy as np  # noqa: E402

from bench_sor import logged_build  # noqa: E402


def timed(fn, reps, warmup=0):
    for _ in range(warmup):
        fn()
    walls, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(walls), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--room", type=int, default=1000000)
    ap.add_argument("--room-radius", type=float, default=0.2)
    ap.add_argument("--lidar-radius", type=float, default=0.5)
    ap.add_argument("--min-size", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster", "bench.json"))
    a = ap.parse_args()
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    import gicp
    from gicp import synthetic as S

    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
    _, room, _ = S.scene_pair_3d(a.room)
    frame = next(iter(S.lidar_stream(1)))[0]
    med = statistics.median
    rows = []
    for name, pts, radius in (("room", room, a.room_radius), ("lidar_frame", frame, a.lidar_radius)):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n = len(pts)
        eng = gicp.Engine(0)
        try:
            one_ms, (kept, idx, labels, sizes) = timed(
                lambda: eng.cluster_points(pts, radius, a.min_size, 0, return_index=True, return_labels=True, return_sizes=True),
                a.reps, a.warmup)
            plain = [logged_build(eng, pts, p)[0] for _ in range(a.warmup + a.reps)][a.warmup:]
            eng.set_cluster(radius, a.min_size, 0)
            runs = [logged_build(eng, pts, p) for _ in range(a.warmup + a.reps)][a.warmup:]
            kept_build = eng.cloud_size("target")
            eng.set_cluster(None)
        finally:
            eng.close()
        host_ms, (_, h_labels, h_sizes) = timed(
            lambda: gicp.cluster_points_host(pts, radius, a.min_size, 0, return_labels=True, return_sizes=True), a.host_reps)
        row = {"cloud": name, "rows": n, "radius": radius, "min_size": a.min_size, "rounds": 1,
               "one_shot_ms": round(one_ms, 3), "stage_ms": round(med([r[1]["cluster"] for r in runs]), 3),
               "build_ms_with_stage": round(med([r[0] for r in runs]), 3), "build_ms_without": round(med(plain), 3),
               "host_ms": round(host_ms, 3), "clusters": int(len(sizes)), "largest": int(sizes.max()),
               "singletons": int((sizes == 1).sum()), "kept": int(len(kept)), "kept_in_build": int(kept_build),
               "clusters_host": int(len(h_sizes)), "labels_equal_host": bool(np.array_equal(labels, h_labels)),
               "one_shot_over_host": round(host_ms / one_ms, 2)}
        if not a.no_scipy:
            def scipy_route():
                pairs = cKDTree(pts).query_pairs(radius, output_type="ndarray")
                g = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
                return connected_components(g, directed=False)[0], len(pairs)

            scipy_ms, (c_scipy, edges) = timed(scipy_route, a.host_reps)
            row.update({"scipy_ms": round(scipy_ms, 3), "clusters_scipy": int(c_scipy), "edges": int(edges),
                        "one_shot_over_scipy": round(scipy_ms / one_ms, 2)})
        rows.append(row)
    res = {"metric": "Euclidean cluster extraction: one-shot wall time and stream-synchronised stage time of a fused build",
           "unit": "ms", "higher_is_better": False, "reps": a.reps, "host_reps": a.host_reps, "warmup": a.warmup, "rows": rows,
           "note": "stage_ms from the build's phase log (every phase synchronised); one-shot and host routes are whole calls, host wall time"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
