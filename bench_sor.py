"""Statistical outlier removal: the stage fused into a cloud build, beside the two routes a caller had
before it -- scipy's cKDTree with 16 workers plus NumPy, and Engine.knn(k + 1) on the resident cloud plus NumPy.

    python bench_sor.py [--sizes 8000,100000,1000000] [--ks 8,15,20] [--reps 15] [--warmup 2] [--out profiles/sor/bench.json]

Per size and k:
  stage_ms     the stream-synchronised time of the stage inside Engine.set_target, from the build's own phase log
               (GICP_VERBOSE=1: every phase ends with a stream synchronisation): sor-index (the index-only build of the
               stage's rows), sor-query (the self-query for k + 1 rows), sor-reduce (means, two tree sums, flags,
               compaction, the result words); median of --reps builds after --warmup, std_ratio 1
  build_ms     the whole verbose build with the stage, and without it (the other phases are synchronised too, so both
               are slower than a plain build: they are there for the share, not as a frame time)
  ckdtree_ms   cKDTree(points).query(points, k + 1, workers=16) plus the NumPy statistics, the tree built inside the
               timed region (a caller filters every frame once); median of --host-reps
  knn_ms       Engine.knn(None, k + 1) on the resident cloud (kernel + the copy of its answers) plus the same NumPy
The number of rows each route keeps is recorded beside the relative distance of the nearest mean to the threshold (the
host routes sum in NumPy's order, so equal counts are expected only where no mean lies within rounding of it); nothing
is asserted.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "generalized-icp_amd"), ROOT]
os.environ["GICP_VERBOSE"] = "1"

import numpy as np  # noqa: E402


def numpy_sor(d2, std_ratio):
    """What a caller writes today: mean of the k roots, mean and sample deviation over the cloud."""
    mean = np.sqrt(d2[:, 1:]).mean(axis=1)
    thr = mean.mean() + std_ratio * mean.std(ddof=1)
    return mean <= thr, mean, thr


def logged_build(eng, pts, p):
    """Engine.set_target with the build's phase log (stderr of the library) captured: (wall ms, {phase: ms})."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tf:
        old = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            t0 = time.perf_counter()
            eng.set_target(pts, p)
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(old, 2)
            os.close(old)
        tf.seek(0)
        text = tf.read().decode()
    m = re.search(r"\| ms:(.*)$", text, re.M)
    tok = m.group(1).split()
    return wall, {tok[i]: float(tok[i + 1]) for i in range(0, len(tok), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8000,100000,1000000")
    ap.add_argument("--ks", default="8,15,20")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sor", "bench.json"))
    a = ap.parse_args()
    from scipy.spatial import cKDTree

    import gicp
    from gicp import synthetic as S

    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
    med = statistics.median
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        _, tgt, _ = S.scene_pair_3d(n)
        tgt = np.ascontiguousarray(tgt)
        eng = gicp.Engine(0)
        try:
            plain = [logged_build(eng, tgt, p)[0] for _ in range(a.warmup + a.reps)][a.warmup:]
            for k in [int(v) for v in a.ks.split(",")]:
                eng.set_sor(k, 1.0)
                runs = [logged_build(eng, tgt, p) for _ in range(a.warmup + a.reps)][a.warmup:]
                kept_dev = eng.cloud_size("target")
                eng.set_sor(None)
                phase = {ph: med([r[1][ph] for r in runs]) for ph in ("sor-index", "sor-query", "sor-reduce")}
                stage = med([sum(r[1][ph] for ph in phase) for r in runs])
                eng.set_target(tgt, p)      # the resident cloud of the knn route: the unfiltered rows

                def ckd():
                    d, _ = cKDTree(tgt).query(tgt, k=k + 1, workers=a.workers)
                    return numpy_sor(d * d, 1.0)

                def knn():
                    _, d2 = eng.knn(None, k=k + 1, squared=True)
                    return numpy_sor(d2, 1.0)

                host = {}
                for name, fn in (("ckdtree", ckd), ("knn", knn)):
                    fn()
                    walls = []
                    for _ in range(a.host_reps):
                        t0 = time.perf_counter()
                        keep, mean, thr = fn()
                        walls.append((time.perf_counter() - t0) * 1e3)
                    host[name] = (med(walls), int(keep.sum()), float(np.abs(mean - thr).min() / thr))
                rows.append({"rows": n, "k": k, "knn_instantiation": 8 if k + 1 <= 8 else 16 if k + 1 <= 16 else 32,
                             "stage_ms": round(stage, 3), "phases_ms": {ph: round(v, 3) for ph, v in phase.items()},
                             "self_query_share": round(phase["sor-query"] / stage, 3),
                             "build_ms_with_stage": round(med([r[0] for r in runs]), 3),
                             "build_ms_without": round(med(plain), 3), "kept": int(kept_dev),
                             "ckdtree_ms": round(host["ckdtree"][0], 3), "ckdtree_workers": a.workers,
                             "knn_plus_numpy_ms": round(host["knn"][0], 3),
                             "kept_ckdtree": host["ckdtree"][1], "kept_knn": host["knn"][1],
                             "nearest_mean_to_threshold_rel": host["knn"][2],
                             "stage_over_ckdtree": round(host["ckdtree"][0] / stage, 2),
                             "stage_over_knn": round(host["knn"][0] / stage, 2)})
        finally:
            eng.close()
    res = {"metric": "statistical outlier removal: stream-synchronised stage time of a fused build", "unit": "ms",
           "higher_is_better": False, "reps": a.reps, "host_reps": a.host_reps, "warmup": a.warmup, "rows": rows,
           "note": "stage_ms from the build's phase log (every phase synchronised); host routes are whole calls, host wall time"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
