"""Exact k-nearest-neighbour queries: Engine.knn against resident clouds of the benchmark's
1M / 1M 3-D room, beside scipy's cKDTree on the same arrays with 16 workers.

    python bench_knn.py [--points 1000000] [--reps 5] [--warmup 2] [--out profiles/knn/bench.json]

Rows:
  self_k20_dn   the target against itself, k = 20, max_distance = d_n (the covariance search's neighbourhoods)
  cross_k1/8/32 the source's points against the target, no limit
Whole calls are timed on the host (queries uploaded and indexed where they are external, the launch, the one
synchronisation, the answers copied back): the median of --reps after --warmup, with min and max.  The self-query
has no upload and no index build, so its figure is the kernel and the copy of its answers.  cKDTree is timed the same
way (the tree is built outside the timed region, as the engine's index is).  The indices are compared with cKDTree's
wherever the reference distances show no exact tie.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "generalized-icp_amd"), ROOT]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn", "bench.json"))
    a = ap.parse_args()
    from scipy.spatial import cKDTree

    import gicp
    from gicp import synthetic as S

    src, tgt, _ = S.scene_pair_3d(a.points)
    d_n = 1.0
    p = gicp.default_params(3, max_distance_correspondence=0.5, max_distance_nearest_neighbors=d_n)
    eng = gicp.Engine(0)
    eng.set_target(tgt, p)
    tree = cKDTree(tgt)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        walls, last = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            last = fn()
            walls.append((time.perf_counter() - t0) * 1e3)
        return walls, last

    work = [("self_k20_dn", None, tgt, 20, d_n)] + [(f"cross_k{k}", src, src, k, None) for k in (1, 8, 32)]
    rows = []
    for name, qs, cpu_qs, k, r in work:
        wg, (idx, d2) = timed(lambda: eng.knn(qs, k=k, max_distance=r, squared=True))
        wc, (cd, ci) = timed(lambda: tree.query(cpu_qs, k=k, workers=a.workers,
                                                distance_upper_bound=np.inf if r is None else r))
        ci = np.asarray(ci).reshape(len(cpu_qs), k)
        ci = np.where(ci == len(tgt), -1, ci)
        # rows whose reference distances are strictly increasing hold no exact tie: there both must agree
        fin = np.where(np.isfinite(d2), d2, np.arange(k)[None, :] + 1e300)
        clear = np.all(np.diff(fin, axis=1) > 0, axis=1) if k > 1 else np.ones(len(idx), dtype=bool)
        mg, mc = statistics.median(wg), statistics.median(wc)
        rows.append({"row": name, "queries": int(len(idx)), "database": int(len(tgt)), "k": k, "max_distance": r,
                     "gpu_ms": round(mg, 3), "gpu_ms_min_max": [round(min(wg), 3), round(max(wg), 3)],
                     "gpu_queries_per_s": round(len(idx) / mg * 1e3, 1),
                     "ckdtree_ms": round(mc, 3), "ckdtree_ms_min_max": [round(min(wc), 3), round(max(wc), 3)],
                     "ckdtree_workers": a.workers, "speedup_over_ckdtree": round(mc / mg, 2),
                     "rows_without_ties": int(clear.sum()),
                     "indices_equal_ckdtree_on_them": bool(np.array_equal(idx[clear], ci[clear]))})
    eng.close()
    res = {"metric": "exact kNN against a resident cloud: whole calls, host wall time", "unit": "ms", "higher_is_better": False,
           "points": a.points, "reps": a.reps, "warmup": a.warmup, "rows": rows,
           "note": "median of whole Engine.knn calls (external queries: upload + index build + kernel + copy back; "
                   "self-query: kernel + copy back); cKDTree.query with the tree built beforehand"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
