"""Measurements of the input filters for profiles/filter/README.md, one MI355X.

    python scripts/measure_filter.py [--out profiles/filter/measure.json]

1. Stage times of a fused source build at 8k (room), 100k (a 64 x 1563 LiDAR frame) and 1M (room) points, 3-D:
   GICP_VERBOSE=1 makes the build print the stream-synchronised wall time of every stage (upload, filter, voxel,
   ...), so a stage's figure is its launches plus its one synchronisation and no host copy.  Three settings per
   cloud -- crop alone, crop + radius outlier removal, and (beside both) the voxel filter on the crop's output, which
   is the whole cloud: the crop's max_range keeps every row.  A child process per setting; medians over the repeats
   after the warm-up, with the smallest and largest.
2. The one-shot gicp.filter_points host to host (copies included), same clouds.
3. A 100k frame pair with 12 max-range returns appended to each: build time, pass-0 time and pairs screened without
   a filter, with Odometry's max_range, and for the clean pair."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generalized-icp_amd"))
import numpy as np  # noqa: E402

P3 = dict(max_distance_correspondence=0.5, max_distance_nearest_neighbors=1.0)
WARM, REPS = 3, 15
RADIUS = {"8k": 1.0, "100k": 0.5, "1M": 0.25}
SETTINGS = {"crop": dict(max_range=1e9), "crop_ror": dict(max_range=1e9, min_neighbors=3), "none": None}
LEAF = 0.25


def cloud(name):
    from gicp import synthetic as S
    if name == "100k":
        return np.ascontiguousarray(next(iter(S.lidar_stream(1, beams=64, azimuths=1563)))[0])
    return S.scene_pair_3d(8000 if name == "8k" else 1000000)[0]


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def child(name, setting):
    import gicp
    pts = cloud(name)
    p = gicp.default_params(3, **P3)
    e = gicp.Engine(0)
    kw = SETTINGS[setting]
    if kw is not None:
        e.set_filter(radius=RADIUS[name] if "min_neighbors" in kw else 0.0, **kw)
    e.set_voxel(LEAF)
    for _ in range(WARM + REPS):
        e.set_source(pts, p)
    print("ROWS", len(pts), e.cloud_size("source"), flush=True)
    if kw is not None:      # the one-shot, host to host
        f = dict(e.filter)
        t = []
        for _ in range(WARM + REPS):
            t0 = time.perf_counter()
            out = e.filter_points(pts, **f)
            t.append((time.perf_counter() - t0) * 1e3)
        print("ONESHOT", json.dumps(spread(t[WARM:])), len(out), flush=True)
    e.close()


def stages(name, setting):
    env = dict(os.environ, GICP_VERBOSE="1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, setting], env=env, capture_output=True,
                         text=True, timeout=600)
    if run.returncode != 0:
        raise RuntimeError(run.stderr[-2000:])
    rows = []
    for line in run.stderr.splitlines():
        m = re.search(r"\| ms:(.*)$", line)
        if m:
            tok = m.group(1).split()
            rows.append({tok[i]: float(tok[i + 1]) for i in range(0, len(tok), 2)})
    rows = rows[WARM:]
    out = {k: spread([r[k] for r in rows]) for k in rows[0]}
    for line in run.stdout.splitlines():
        if line.startswith("ONESHOT"):
            out["one_shot_host_to_host_ms"] = json.loads(line.split(" ", 1)[1].rsplit(" ", 1)[0])
        if line.startswith("ROWS"):
            out["rows_in"], out["rows_indexed"] = int(line.split()[1]), int(line.split()[2])
    return out


def stretched_frame():
    import gicp
    from gicp import synthetic as S
    clean = [np.ascontiguousarray(f) for f, _ in S.lidar_stream(2, beams=64, azimuths=1563)]
    rng = np.random.default_rng(23)
    raw = []
    for f in clean:
        d = rng.normal(size=(12, 3))
        raw.append(np.concatenate([f, 1e5 * d / np.linalg.norm(d, axis=1, keepdims=True)]))
    p = gicp.default_params(3, **P3)
    out = {}
    for what, (a, b), filt in (("raw_no_filter", raw, {}), ("raw_max_range_100", raw, dict(max_range=100.0)),
                               ("clean", clean, {})):
        build, pass0, pairs = [], [], []
        for _ in range(WARM + 7):
            e = gicp.Engine(0)
            e.set_filter(**filt)
            t0 = time.perf_counter()
            e.set_target(b, p)
            e.set_source(a, p)
            t1 = time.perf_counter()
            e.iterate(np.eye(4))
            t2 = time.perf_counter()
            build.append((t1 - t0) * 1e3)
            pass0.append((t2 - t1) * 1e3)
            pairs.append(e.pass_info()["pairs"])
            e.close()
        assert len(set(pairs)) == 1
        out[what] = dict(build_ms=spread(build[WARM:]), pass0_ms=spread(pass0[WARM:]), pairs_screened=pairs[0], rows=len(a))
    assert out["raw_max_range_100"]["pairs_screened"] == out["clean"]["pairs_screened"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    res = {"leaf": LEAF, "radius": RADIUS, "stages_ms": {}}
    for name in ("8k", "100k", "1M"):
        res["stages_ms"][name] = {s: stages(name, s) for s in SETTINGS}
    res["stretched_100k_frame"] = stretched_frame()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
