#!/usr/bin/env python3
"""Record the statistics of every case of tests/stats_epilogue_cases.py as raw 64-bit words:

    GICP_LIB_VARIANT=<build> python scripts/make_stats_epilogue_golden.py OUT.npz

tests/golden/stats_epilogue/stats_epilogue_parent.npz is this script's output with the library built from the commit
before the statistics epilogue changed (make VARIANT=parent in a checkout of that commit), on an MI355X.
tests/test_gpu_stats_epilogue.py holds every later build to those bits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generalized-icp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import gicp  # noqa: E402
import stats_epilogue_cases as K  # noqa: E402


def main(out):
    eng = gicp.Engine(0)
    rec = {}
    try:
        for key, src, tgt, T, d_c, d_n, model in K.all_cases():
            st, dbg, info = K.engine_pass(gicp, eng, src, tgt, T, d_c, d_n, model)
            rec[key] = np.ascontiguousarray(st).view(np.uint64).copy()
            print(f"{key}: accepted {int(np.sum(dbg['index'] >= 0))} of {len(src)}, walked tiles "
                  f"{info['walked_tiles']:.0f}, count {st[-1]:.0f}")
    finally:
        eng.close()
    assert list(rec) == K.case_keys()
    np.savez_compressed(out, **rec)
    print(f"{gicp._lib.LIB_PATH} ({gicp._lib.build_info()}): {len(rec)} cases -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
