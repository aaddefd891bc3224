#!/usr/bin/env python3
"""Record what every case of tests/point_record_cases.py gives, as raw words and digests:

    GICP_LIB_VARIANT=<build> python scripts/make_point_record_golden.py OUT.npz

tests/golden/point_record/point_record_parent.npz is this script's output with the library built from the commit
before the clouds' positions and covariances became 48-byte point records (make VARIANT=parent in a checkout of that
commit), on an MI355X.  tests/test_gpu_point_record.py holds every later build to those bits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "generalized-icp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import gicp  # noqa: E402
import point_record_cases as K  # noqa: E402


def main(out):
    eng = gicp.Engine(0)
    try:
        rec = K.record_all(gicp, eng)
    finally:
        eng.close()
    np.savez_compressed(out, **rec)
    print(f"{gicp._lib.LIB_PATH} ({gicp._lib.build_info()}): {len(rec)} entries -> {out}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
