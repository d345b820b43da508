"""Generates tests/golden/lift_geom_bits.npz: the raw outputs of mp_lift_fuse, mp_lift_fuse_place, mp_lift_fuse_path, mp_lift_align_views,
mp_lift_bundle_views and mp_lift_score on the scenes of tests/test_gpu_lift_geom_bits.py (its record_*() functions: the recording and the test
run the same code).  Outputs only; the inputs are regenerated from their seeds.  Needs an MI355X.

    MANIPOSE_HIP_LIB=<library built at the commit to record> python tools/gen_golden_lift_geom_bits.py [out.npz]

The committed file was run against 93e0414 ("Bundle-adjust a take's estimated cameras: mp_lift_bundle_views"), the last commit at which every
lifting kernel file carried its own rotation, camera model and solves; it is not to be re-recorded to make a changed kernel pass."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "hpe"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_lift_geom_bits as bits  # noqa: E402


def main():
    from manipose_amd import _lib
    path = sys.argv[1] if len(sys.argv) > 1 else bits.GOLD
    out = {}
    for record in bits.RECORDERS:
        got = record()
        assert not set(got) & set(out)
        out.update(got)
        print(f"{record.__name__}: {len(got)} arrays, {sum(a.nbytes for a in got.values())} bytes")
    np.savez_compressed(path, **out)
    print("lift_geom_bits: ok", _lib.LIB_PATH, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
