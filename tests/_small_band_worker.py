"""Child process of tests/test_gpu_small_band.py: solves the band layout's test batches in a fresh process (the environment decides the
layout: the parent sets QPDO_SMALL_BAND) and writes layouts and results to an .npz file.
usage: _small_band_worker.py OUT.npz SCALING GROUP[,GROUP...]   (GROUP: letters of the shapes, e.g. ABCDE)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from qpdo_amd import solver  # noqa: E402
from test_gpu_small_band import INFO_FIELDS, shapes  # noqa: E402


def main():
    out, scaling, groups = sys.argv[1], int(sys.argv[2]), sys.argv[3].split(",")
    S = shapes()
    rec = {}
    for g in groups:
        res, failed = solver.solve_batch([S[k] for k in g], max_iter=1000, verbose=0, scaling=scaling)
        rec["%s_layout" % g] = np.array([solver.batch_factor_layout(), failed])
        for k, r in zip(g, res):
            rec["%s_%s_x" % (g, k)], rec["%s_%s_y" % (g, k)] = r["x"], r["y"]
            rec["%s_%s_info" % (g, k)] = np.array([float(r["info"][f]) for f in INFO_FIELDS])
    np.savez(out, **rec)


if __name__ == "__main__":
    main()
