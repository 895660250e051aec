"""Records tests/golden/slab_trips_n6400.npz: the n6400 problem of tests/test_gpu_inner_refine.py solved on the GPU with the slab kernels
forced, plain and under QPDO_SLAB_MAX_W=1280 -- x, y, the three integers of the info and every counter of stats() -- by the build that
the process loads (QPDO_AMD_LIB names another one).  Taken ONCE, with the build from before the slab kernel's row trips became
branch-free: tests/test_gpu_slab_trips.py expects every later build to reproduce it bit for bit.

    python tests/golden/make_slab_trips_golden.py [output.npz]

Each solve runs twice; the script refuses to write a record that the same build does not repeat."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from qpdo_amd import problems, solver  # noqa: E402

PROBLEM = (0, 6400, 20000, 0.003, 0)                    # test_gpu_inner_refine.PROBLEMS["n6400"]
CAPS = {"plain": None, "max_w_1280": "1280"}
INFO_KEYS = ("status_val", "iterations", "oterations")
# the counters: every integer field of the statistics but the numbers of timing samples, and the two worst-case ratios (doubles that the
# arithmetic alone decides); the remaining doubles are times and byte counts of timed samples
SKIP = ("spmv_Q_samples", "spmv_Ac_samples")
RATIOS = ("pcg_max_relres", "inner_refine_max_res_over_tol")


def counter_keys():
    import ctypes
    return [f for f, t in solver.Stats._fields_ if (t is ctypes.c_long and f not in SKIP) or f in RATIOS]


def solve(cap):
    for k in ("QPDO_PCG_INNER_REFINE", "QPDO_PCG_INNER_F32", "QPDO_INNER_REFINE_MAXSWEEP", "QPDO_INNER_REFINE_THETA", "QPDO_SCHUR_TAU",
              "QPDO_INNER_FOLD", "QPDO_SLAB_NT", "QPDO_IDX16", "QPDO_SLAB_OVERLAP", "QPDO_INNER_H16", "QPDO_INNER_H16_ETA",
              "QPDO_INNER_H16_MAXSWEEP", "QPDO_INNER_X32", "QPDO_SLAB_MAX_W"):
        os.environ.pop(k, None)
    os.environ.update(QPDO_LINSOLVE="pcg", QPDO_PCG_SCHUR="1", QPDO_SPMV="slab")
    if CAPS[cap]:
        os.environ["QPDO_SLAB_MAX_W"] = CAPS[cap]
    r = solver.solve_problem(problems.random_qp(*PROBLEM), verbose=0)
    rec = {"x": r["x"], "y": r["y"]}
    rec.update({k: np.int64(r["info"][k]) for k in INFO_KEYS})
    rec.update({"stats_" + k: np.asarray(r["stats"][k]) for k in counter_keys()})
    return rec


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.atleast_1d(a[k]).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)) for k in a)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "slab_trips_n6400.npz")
    data = {}
    for cap in CAPS:
        a, b = solve(cap), solve(cap)
        if not same(a, b):
            sys.exit("%s: two solves of the same build differ in %s" % (cap, [k for k in a if not np.array_equal(a[k], b[k])]))
        print(cap, {k: int(a[k]) for k in INFO_KEYS}, {k[6:]: a[k].item() for k in a if k.startswith("stats_inner_")})
        data.update({cap + "_" + k: v for k, v in a.items()})
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")
