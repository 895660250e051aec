"""Wall times of qpdo_amd_adjoint (solver.QPDO.adjoint) beside qpdo_solve on the same workspace, in one process:

    python tools/workspace_adjoint_latency.py [--out profiles/workspace_adjoint_latency.txt] [--configs C1,mid,C2]

C1: problems.config_qp('C1') (n = 200); mid: random_qp(n = 1000, m = 2000, density 0.02); C2: config_qp('C2') (n = 1e4, m = 2e4).  Every
workspace is set up with QPDO_LINSOLVE=dense (the automatic choice at these sizes; set explicitly so that C2 does not start its solves with
PCG and the factor under test is the one qpdo_amd_bench_dense_factor times).  Per configuration: 3 untimed calls, then the median and
min .. max of 12, for qpdo_solve (cold start), adjoint at nrhs = 1 and at nrhs = 8; the sweeps; the HIP-event time of one dense
factorization on the same workspace.  Two conditions are checked and printed:
  1. nrhs = 8 costs less than 8 times nrhs = 1 (one factorization per call), with the nrhs = 1 call's own min .. max spread as the
     margin: PASS when median(8) < 8 min(1), WITHIN SPREAD when it holds only against 8 max(1), FAIL otherwise (exit status 1).
  2. adjoint(nrhs = 1) / qpdo_solve: the cost of the whole gradient against ONE finite-difference component.  Reported; no threshold."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qpdo_amd import problems, solver  # noqa: E402

WARM, REPS = 3, 12


def timed(call):
    for _ in range(WARM):
        call()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def fmt(t):
    return "%9.3f ms  (%.3f .. %.3f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def run(name, p, out):
    os.environ["QPDO_LINSOLVE"] = "dense"
    qp = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p["Qstype"], c=p.get("c", 0.0), verbose=0, max_iter=2000)
    try:
        r = qp.solve()
        assert r["info"]["status_val"] == 1, r["info"]
        rng = np.random.default_rng(1)
        g1, g8 = rng.standard_normal(p["n"]), rng.standard_normal((8, p["n"]))
        t_solve = timed(qp.solve)
        a1 = qp.adjoint(g1)
        a8 = qp.adjoint(g8)
        assert a1["status"][0] == 0 and (a8["status"][:, 0] == 0).all(), (a1["status"], a8["status"])
        t1 = timed(lambda: qp.adjoint(g1))
        t8 = timed(lambda: qp.adjoint(g8))
        tf, _ = qp.bench_dense_factor(reps=5, check=False)
        verdict = "PASS" if t8[0] < 8 * t1[1] else "WITHIN SPREAD" if t8[0] < 8 * t1[2] else "FAIL"
        lines = ["%s: n = %d, m = %d, %d passes, k = %d" % (name, p["n"], p["m"], r["info"]["iterations"], a1["status"][2]),
                 "  qpdo_solve (cold)        %s" % fmt(t_solve),
                 "  adjoint nrhs = 1         %s   sweeps %d" % (fmt(t1), a1["status"][1]),
                 "  adjoint nrhs = 8         %s   sweeps %s" % (fmt(t8), a8["status"][:, 1].tolist()),
                 "  one dense factorization  %9.3f ms  (HIP events)" % (1e3 * tf),
                 "  condition 1: median(nrhs 8) / median(nrhs 1) = %.2f < 8: %s" % (t8[0] / t1[0], verdict),
                 "  condition 2: adjoint(nrhs 1) / qpdo_solve = %.3f  (the whole gradient against one finite-difference component)" % (t1[0] / t_solve[0])]
        for ln in lines:
            print(ln, flush=True)
            out.write(ln + "\n")
        out.flush()
        return verdict != "FAIL"
    finally:
        qp.delete()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "workspace_adjoint_latency.txt"))
    ap.add_argument("--configs", default="C1,mid,C2")
    a = ap.parse_args()
    make = {"C1": lambda: problems.config_qp("C1"), "mid": lambda: problems.random_qp(77, 1000, 2000, 0.02), "C2": lambda: problems.config_qp("C2")}
    with open(a.out, "w") as out:
        out.write("qpdo_amd_adjoint beside qpdo_solve, wall times on one workspace in one process: %d untimed calls, then median (min .. max) of %d\n" % (WARM, REPS))
        ok = [run(name, make[name](), out) for name in a.configs.split(",")]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
