"""Wall times of qpdo_amd_tangent (solver.QPDO.tangent) beside qpdo_amd_adjoint and beside the warm-started re-solve it replaces, on the
same workspace, in one process:

    python tools/workspace_tangent_latency.py [--out profiles/workspace_tangent_latency.txt] [--configs C1,mid,C2]

The configurations and the set-up are those of tools/workspace_adjoint_latency.py (C1: n = 200; mid: n = 1000, m = 2000; C2: n = 1e4,
m = 2e4; QPDO_LINSOLVE=dense).  Every call ends in a stream synchronise, so the host clock around it is the call's time.  Per
configuration: 3 untimed calls, then the median and min .. max of 12, for
  the tangent with tq only and with all five arrays, at nrhs = 1 and nrhs = 8;
  the adjoint at nrhs = 1 (gx = the same vector) -- timed ALTERNATING with the tq-only tangent, call by call, so that both see the same
  machine;
  update_q(q + tq) -> warm start from the solution -> qpdo_solve: the re-solve that x + dx stands in for.
Condition 1 (exit status 1 on a miss): the tq-only tangent at nrhs = 1 takes no longer than 1.25 times the adjoint at nrhs = 1 --
max(tangent) <= 1.25 min(adjoint).  Both run the same factorization and the same sweeps on one driver and differ by a few small launches;
the margin covers those and the run-to-run spread.  If their sweep counts differ, both are printed and the times are compared per sweep.
Reported without a threshold: tangent / warm re-solve, all five arrays / tq alone."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qpdo_amd import problems, solver  # noqa: E402

WARM, REPS = 3, 12


def timed(*calls):
    """the calls alternate, one after the other per repetition; per call (median, min, max)"""
    for _ in range(WARM):
        for c in calls:
            c()
    t = [[] for _ in calls]
    for _ in range(REPS):
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            c()
            t[i].append(time.perf_counter() - t0)
    return [(float(np.median(v)), float(min(v)), float(max(v))) for v in t]


def fmt(t):
    return "%9.3f ms  (%.3f .. %.3f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def run(name, p, out):
    os.environ["QPDO_LINSOLVE"] = "dense"
    qp = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p["Qstype"], c=p.get("c", 0.0), verbose=0, max_iter=2000)
    try:
        r = qp.solve()
        assert r["info"]["status_val"] == 1, r["info"]
        n, m = p["n"], p["m"]
        rng = np.random.default_rng(1)
        Q = sp.csc_matrix(p["Q"]); Q.sort_indices()
        tQ = rng.standard_normal((8, Q.nnz))
        if p["Qstype"] == 0:                 # (a full-storage perturbation is passed symmetric)
            for s in range(8):
                T = sp.csc_matrix((tQ[s], Q.indices, Q.indptr), shape=Q.shape)
                T = ((T + T.T) / 2).tocsc(); T.sort_indices()
                tQ[s] = T.data
        t8 = dict(tq=rng.standard_normal((8, n)), tl=rng.standard_normal((8, m)), tu=rng.standard_normal((8, m)), tQ_values=tQ,
                  tA_values=rng.standard_normal((8, sp.csc_matrix(p["A"]).nnz)))
        t1 = {k: v[0] for k, v in t8.items()}
        first = {"q1": qp.tangent(tq=t1["tq"]), "q8": qp.tangent(tq=t8["tq"]), "a1": qp.tangent(**t1), "a8": qp.tangent(**t8), "adj": qp.adjoint(t1["tq"])}
        assert all((v["status"][..., 0] == 0).all() for k, v in first.items() if k in ("q1", "q8", "adj")), {k: v["status"].tolist() for k, v in first.items()}
        tan_q1, adj1 = timed(lambda: qp.tangent(tq=t1["tq"]), lambda: qp.adjoint(t1["tq"]))
        (tan_q8,) = timed(lambda: qp.tangent(tq=t8["tq"]))
        (tan_a1,) = timed(lambda: qp.tangent(**t1))
        (tan_a8,) = timed(lambda: qp.tangent(**t8))
        x0, y0, q1 = r["x"].copy(), r["y"].copy(), p["q"] + t1["tq"]

        def resolve():
            qp.update_q(q1)
            qp.warm_start(x0, y0)
            res = qp.solve()
            assert res["info"]["status_val"] == 1
            return res
        passes = resolve()["info"]["iterations"]
        (t_re,) = timed(resolve)
        s_tan, s_adj = int(first["q1"]["status"][1]), int(first["adj"]["status"][1])
        if s_tan == s_adj:
            ok = tan_q1[2] <= 1.25 * adj1[1]
            cond = "max(tangent) / min(adjoint) = %.3f <= 1.25: %s" % (tan_q1[2] / adj1[1], "PASS" if ok else "FAIL")
        else:
            ok = tan_q1[2] / max(s_tan, 1) <= 1.25 * adj1[1] / max(s_adj, 1)
            cond = "sweeps differ (tangent %d, adjoint %d); per sweep, max(tangent) / min(adjoint) = %.3f <= 1.25: %s" % (
                s_tan, s_adj, (tan_q1[2] / max(s_tan, 1)) / (adj1[1] / max(s_adj, 1)), "PASS" if ok else "FAIL")
        lines = ["%s: n = %d, m = %d, k = %d" % (name, n, m, first["q1"]["status"][2]),
                 "  tangent tq only,  nrhs = 1   %s   sweeps %d" % (fmt(tan_q1), s_tan),
                 "  adjoint           nrhs = 1   %s   sweeps %d   (alternating with the line above)" % (fmt(adj1), s_adj),
                 "  tangent tq only,  nrhs = 8   %s   sweeps %s" % (fmt(tan_q8), first["q8"]["status"][:, 1].tolist()),
                 "  tangent all five, nrhs = 1   %s   sweeps %d, code %d" % (fmt(tan_a1), first["a1"]["status"][1], first["a1"]["status"][0]),
                 "  tangent all five, nrhs = 8   %s   sweeps %s, codes %s" % (fmt(tan_a8), first["a8"]["status"][:, 1].tolist(), first["a8"]["status"][:, 0].tolist()),
                 "  update_q, warm start, solve  %s   %d passes" % (fmt(t_re), passes),
                 "  condition 1: " + cond,
                 "  tangent(tq, nrhs 1) / warm re-solve = %.3f;  all five / tq alone = %.2f (nrhs 1), %.2f (nrhs 8);  nrhs 8 / nrhs 1 = %.2f (tq), %.2f (all five)"
                 % (tan_q1[0] / t_re[0], tan_a1[0] / tan_q1[0], tan_a8[0] / tan_q8[0], tan_q8[0] / tan_q1[0], tan_a8[0] / tan_a1[0])]
        for ln in lines:
            print(ln, flush=True)
            out.write(ln + "\n")
        out.flush()
        return ok
    finally:
        qp.delete()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "workspace_tangent_latency.txt"))
    ap.add_argument("--configs", default="C1,mid,C2")
    a = ap.parse_args()
    make = {"C1": lambda: problems.config_qp("C1"), "mid": lambda: problems.random_qp(77, 1000, 2000, 0.02), "C2": lambda: problems.config_qp("C2")}
    with open(a.out, "w") as out:
        out.write("qpdo_amd_tangent beside qpdo_amd_adjoint and the warm re-solve, wall times on one workspace in one process: %d untimed calls, then median (min .. max) of %d\n" % (WARM, REPS))
        ok = [run(name, make[name](), out) for name in a.configs.split(",")]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
