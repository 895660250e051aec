"""Wall times of qpdo_amd_adjoint / qpdo_amd_tangent with their right-hand sides carried through the sweep loop in groups (the default,
G = 8) beside the same calls with the right-hand sides one after the other (a workspace set up with QPDO_AMD_RHS_GROUP=1, which runs the
launch sequence of a build without groups), in one process:

    python tools/workspace_group_latency.py [--out profiles/workspace_group_latency.txt] [--configs C1,mid,C2,band]

Configurations: C1 (n = 200), mid (n = 1000, m = 2000) and C2 (n = 1e4, m = 2e4) under QPDO_LINSOLVE=dense, and problems.banded_qp(1,
20000) on the band solver.  Per configuration TWO workspaces on the one problem, one default and one with QPDO_AMD_RHS_GROUP=1.  Every call
ends in a stream synchronise, so the host clock around it is the call's time.  Per line: 3 untimed calls, then the median and min .. max
of 12, the two workspaces ALTERNATING call by call, so that both see the same machine: the adjoint (gx, gy) and the tq-only tangent at nrhs = 8, at nrhs = 64 and at nrhs = 1.  groups_run,
rounds_total (QPDOAmdGroupStats: the read-backs of the sweep loop) and the sweep counts of one call are printed beside the times.
Condition 1 (exit status 1 on a miss): for every configuration and both calls the median of the default workspace's nrhs = 8 call is
below the median of the QPDO_AMD_RHS_GROUP=1 workspace's nrhs = 8 call of the same alternating run.  No margin.
Reported without a threshold: nrhs 8 / nrhs 1 and nrhs 64 / nrhs 8 on both workspaces; at C1, jacobian(wrt=("q",)) in both modes."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qpdo_amd import problems, solver  # noqa: E402

WARM, REPS = 3, 12
SWITCHES = ("QPDO_AMD_RHS_GROUP",)


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


def setup(p, linsolve, **env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ["QPDO_LINSOLVE"] = linsolve
    os.environ.update(env)
    qp = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p["Qstype"], c=p.get("c", 0.0), verbose=0, max_iter=2000)
    for k in SWITCHES:
        os.environ.pop(k, None)
    r = qp.solve()
    assert r["info"]["status_val"] == 1, r["info"]
    return qp


def counted(qp, call):
    """one call: (its result, groups_run and rounds_total it added)"""
    s0 = qp.group_stats()
    o = call()
    s1 = qp.group_stats()
    return o, s1["groups_run"] - s0["groups_run"], s1["rounds_total"] - s0["rounds_total"]


def sweeps_of(o):
    sw = np.atleast_2d(o["status"])[:, 1]
    return "%d" % sw[0] if len(sw) == 1 else "%d .. %d" % (sw.min(), sw.max())


def run(name, p, linsolve, out):
    n, m = p["n"], p["m"]
    ws = [("default", setup(p, linsolve)), ("RHS_GROUP=1", setup(p, linsolve, QPDO_AMD_RHS_GROUP="1"))]
    ok = True
    lines = []
    try:
        rng = np.random.default_rng(1)
        gx, gy, tq = rng.standard_normal((64, n)), rng.standard_normal((64, m)), rng.standard_normal((64, n))
        lines.append("%s: n = %d, m = %d, group sizes %s" % (name, n, m, ", ".join("%s: %d" % (w, q.rhs_group()) for w, q in ws)))
        med = {}
        for R in (8, 64, 1):
            for kind in ("adjoint", "tangent"):
                def call_on(q):
                    if kind == "adjoint":
                        return (lambda: q.adjoint(gx[0], gy[0])) if R == 1 else (lambda: q.adjoint(gx[:R], gy[:R]))
                    return (lambda: q.tangent(tq=tq[0])) if R == 1 else (lambda: q.tangent(tq=tq[:R]))
                use = ws
                info = [counted(q, call_on(q)) for _, q in use]
                assert all((np.atleast_2d(o["status"])[:, 0] != 3).all() for o, _, _ in info), (name, kind, R)
                times = timed(*[call_on(q) for _, q in use])
                for (w, _), t, (o, g, rd) in zip(use, times, info):
                    med[(kind, R, w)] = t[0]
                    lines.append("  %-8s nrhs = %-2d  %-20s %s   groups %d, read-backs %d, sweeps %s, accepted %d"
                                 % (kind, R, w, fmt(t), g, rd, sweeps_of(o), int((np.atleast_2d(o["status"])[:, 0] == 0).sum())))
        for kind in ("adjoint", "tangent"):
            a, b = med[(kind, 8, "default")], med[(kind, 8, "RHS_GROUP=1")]
            hit = a < b
            ok = ok and hit
            lines.append("  condition 1, %s: median(default, nrhs 8) / median(RHS_GROUP=1, nrhs 8) = %.3f < 1: %s" % (kind, a / b, "PASS" if hit else "FAIL"))
            lines.append("  %s: nrhs 8 / nrhs 1 = %.2f (default), %.2f (RHS_GROUP=1);  nrhs 64 / nrhs 8 = %.2f (default), %.2f (RHS_GROUP=1)"
                         % (kind, a / med[(kind, 1, "default")], b / med[(kind, 1, "RHS_GROUP=1")], med[(kind, 64, "default")] / a, med[(kind, 64, "RHS_GROUP=1")] / b))
        if name == "C1":
            q = ws[0][1]
            jt, ja = timed(lambda: q.jacobian(wrt=("q",), mode="tangent"), lambda: q.jacobian(wrt=("q",), mode="adjoint"))
            lines.append("  jacobian(wrt=(q,)), %d right-hand sides:  tangent mode %s   adjoint mode %s" % (n, fmt(jt), fmt(ja)))
    finally:
        for _, q in ws:
            q.delete()
    for ln in lines:
        print(ln, flush=True)
        out.write(ln + "\n")
    out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "workspace_group_latency.txt"))
    ap.add_argument("--configs", default="C1,mid,C2,band")
    a = ap.parse_args()
    make = {"C1": (lambda: problems.config_qp("C1"), "dense"), "mid": (lambda: problems.random_qp(77, 1000, 2000, 0.02), "dense"),
            "C2": (lambda: problems.config_qp("C2"), "dense"), "band": (lambda: problems.banded_qp(1, 20000), "band")}
    with open(a.out, "w") as out:
        out.write("qpdo_amd_adjoint / qpdo_amd_tangent in groups of 8 right-hand sides beside one after the other, wall times in one process: "
                  "%d untimed calls, then median (min .. max) of %d, the workspaces alternating call by call\n" % (WARM, REPS))
        ok = [run(name, make[name][0](), make[name][1], out) for name in a.configs.split(",")]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
