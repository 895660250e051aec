#!/usr/bin/env python3
"""Closed-loop re-solve of a fleet of MPC-sized QPs: what does a control step cost through a resident Fleet (update + warm_start_last +
solve: three launches, only q, l, u go up) against the path that existed before it -- qpdo_amd_solve_batch on the updated data with
x0 / y0 = the previous solution, which converts, packs, uploads and scales every matrix again?

    python tools/fleet_resolve_latency.py [--count 4096] [--steps 8] [--repeats 3] [--max-iter 300] [--out profiles/fleet_resolve_latency.txt]

Every step perturbs q and the inequality bounds deterministically from the previous step's.  Both paths see the same data and must end
every step with the same statuses (checked).  Printed: median step time (wall clock around the C calls only), kernel time (HIP events of
the solve launch) and uploaded bytes per step, for each of `repeats` runs of the whole loop; the claim to check is "a fleet step is not
slower than a batch step", the margin being the spread of the batch step over the repeats.  Step 0 (the cold solve) is not counted."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402


def perturbed(k, q0, l0, u0):
    """data of step k from the setup's: a slowly rotating q, inequality rows breathing by a few percent (equality rows stay equalities)"""
    ph = 0.37 * k
    q = [q * (1.0 + 0.05 * np.sin(ph + 0.1 * np.arange(len(q)))) for q in q0]
    w = 0.02 * (1.0 + np.sin(ph))
    l = [np.where(l < u, l - w, l) for l, u in zip(l0, u0)]
    u = [np.where(l < u, u + w, u) for l, u in zip(l0, u0)]
    return q, l, u


def round256(b):
    return (b + 255) & ~255


def run_loop(probs, steps, st, first=0):
    N = len(probs)
    q0 = [np.array(p["q"], float) for p in probs]
    l0 = [np.clip(p["l"], -1e20, 1e20) for p in probs]
    u0 = [np.clip(p["u"], -1e20, 1e20) for p in probs]
    settings = solver.default_settings(**st)
    F = solver.Fleet(probs, settings=settings)
    B = solver.Batch(probs)
    bq = [np.ctypeslib.as_array(B.items[i].data.contents.q, shape=(p["n"],)) for i, p in enumerate(probs)]
    bl = [np.ctypeslib.as_array(B.items[i].data.contents.l, shape=(p["m"],)) for i, p in enumerate(probs)]
    bu = [np.ctypeslib.as_array(B.items[i].data.contents.u, shape=(p["m"],)) for i, p in enumerate(probs)]
    x0 = [np.zeros(p["n"]) for p in probs]
    y0 = [np.zeros(p["m"]) for p in probs]
    matrix_bytes = F.stats()["matrix_bytes_uploaded"]
    rows = []
    F.solve(results=False)
    B.run(settings, results=False)
    assert np.array_equal(F.info_view()["status_val"], B.info_view()["status_val"]), "cold solve: statuses differ"
    for k in range(1, steps + 1):
        q, l, u = perturbed(k, q0, l0, u0)
        # the batch path's inputs (outside the timed region: a caller would own these arrays anyway)
        sb = B.info_view()["status_val"].copy()
        nws = 0
        for i in range(N):
            bq[i][:] = q[i]; bl[i][:] = l[i]; bu[i][:] = u[i]
            if sb[i] in (-3, -4, -10, -99):
                B.items[i].x0, B.items[i].y0 = None, None
            else:
                x0[i][:] = B.outs[i][0]; y0[i][:] = B.outs[i][1]
                B.items[i].x0, B.items[i].y0 = x0[i].ctypes.data_as(solver.dp), y0[i].ctypes.data_as(solver.dp)
                nws += 1
        batch_first = (k + first) % 2 == 1              # the order alternates per step (and starts the other way round every repeat)
        if batch_first:
            tb0 = time.perf_counter()
            B.run(settings, results=False)
            tb1 = time.perf_counter()
        t0 = time.perf_counter()
        F.update(q=q, l=l, u=u)
        t1 = time.perf_counter()
        up = F.stats()["vector_bytes_uploaded_last_call"]
        t2 = time.perf_counter()
        F.warm_start_last()
        t3 = time.perf_counter()
        F.solve(results=False)
        t4 = time.perf_counter()
        if not batch_first:
            tb0 = time.perf_counter()
            B.run(settings, results=False)
            tb1 = time.perf_counter()
        # The two paths are not the same computation: the batch call sets the item up again (cost scaling c from the new q alone), the fleet
        # does what qpdo_update_q does (c from the new q and the current Qx), and a fleet item that runs out of passes keeps its earlier
        # status (qpdo.c:451-453).  So an item that reaches the pass limit on either path may report differently; every other item must agree.
        sf, sb = F.info_view()["status_val"], B.info_view()["status_val"]
        capped = (F.info_view()["iterations"] >= st["max_iter"]) | (B.info_view()["iterations"] >= st["max_iter"])
        differ = (sf != sb)
        assert not (differ & ~capped).any(), "step %d: statuses differ on %d items that did not reach the pass limit" % (k, int((differ & ~capped).sum()))
        # an ESTIMATE of what the batch call uploads: the fleet's one-time image (same layout) + x0, y0 of the warm-started items
        bbytes = matrix_bytes + sum(round256(8 * p["n"]) + round256(8 * p["m"] + 8) for i, p in enumerate(probs) if B.items[i].x0)
        rows.append(dict(fleet=(t1 - t0) + (t3 - t2) + (t4 - t3), f_update=t1 - t0, f_ws=t3 - t2, f_solve=t4 - t3, f_kernel=F.kernel_seconds,
                         f_bytes=up, batch=tb1 - tb0, b_kernel=B.kernel_seconds, b_bytes=bbytes,
                         passes=int(F.info_view()["iterations"].sum()), b_passes=int(B.info_view()["iterations"].sum()),
                         capped=int(capped.sum()), differ=int(differ.sum())))
    F.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="label for the table (default: git rev-parse of this tree)")
    a = ap.parse_args()
    probs = [problems.config_qp("C3", i) for i in range(a.count)]
    st = dict(verbose=0, max_iter=a.max_iter)
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    lines = []
    commit = a.commit
    try:
        if commit is None:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), text=True,
                                             stderr=subprocess.DEVNULL).strip() + " (+ working tree)"
    except Exception:
        commit = "unknown"
    lines.append("closed loop over %d config_qp('C3', i) items, %d steps after the cold solve, max_iter %d; commit %s" % (a.count, a.steps, a.max_iter, commit))
    lines.append("median per step; times in ms; which path runs first alternates per step.  Statuses: equal on every item that stays below the pass limit on")
    lines.append("both paths (asserted); 'capped' = items at the limit on either path, 'differ' = of those, items whose statuses differ (median per step)")
    lines.append("bytes per step: fleet = counted by the library; batch = ESTIMATE from the layout of its upload (the fleet's one-time image + x0, y0), not counted")
    lines.append("%-4s | %9s %9s %9s %9s %9s %12s | %9s %9s %12s | %8s %8s %6s %6s" % ("run", "fleet", "update", "warmstart", "solve", "kernel", "bytes", "batch", "kernel", "est.bytes", "f.passes", "b.passes", "capped", "differ"))
    fm, bm = [], []
    for r in range(a.repeats):
        rows = run_loop(probs, a.steps, st, first=r)
        fm.append(med(rows, "fleet")); bm.append(med(rows, "batch"))
        lines.append("%-4d | %9.3f %9.3f %9.3f %9.3f %9.3f %12d | %9.3f %9.3f %12d | %8d %8d %6d %6d" % (
            r, 1e3 * med(rows, "fleet"), 1e3 * med(rows, "f_update"), 1e3 * med(rows, "f_ws"), 1e3 * med(rows, "f_solve"), 1e3 * med(rows, "f_kernel"),
            int(med(rows, "f_bytes")), 1e3 * med(rows, "batch"), 1e3 * med(rows, "b_kernel"), int(med(rows, "b_bytes")), int(med(rows, "passes")), int(med(rows, "b_passes")),
            int(med(rows, "capped")), int(med(rows, "differ"))))
    spread = max(bm) - min(bm)
    lines.append("batch step: median of runs %.3f ms, run-to-run spread (max - min of %d runs) %.3f ms" % (1e3 * float(np.median(bm)), a.repeats, 1e3 * spread))
    lines.append("fleet step: median of runs %.3f ms, spread %.3f ms" % (1e3 * float(np.median(fm)), 1e3 * (max(fm) - min(fm))))
    verdict = float(np.median(fm)) <= float(np.median(bm)) + spread
    lines.append("claim 'a fleet step is not slower than a batch step (margin: the batch spread)': %s" % ("HOLDS" if verdict else "FAILS"))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
