#!/usr/bin/env python3
"""What does the adjoint of a fleet's solve cost beside the solve itself?  A fleet of C3 items (n = 120, m = 360), both scalings:

  adjoint      HIP-event time of one Fleet.adjoint_device call (k_small_fleet_adjoint, gy = None, no matrix outputs), events on the caller's stream
  adjoint+QA   the same with dQ_values / dA_values written
  re-solve     the same fleet's warm re-solve launch (warm_start_last_device -> solve_device; events around the solve call, scatter included)
  pass         the cold solve's last_kernel_seconds over the largest `iterations` of the launch: one Newton pass of the slowest item

    python tools/fleet_adjoint_latency.py [--count 4096] [--reps 20] [--warmup 5] [--max-iter 300] [--out profiles/fleet_adjoint_latency.txt]

Median of `reps` after `warmup` untimed calls.  The expectation from the operation count is one to two passes' worth (one assembly, one
factorization, 1 + sweeps solves with a few small products each); the table states the ratio, nothing is asserted.  No GPU: the tool fails."""
import argparse
import os
import sys

import numpy as np
import torch  # (before qpdo_amd loads its library: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402


def timed(fn, reps, warmup):
    """median, min, max in seconds of fn() between two events on the current stream"""
    ts = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), min(ts), max(ts)


def measure(count, scaling, reps, warmup, max_iter):
    probs = [problems.config_qp("C3", i) for i in range(count)]
    F = solver.Fleet(probs, matrix_updates=True, adjoint=True, verbose=0, max_iter=max_iter, scaling=scaling)
    try:
        no, mo = F.packed_layout()
        gx = torch.from_numpy(np.random.default_rng(1).standard_normal(int(no[-1]))).cuda()
        cold = F.solve()
        iters = max(r["info"]["iterations"] for r in cold)
        solved = sum(r["info"]["status_val"] == 1 for r in cold)
        one_pass = F.stats()["last_kernel_seconds"] / iters
        adj = timed(lambda: F.adjoint_device(gx), reps, warmup)
        st = F.adjoint_device(gx)["status"].cpu().numpy()
        adjm = timed(lambda: F.adjoint_device(gx, matrices=True), reps, warmup)
        ok = st[:, 0] == 0
        ran = st[:, 0] < 2                                   # every item that swept: accepted or not

        def resolve():
            F.solve_device()
        # (the warm start belongs to the step, not to the window: it is enqueued before the first event)
        ts = []
        for k in range(warmup + reps):
            F.warm_start_last_device()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); resolve(); e1.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ts.append(e0.elapsed_time(e1) * 1e-3)
        return dict(scaling=scaling, count=count, solved=int(solved), accepted=int(ok.sum()), iters=int(iters), one_pass=one_pass, adj=adj, adjm=adjm,
                    resolve=(float(np.median(ts)), min(ts), max(ts)), sweeps_max=int(st[ran, 1].max()) if ran.any() else -1,
                    sweeps_mean=float(st[ran, 1].mean()) if ran.any() else float("nan"), sweeps_mean_all=float(st[:, 1].mean()),
                    not_accepted=int((st[:, 0] == 1).sum()), bad_pivot=int((st[:, 0] == 3).sum()), layout=F.factor_layout())
    finally:
        F.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fleet_adjoint_latency: no GPU visible; this measurement has no CPU form")
    lines = ["adjoint of a fleet's solve: %d config_qp('C3', i) items (n = 120, m = 360), max_iter %d; HIP events on the caller's stream, median (min ... max) of %d calls "
             "after %d untimed ones; ms" % (a.count, a.max_iter, a.reps, a.warmup),
             "%-7s | %6s %8s | %-26s | %-26s | %-26s | %9s %6s | %11s | %10s %11s" % ("scaling", "solved", "accepted", "adjoint", "adjoint + dQ, dA", "warm re-solve", "pass", "passes",
                                                                                      "adj / pass", "sweeps max", "sweeps mean")]
    extra = []
    for scaling in (10, 0):
        r = measure(a.count, scaling, a.reps, a.warmup, a.max_iter)
        f = lambda t: "%8.3f (%7.3f ... %7.3f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])
        lines.append("%-7d | %6d %8d | %s | %s | %s | %9.4f %6d | %11.2f | %10d %11.2f" % (
            scaling, r["solved"], r["accepted"], f(r["adj"]), f(r["adjm"]), f(r["resolve"]), 1e3 * r["one_pass"], r["iters"], r["adj"][0] / r["one_pass"],
            r["sweeps_max"], r["sweeps_mean"]))
        extra.append("scaling %d: %d items not accepted (code 1), %d with a bad pivot (code 3); mean of adj_status[:, 1] over all %d items %.2f" % (
            scaling, r["not_accepted"], r["bad_pivot"], r["count"], r["sweeps_mean_all"]))
    lines.append("sweeps max / mean: over every item that swept (codes 0 and 1; an item with code 2 or 3 reports 0 sweeps).  " + "; ".join(extra) + ".")
    lines.append("pass: last_kernel_seconds of the cold solve launch over the largest `iterations` among its items (one Newton pass of the slowest item, the launch being as "
                 "long as that item); adj / pass: the adjoint launch in such passes.  Items whose solve did not reach status 1 within max_iter leave the adjoint launch at once (code 2).")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
