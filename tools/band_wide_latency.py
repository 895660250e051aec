"""Latency of the band solver for half-bandwidths 128 .. 1023 (dev/band_wide.inc) against the default path on the same instance.

usage: band_wide_latency.py [--n 4096,20000,100000] [--b 128,256,512,1023] [--reps 3] [--out FILE]

Per (n, b), on problems.banded_random_qp(900 + b, n, b):
  factor+solve, solve   one qpdo_amd_direct_solve with and without a refactorization (host wall clock around the call, which uploads the
                        weights and the right-hand side and waits for the result; best of --reps), their difference = the factorization
  band solve            the whole qpdo_solve with QPDO_LINSOLVE=band
  default solve         the whole qpdo_solve with QPDO_LINSOLVE unset (dense up to n = 12288, PCG above)
On a commit without the wide solver the band columns read "refused" (qpdo_setup fails) and the default column is the comparison.
MFMA fraction: the update kernel's flops, 2 * 64^3 per tile pair, over the factorization time and the 78.6 TFLOP/s fp64 matrix peak."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver

PEAK = 78.6e12


def best(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


def update_flops(n, b):
    nbc, w = (n + 63) // 64, (b + 63) // 64
    tot = 0
    for k in range(nbc):
        wk = min(w, nbc - 1 - k)
        tot += wk * (wk + 1) // 2
    return tot * 2.0 * 64 ** 3


def whole_solve(p, linsolve):
    if linsolve:
        os.environ["QPDO_LINSOLVE"] = linsolve
    else:
        os.environ.pop("QPDO_LINSOLVE", None)
    try:
        s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    except RuntimeError:
        return None
    try:
        t0 = time.perf_counter(); r = s.solve(); dt = time.perf_counter() - t0
        st = s.stats()
    finally:
        s.delete()
    return dt, r["info"]["status_val"], r["info"]["iterations"], st["linsolve"], st["factor_count"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,20000,100000")
    ap.add_argument("--b", default="128,256,512,1023")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["%7s %5s | %14s %10s %10s %6s | %22s | %26s" % ("n", "b", "factor+solve ms", "solve ms", "factor ms", "MFMA %",
                                                              "band solve s (passes)", "default solve s (solver)")]
    print(lines[0], flush=True)
    for n in [int(v) for v in a.n.split(",")]:
        for b in [int(v) for v in a.b.split(",")]:
            if n < 4 * (b + 1):
                continue
            p = problems.banded_random_qp(900 + b, n, b)
            rng = np.random.default_rng(b)
            dw, rhs = 0.1 + 9.9 * rng.random(p["m"]), rng.standard_normal(n)
            os.environ["QPDO_LINSOLVE"] = "band"
            try:
                ws = solver.QPDO().setup(p["Q"], np.zeros(n), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)
            except RuntimeError:
                ws = None
            if ws is not None:
                try:
                    ws.direct_solve(dw, 1.0, rhs, refactor=True)                      # allocation, first launches
                    tfs = best(lambda: ws.direct_solve(dw, 1.0, rhs, refactor=True), a.reps)
                    ts = best(lambda: ws.direct_solve(dw, 1.0, rhs, refactor=False), a.reps)
                finally:
                    ws.delete()
                tf = max(tfs - ts, 1e-9)
                lin = "%14.2f %10.2f %10.2f %6.2f" % (tfs * 1e3, ts * 1e3, tf * 1e3, 100.0 * update_flops(n, b) / tf / PEAK)
                rb = whole_solve(p, "band")
                band = "%8.3f (%d, status %d)" % (rb[0], rb[2], rb[1])
            else:
                lin, band = "%14s %10s %10s %6s" % ("refused", "-", "-", "-"), "refused"
            rd = whole_solve(p, None)
            dflt = "%8.3f (%s, status %d)" % (rd[0], {0: "pcg", 1: "dense", 2: "fused", 3: "band"}[rd[3]], rd[1])
            lines.append("%7d %5d | %s | %22s | %26s" % (n, b, lin, band, dflt))
            print(lines[-1], flush=True)
            if a.out:                                                             # (rewritten per row: a run cut short keeps its rows)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
