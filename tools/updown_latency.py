"""Whole-solve wall time of mid-size single QPs (the problems of tools/mid_latency.py) with the in-place up/downdate of the kept dense
factor off (the default path, launch-ahead included) and on with caps 1, 3, 5, 9 (QPDO_DENSE_UPDOWN, read at qpdo_setup).
usage: updown_latency.py [--reps R] [--only n,n,...] [--modes off,1,3,...]
Every mode gets its own workspace; the modes are timed alternately, R rounds after one warm-up solve each, and the table gives the
median and the min .. max of a mode's R solves (the spread a difference has to beat), the passes, factorizations and updown counters."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver

PROBLEMS = {200: lambda: problems.config_qp("C1"), 500: lambda: problems.random_qp(32, 500, 1000, 0.05),
            1000: lambda: problems.random_qp(33, 1000, 2000, 0.02), 2000: lambda: problems.random_qp(34, 2000, 4000, 0.01),
            4000: lambda: problems.random_qp(35, 4000, 8000, 0.01)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="200,500,1000,2000,4000")
    ap.add_argument("--modes", default="off,1,3,5,9")
    a = ap.parse_args()
    modes = a.modes.split(",")
    os.environ["QPDO_LINSOLVE"] = "dense"
    print("%6s %5s %10s %19s %7s %8s %7s %7s %8s %7s" % ("n", "mode", "median ms", "min .. max ms", "passes", "factors", "ud rows", "ud slv", "ud rej", "status"), flush=True)
    for n in [int(x) for x in a.only.split(",")]:
        p = PROBLEMS[n]()
        ws = {}
        for mode in modes:
            os.environ.pop("QPDO_DENSE_UPDOWN", None)
            if mode != "off":
                os.environ["QPDO_DENSE_UPDOWN"] = mode
            ws[mode] = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
            ws[mode].solve()
        times = {mode: [] for mode in modes}
        last = {}
        for rep in range(a.reps):
            for mode in modes:
                t = time.perf_counter()
                last[mode] = ws[mode].solve()          # (returns after the solution has been copied back: a device synchronise)
                times[mode].append(time.perf_counter() - t)
        for mode in modes:
            st = ws[mode].stats()
            ts = [1e3 * t for t in times[mode]]
            print("%6d %5s %10.3f %8.3f .. %8.3f %7d %8d %7d %7d %8d %7d" % (p["n"], mode, statistics.median(ts), min(ts), max(ts), last[mode]["info"]["iterations"],
                  st["factor_count"], st["updown_rows"], st["updown_solves"], st["updown_rejects"], last[mode]["info"]["status_val"]), flush=True)
            ws[mode].delete()


if __name__ == "__main__":
    main()
