"""Latency of chain QPs whose variables are not numbered along the chain: QPDO_BAND_ORDER=rcm (reverse Cuthill-McKee on the host, the band
solver under that order; qpdo_amd/csrc/band_order.c) against the variable unset, which is the route of the commit before it for such a
problem (dense up to n = 12288, PCG above), and against the same QP numbered along the chain on the natural-order band solver -- what
the order can at best give back.

usage: band_order_latency.py [--n 20000] [--reps 12] [--warmup 3] [--out profiles/band_order_latency.txt]

Problems: problems.banded_qp(1, n) and problems.banded_random_qp(7, n, 31), each relabelled even indices first, then odd.  Per problem and
mode a fresh workspace per repeat in ONE process: qpdo_setup (host clock; it ends synchronised), then qpdo_solve (host clock around the
call, which ends with the solution on the host).  The modes alternate their order from repeat to repeat; --warmup repeats are dropped,
the table gives the median and the spread (max - min) of the other --reps.  order_seconds (QPDOAmdBandOrderInfo: the ordering itself, on
the host) stands beside the setup time it is part of.  No speed-up is fixed in advance: the table is the measurement."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVERS = {0: "pcg", 1: "dense", 2: "fused", 3: "band"}
MODES = ("rcm", "unset", "chain")          # relabelled + QPDO_BAND_ORDER=rcm | relabelled, unset | numbered along the chain, unset


def run(p, mode):
    from qpdo_amd import solver
    os.environ.pop("QPDO_LINSOLVE", None)
    if mode == "rcm":
        os.environ["QPDO_BAND_ORDER"] = "rcm"
    else:
        os.environ.pop("QPDO_BAND_ORDER", None)
    t0 = time.perf_counter()
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    solver.lib().qpdo_amd_sync(s._w)
    t1 = time.perf_counter()
    res = s.solve()
    t2 = time.perf_counter()
    st, bo = s.stats(), s.band_order_info()
    s.delete()
    return dict(setup=t1 - t0, solve=t2 - t1, status=res["info"]["status_val"], passes=res["info"]["iterations"], linsolve=st["linsolve"],
                factors=st["factor_count"], order_seconds=bo["order_seconds"], adopted=bo["adopted"], b_natural=bo["b_natural"], b_ordered=bo["b_ordered"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_order_latency.txt"))
    a = ap.parse_args()
    import numpy as np
    from qpdo_amd import problems, solver
    if solver.device_count() < 1:
        raise SystemExit("band_order_latency: no HIP device (a measurement needs the GPU)")
    lines = ["whole qpdo_solve and qpdo_setup, seconds: median (max - min) of %d repeats after %d, fresh workspace per repeat, the modes alternating" % (a.reps, a.warmup),
             "rcm: relabelled even/odd, QPDO_BAND_ORDER=rcm | unset: relabelled, the variable unset (the route without the order) | chain: numbered along the chain, unset",
             "%-26s %-5s | %-6s %3s | %19s | %19s | %13s | %s" % ("problem", "mode", "solver", "st", "solve", "setup", "order_seconds", "passes, factors, b natural -> ordered")]

    def flush():
        with open(a.out, "w") as f:                         # (rewritten per row: a run cut short keeps its rows)
            f.write("\n".join(lines) + "\n")

    for ln in lines:
        print(ln, flush=True)
    shuffle = np.concatenate([np.arange(0, a.n, 2), np.arange(1, a.n, 2)])
    for name, p in (("banded_qp(1, %d)" % a.n, problems.banded_qp(1, a.n)), ("banded_random_qp(7, %d, 31)" % a.n, problems.banded_random_qp(7, a.n, 31))):
        inst = {"rcm": problems.permute_variables(p, shuffle), "chain": p}
        inst["unset"] = inst["rcm"]
        runs = {m: [] for m in MODES}
        for rep in range(a.warmup + a.reps):
            for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
                r = run(inst[mode], mode)
                if rep >= a.warmup:
                    runs[mode].append(r)
        for mode in MODES:
            rs = runs[mode]
            cell = {k: (statistics.median([x[k] for x in rs]), max(x[k] for x in rs) - min(x[k] for x in rs)) for k in ("solve", "setup", "order_seconds")}
            last = rs[-1]
            lines.append("%-26s %-5s | %-6s %3d | %9.4f (%7.4f) | %9.4f (%7.4f) | %13.4f | %d, %d, %d -> %d%s" % (
                name, mode, SOLVERS[last["linsolve"]], last["status"], cell["solve"][0], cell["solve"][1], cell["setup"][0], cell["setup"][1],
                cell["order_seconds"][0], last["passes"], last["factors"], last["b_natural"], last["b_ordered"], "" if mode != "rcm" or last["adopted"] else "  (NOT adopted)"))
            print(lines[-1], flush=True)
            flush()


if __name__ == "__main__":
    main()
