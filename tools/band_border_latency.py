"""Latency of chain QPs with a few coupling variables: QPDO_BAND_BORDER=64 (bordered band by block elimination, dev/band.inc) against the
variable unset, which is the default path on the same build -- dense up to n = 12288, PCG above.

usage: band_border_latency.py [--n 4096,20000] [--b 5,31] [--c 1,8,64] [--reps 12] [--warmup 3] [--max-seconds 120]
                              [--out profiles/band_border_latency.txt] [--no-kernels]
       band_border_latency.py --kernels N B C REPS        (child, run under the kernel trace: REPS refactoring linear solves)

Whole solves: per (n_core, b, c) on problems.bordered_banded_qp(11, n_core, b, c), two workspaces in ONE process -- the variable set for
the first setup, unset for the second --, every solve from the cold start x = y = 0 (an explicit warm start with zeros, outside the
timed window), host clock around qpdo_solve (which ends synchronised).  The two modes alternate; --warmup untimed solves per mode, then
--reps timed ones: the table gives each mode's median and min ... max in seconds, the status, the passes and the solver that ran.  A cell
whose solves would take longer than --max-seconds in all is cut short and says how many timed solves it holds.
Kernels: device time of ONE refresh (band_border_refresh) split into B (k_band_assemble + k_band_factor), Z (k_bb_assemble +
k_band_solve_group) and S (k_bb_S + k_bc_factor_S), and of one solve (k_band_solve + k_bb_t + k_bb_apply); rocprofv3 --kernel-trace in a
run of its own per shape, median over the calls behind the first."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVERS = {0: "pcg", 1: "dense", 2: "fused", 3: "band"}
PARTS = {"B": ("k_band_assemble", "k_band_factor"), "Z": ("k_bb_assemble", "k_band_solve_group"), "S": ("k_bb_S", "k_bc_factor_S"),
         "solve": ("k_band_solve", "k_bb_t", "k_bb_apply")}


def workspace(p, border):
    from qpdo_amd import solver
    os.environ.pop("QPDO_LINSOLVE", None)
    os.environ.pop("QPDO_BAND_COUPLING", None)
    os.environ.pop("QPDO_BAND_ORDER", None)
    if border:
        os.environ["QPDO_BAND_BORDER"] = "64"
    else:
        os.environ.pop("QPDO_BAND_BORDER", None)
    return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)


def timed_solve(s, x0, y0):
    from qpdo_amd import solver
    s.warm_start(x0, y0)
    solver.lib().qpdo_amd_sync(s._w)
    t0 = time.perf_counter()
    res = s.solve()
    return time.perf_counter() - t0, res


def kernels(n, b, c, reps):
    import numpy as np
    from qpdo_amd import problems, solver
    p = problems.bordered_banded_qp(900 + b, n, b, c)
    os.environ["QPDO_LINSOLVE"], os.environ["QPDO_BAND_BORDER"] = "band", "64"
    rng = np.random.default_rng(b)
    dw, rhs = 0.1 + 9.9 * rng.random(p["m"]), rng.standard_normal(p["n"])
    ws = solver.QPDO().setup(p["Q"], np.zeros(p["n"]), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)
    assert ws.band_border()["border"] == c
    for _ in range(reps + 1):
        ws.direct_solve(dw, 1.0, rhs, refactor=True)
    ws.delete()


def kernel_times(n, b, c, reps):
    """median device time in us of the parts of one refresh and one solve over the calls of one traced child (the first call is the warm-up)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
               "--kernels", str(n), str(b), str(c), str(reps)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            raise RuntimeError("traced child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
        durs = {k: [] for names in PARTS.values() for k in names}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")
                    if name in durs:
                        durs[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    if any(not v for v in durs.values()):
        raise RuntimeError("the trace misses launches of %s" % [k for k, v in durs.items() if not v])
    return {part: sum(statistics.median(durs[k][1:] if len(durs[k]) > 1 else durs[k]) for k in names) for part, names in PARTS.items()}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        return kernels(*(int(v) for v in sys.argv[2:6]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,20000")
    ap.add_argument("--b", default="5,31")
    ap.add_argument("--c", default="1,8,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-seconds", type=float, default=120.0)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_border_latency.txt"))
    a = ap.parse_args()
    import numpy as np
    from qpdo_amd import problems, solver
    if solver.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured")
    lines = ["whole qpdo_solve from x = y = 0, seconds: median (min ... max) of the timed solves of one process, the modes alternating, %d untimed solves per mode first" % a.warmup,
             "%6s %3s %3s | %44s | %44s" % ("n_core", "b", "c", "QPDO_BAND_BORDER=64", "unset (default path)")]
    tail = []

    def flush():
        with open(a.out, "w") as f:                         # (rewritten per row: a run cut short keeps its rows)
            f.write("\n".join(lines + tail) + "\n")

    for ln in lines:
        print(ln, flush=True)
    shapes = [(n, b, c) for n in [int(v) for v in a.n.split(",")] for b in [int(v) for v in a.b.split(",")] for c in [int(v) for v in a.c.split(",")]]
    for n, b, c in shapes:
        p = problems.bordered_banded_qp(11, n, b, c)
        x0, y0 = np.zeros(p["n"]), np.zeros(p["m"])
        ws = {"on": workspace(p, True), "off": workspace(p, False)}
        assert ws["on"].band_border()["border"] == c and ws["off"].band_border()["border"] == 0
        runs, last, spent = {"on": [], "off": []}, {}, 0.0
        for rep in range(a.warmup + a.reps):
            for mode in (("on", "off") if rep % 2 == 0 else ("off", "on")):
                dt, res = timed_solve(ws[mode], x0, y0)          # (a solve that ends with an error status is timed and shown with that status)
                spent += dt
                last[mode] = (res["info"]["status_val"], res["info"]["iterations"], ws[mode].stats())
                if rep >= a.warmup:
                    runs[mode].append(dt)
            if spent > a.max_seconds and rep >= a.warmup:
                break
        cells = []
        for mode in ("on", "off"):
            ts, (status, passes, st) = runs[mode], last[mode]
            cells.append("%8.4f (%8.4f ... %8.4f) %-5s st %2d %3d passes" % (statistics.median(ts), min(ts), max(ts), SOLVERS[st["linsolve"]], status, passes))
        note = "" if len(runs["on"]) == a.reps else "  (%d timed solves per mode: cut at --max-seconds)" % len(runs["on"])
        extra = "  border_solves %d, band_fallbacks %d" % (ws["on"].band_border()["border_solves"], last["on"][2]["band_fallbacks"])
        lines.append("%6d %3d %3d | %s | %s%s%s" % (n, b, c, cells[0], cells[1], extra, note))
        print(lines[-1], flush=True)
        for s in ws.values():
            s.delete()
        flush()
    if not a.no_kernels:
        tail.append("device time of one refresh (B = assemble + factor of the core, Z = border columns + B^-1 C, S = Schur complement + its factor) and of one solve, us (median of 5 calls):")
        for n, b, c in shapes:
            kt = kernel_times(n, b, c, 5)
            tail.append("  n_core = %5d, b = %2d, c = %2d: B %9.1f   Z %9.1f   S %9.1f   solve %9.1f" % (n, b, c, kt["B"], kt["Z"], kt["S"], kt["solve"]))
            print(tail[-1], flush=True)
            flush()


if __name__ == "__main__":
    main()
