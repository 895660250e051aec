"""Latency of chain QPs with dense coupling rows: QPDO_BAND_COUPLING=64 (band plus low rank, dev/band.inc) against the variable unset,
which is the default path of the commit before it -- dense up to n = 12288, PCG above.

usage: band_coupled_latency.py [--n 4096,20000] [--b 5,31] [--r 1,8,64] [--reps 3] [--out profiles/band_coupled_latency.txt]
       band_coupled_latency.py --one FILE on|off          (child: one whole solve of the instance in FILE, prints one JSON line)
       band_coupled_latency.py --kernels N B K REPS       (child, run under the kernel trace: REPS refactoring linear solves with K weighted rows)

Whole solves: per (n, b, r) on tests/band_coupled_ref.coupled_banded_qp(11, n, b, r) -- generated once by this process, the free problem
behind the coupling rows' bounds solved on the device's default path (the oracle's dense factorization does not reach n = 20000) --, a
fresh process per solve, the two modes alternating, --reps repeats; the table gives each mode's median and its spread (max - min) in seconds, the passes and the solver that
ran.  The claim checked and recorded under the table: at n = 20000 the coupled path is not slower than the default path, with the
default path's own run-to-run spread as the margin.
Kernels: device time of ONE k_band_solve_multi launch with k = 1, 8 and 64 columns beside the time of one k_band_solve on the same
factor (n = 20000, b = 31, r = 64; rocprofv3 --kernel-trace in a run of its own per k, median over the launches)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SOLVERS = {0: "pcg", 1: "dense", 2: "fused", 3: "band"}


def default_path_x(p):
    from qpdo_amd import solver
    os.environ.pop("QPDO_LINSOLVE", None)
    os.environ.pop("QPDO_BAND_COUPLING", None)
    res = solver.solve_problem(p, verbose=0)
    if res["info"]["status_val"] != 1:
        raise RuntimeError("instance generation: the free problem ended with status %d" % res["info"]["status_val"])
    return res["x"]


def save_instance(path, p):
    import numpy as np
    A, Q = p["A"].tocsc(), p["Q"].tocsc()
    np.savez(path, n=p["n"], m=p["m"], Ap=A.indptr, Ai=A.indices, Ax=A.data, Qp=Q.indptr, Qi=Q.indices, Qx=Q.data, q=p["q"], l=p["l"], u=p["u"])


def load_instance(path):
    import numpy as np
    import scipy.sparse as sp
    z = np.load(path)
    n, m = int(z["n"]), int(z["m"])
    return dict(n=n, m=m, A=sp.csc_matrix((z["Ax"], z["Ai"], z["Ap"]), shape=(m, n)), Q=sp.csc_matrix((z["Qx"], z["Qi"], z["Qp"]), shape=(n, n)),
                q=z["q"], l=z["l"], u=z["u"])


def one(path, mode):
    from qpdo_amd import solver
    os.environ.pop("QPDO_LINSOLVE", None)
    if mode == "on":
        os.environ["QPDO_BAND_COUPLING"] = "64"
    else:
        os.environ.pop("QPDO_BAND_COUPLING", None)
    p = load_instance(path)
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    solver.lib().qpdo_amd_sync(s._w)
    t0 = time.perf_counter(); res = s.solve(); dt = time.perf_counter() - t0
    st = s.stats()
    s.delete()
    print(json.dumps(dict(seconds=dt, status=res["info"]["status_val"], passes=res["info"]["iterations"], linsolve=st["linsolve"],
                          factors=st["factor_count"], coupled_solves=st["coupled_solves"], coupled_sweeps=st["coupled_sweeps"],
                          coupled_rejects=st["coupled_rejects"], band_fallbacks=st["band_fallbacks"], lin_iters=st["lin_iters"])))


def kernels(n, b, k, reps):
    import numpy as np
    import band_coupled_ref as ref
    from qpdo_amd import problems, solver
    r = 64
    base = problems.banded_random_qp(900 + b, n, b)
    p = ref.append_rows(base, ref.coupling_rows(900 + b, n, r), -np.ones(r), np.ones(r))
    os.environ["QPDO_LINSOLVE"], os.environ["QPDO_BAND_COUPLING"] = "band", "64"
    rng = np.random.default_rng(b)
    dw, rhs = 0.1 + 9.9 * rng.random(p["m"]), rng.standard_normal(n)
    dw[p["m"] - r + k:] = 0.0                                # k weighted coupling rows
    ws = solver.QPDO().setup(p["Q"], np.zeros(n), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)
    for _ in range(reps + 1):
        ws.direct_solve(dw, 1.0, rhs, refactor=True)
    ws.delete()


def child(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("child %s failed (%d): %s" % (args, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def kernel_times(n, b, k, reps):
    """median device time in us of k_band_solve_multi and of k_band_solve over the launches of one traced child"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
               "--kernels", str(n), str(b), str(k), str(reps)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        if out.returncode != 0:
            raise RuntimeError("traced child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
        durs = {"k_band_solve_multi": [], "k_band_solve": []}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"].split("(")[0]
                    if name in durs:
                        durs[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    if not durs["k_band_solve_multi"] or not durs["k_band_solve"]:
        raise RuntimeError("the trace holds no launch of the band solve kernels")
    # (the first call of the child is the warm-up: its launches are dropped)
    return {name: (statistics.median(v[1:] if len(v) > 1 else v), len(v)) for name, v in durs.items()}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        return one(sys.argv[2], sys.argv[3])
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        return kernels(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,20000")
    ap.add_argument("--b", default="5,31")
    ap.add_argument("--r", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_coupled_latency.txt"))
    a = ap.parse_args()
    import band_coupled_ref as ref
    lines = ["whole qpdo_solve, seconds: median (max - min) over %d fresh processes per mode, the modes alternating" % a.reps,
             "%6s %3s %3s | %28s | %28s | %s" % ("n", "b", "r", "QPDO_BAND_COUPLING=64", "unset (default path)", "coupled: passes, factors, solves, sweeps, rejects, fallbacks")]
    verdicts = []

    def flush():
        with open(a.out, "w") as f:                         # (rewritten per row: a run cut short keeps its rows)
            f.write("\n".join(lines + verdicts) + "\n")

    for ln in lines:
        print(ln, flush=True)
    for n in [int(v) for v in a.n.split(",")]:
        for b in [int(v) for v in a.b.split(",")]:
            for r in [int(v) for v in a.r.split(",")]:
                runs = {"on": [], "off": []}
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "instance.npz")
                    save_instance(path, ref.coupled_banded_qp(11, n, b, r, solve=default_path_x))
                    for rep in range(a.reps):
                        for mode in (("on", "off") if rep % 2 == 0 else ("off", "on")):
                            runs[mode].append(child(["--one", path, mode]))
                cell = {}
                for mode, rs in runs.items():
                    ts = [x["seconds"] for x in rs]
                    cell[mode] = (statistics.median(ts), max(ts) - min(ts))
                on, off = runs["on"][-1], runs["off"][-1]
                lines.append("%6d %3d %3d | %8.3f (%6.3f) %-5s st %2d | %8.3f (%6.3f) %-5s st %2d | %d, %d, %d, %d, %d, %d%s" % (
                    n, b, r, cell["on"][0], cell["on"][1], SOLVERS[on["linsolve"]], on["status"], cell["off"][0], cell["off"][1],
                    SOLVERS[off["linsolve"]], off["status"], on["passes"], on["factors"], on["coupled_solves"], on["coupled_sweeps"],
                    on["coupled_rejects"], on["band_fallbacks"], "" if on["passes"] == off["passes"] else "  (default path: %d passes)" % off["passes"]))
                print(lines[-1], flush=True)
                if n == 20000:
                    ok = cell["on"][0] <= cell["off"][0] + cell["off"][1]
                    verdicts.append("claim at n = %d, b = %d, r = %d: coupled %.3f s <= default %.3f s + its spread %.3f s: %s" % (
                        n, b, r, cell["on"][0], cell["off"][0], cell["off"][1], "HOLDS" if ok else "DOES NOT HOLD"))
                flush()
    for v in verdicts:
        print(v, flush=True)
    if not a.no_kernels:
        verdicts.append("device time of one launch, us (median; n = 20000, b = 31, r = 64):")
        for k in (1, 8, 64):
            kt = kernel_times(20000, 31, k, 5)
            verdicts.append("  k = %2d: k_band_solve_multi %9.1f (%d launches)   k_band_solve %9.1f (%d launches)" % (
                k, kt["k_band_solve_multi"][0], kt["k_band_solve_multi"][1], kt["k_band_solve"][0], kt["k_band_solve"][1]))
            print(verdicts[-1], flush=True)
            flush()


if __name__ == "__main__":
    main()
