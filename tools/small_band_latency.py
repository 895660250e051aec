#!/usr/bin/env python3
"""What the fused small-QP kernel costs on chain-structured QPs whose packed factor does not fit the workgroup's LDS, with the Newton
matrix in global memory (the parent of the band layout) and as a lower band in LDS (include/qpdo_amd_ext.h, QPDO_AMD_SMALL_K_BAND).

Uses only calls both builds have (solve_batch, Fleet, the kernels' HIP-event times), so the same script measures either library:

  small_band_latency.py --series [--runs 5]                 one series with the library this process loads (QPDO_AMD_LIB or the tree's),
                                                            one JSON line per workload
  small_band_latency.py --baseline-lib PARENT.so --out F    alternates fresh child processes, parent / this build / parent / this build,
                                                            and writes the table: median, min .. max over all runs of each build

Workloads: 256 copies (seeds varied) of the shapes A (n 256, b 12), C (n 333, b 31), D (n 610, b 5), F (n 200, b 70) of
tests/test_gpu_small_band.py as one qpdo_amd_solve_batch each, by the kernel's HIP-event time; a fleet of 64 x A over ten closed-loop steps
(update q -> warm_start_last -> solve), the sum of the ten solve launches' event times; the control: 256 C3 items (n 120, m 360, packed
layout), which the band layout must not move.  One warm-up run of every workload, then --runs timed ones."""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPIES, FLEET_ITEMS, FLEET_STEPS = 256, 64, 10
SHAPES = dict(A=(256, 12), C=(333, 31), D=(610, 5), F=(200, 70))


def series(runs):
    import numpy as np
    from qpdo_amd import problems, solver
    st = dict(max_iter=1000, verbose=0)
    work = [("batch %s" % k, [problems.banded_random_qp(1000 + s, n, b) for s in range(COPIES)]) for k, (n, b) in SHAPES.items()]
    work.append(("batch C3 (control)", [problems.config_qp("C3", s) for s in range(COPIES)]))
    for name, probs in work:
        batch = solver.Batch(probs)
        times = []
        for r in range(runs + 1):
            _, failed = batch.run(results=False, **st)
            assert failed == 0
            if r:
                times.append(batch.kernel_seconds)
        info = batch.info_view()
        print(json.dumps(dict(workload=name, seconds=times, solved=int((info["status_val"] == 1).sum()), passes=int(info["iterations"].sum()))), flush=True)
    probs = [problems.banded_random_qp(2000 + s, 256, 12) for s in range(FLEET_ITEMS)]
    rng = np.random.default_rng(5)
    qs = [[p["q"] + 0.05 * rng.standard_normal(p["n"]) for p in probs] for _ in range(FLEET_STEPS)]
    times = []
    for r in range(runs + 1):
        F = solver.Fleet(probs, **st)
        F.solve(results=False)
        total = 0.0
        for q in qs:
            F.update(q=q)
            F.warm_start_last()
            F.solve(results=False)
            total += F.stats()["last_kernel_seconds"]
        F.close()
        if r:
            times.append(total)
    print(json.dumps(dict(workload="fleet 64 x A, %d steps" % FLEET_STEPS, seconds=times, solved=-1, passes=-1)), flush=True)


def child(lib, runs):
    env = dict(os.environ)
    if lib:
        env["QPDO_AMD_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--series", "--runs", str(runs)], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("series failed (%s): %s" % (lib, (p.stdout + p.stderr)[-2000:]))
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--this-lib", default=os.environ.get("QPDO_AMD_LIB", ""))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.series:
        return series(a.runs)
    if not a.baseline_lib:
        ap.error("--series or --baseline-lib")
    acc = {}
    for rep in range(2):                              # parent, this build, parent, this build: drift shows as spread, not as a difference
        for tag, lib in (("parent", a.baseline_lib), ("band", a.this_lib)):
            recs = child(lib, a.runs)
            print("series %d of the %s build done" % (rep + 1, tag), file=sys.stderr, flush=True)
            for rec in recs:
                e = acc.setdefault(rec["workload"], dict(parent=[], band=[], check={}))
                e[tag] += rec["seconds"]
                e["check"].setdefault(tag, (rec["solved"], rec["passes"]))
    lines = ["%-26s %33s %33s %8s  %s" % ("workload", "parent: median (min .. max) ms", "this build: median (min .. max) ms", "ratio", "verdict")]
    for name, e in acc.items():
        p, b = e["parent"], e["band"]
        mp, mb = statistics.median(p), statistics.median(b)
        if "control" in name:
            verdict = "inside the parent's spread" if min(p) <= mb <= max(p) else "OUTSIDE the parent's spread"
        else:
            verdict = "faster beyond the spread" if max(b) < min(p) else "NOT faster beyond the spread"
        same = "" if e["check"].get("parent") == e["check"].get("band") else "  (solved / passes differ: %r)" % (e["check"],)
        fmt = lambda v, m: "%9.3f (%9.3f .. %9.3f)" % (1e3 * m, 1e3 * min(v), 1e3 * max(v))
        lines.append("%-26s %33s %33s %7.2fx  %s%s" % (name, fmt(p, mp), fmt(b, mb), mp / mb, verdict, same))
    lines.append("(%d runs per build and workload after one warm-up run each, in two alternating series of fresh processes; HIP-event times of the launches)" % (2 * a.runs))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
