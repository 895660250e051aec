#!/usr/bin/env python3
"""Re-linearised control step of a fleet of MPC-sized QPs (new Q and A values in the same pattern every step): what does it cost through
(a) Fleet.update_matrices + warm_start_last + solve on a fleet created with matrix_updates=True -- one upload of the values, three launches --
against (b) what existed before it: destroy the fleet, create it again on the new data (host conversions, the whole upload, allocations,
tpos, scaling), warm_start with the previous x, y from the host, solve?

    python tools/fleet_matrix_update_latency.py [--count 4096] [--steps 3] [--repeats 3] [--max-iter 300] [--out profiles/fleet_matrix_update_latency.txt]

Both paths run in one process on the same data; which one goes first alternates per step and per repeat.  Times are wall clock around the C
calls only (the scipy -> ctypes images of both paths are prepared outside the timed region).  Two rows: every item changes, and 1 % of the
items change (path (b) has no cheaper way for that).  The claim to check is "(a) is not slower than (b)", the margin being (b)'s run-to-run
spread.  Also printed: the HIP-event time of k_small_fleet_matrices against its algorithmic bytes."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402

HBM_BYTES_PER_S = 8.0e12     # MI355X: 8 TB/s peak


def step_values(p, k):
    """an SQP-like step: every value moves by a few percent, smoothly in k; Q stays S Q S with a positive diagonal S (convex)"""
    Q, A = sp.csc_matrix(p["Q"], copy=True), sp.csc_matrix(p["A"], copy=True)
    Q.sort_indices(); A.sort_indices()
    s = 1.0 + 0.05 * np.sin(0.37 * k + 0.1 * np.arange(p["n"]))
    r = 1.0 + 0.05 * np.cos(0.23 * k + 0.07 * np.arange(p["m"]))
    Q.data = Q.data * s[Q.indices] * s[np.repeat(np.arange(p["n"]), np.diff(Q.indptr))]
    A.data = A.data * r[A.indices] * s[np.repeat(np.arange(p["n"]), np.diff(A.indptr))]
    return Q, A


def kernel_bytes(probs, scaling):
    """algorithmic bytes of one k_small_fleet_matrices launch that gives every item a new Q and A (what the code reads and writes, caches ignored)"""
    gather = ruiz = 0
    for p in probs:
        n, m = p["n"], p["m"]
        a, qs, qf = sp.csc_matrix(p["A"]).nnz, sp.csc_matrix(p["Q"]).nnz, problems.full_Q(p).nnz
        gather += 8 * (a + qs) + 4 * (a + qf) + 8 * 2 * (2 * a + qf) + 8 * 2 * (n + 2 * m)     # staging, maps, three images + their unscaled copies (Tval read back for the gather), q l u
        per_iter = 16 * a + 4 * (n + m) + 8 * 2 * (n + m) + 48 * a + 8 * a                      # two norm passes; two scaling passes (read + write, column indices)
        ruiz += 8 * (6 * n + 7 * m) + scaling * per_iter + 2 * (16 * qf) + 4 * qf + 8 * (6 * n + 6 * m)
    return gather, ruiz


def run(probs, steps, st, fraction, first, data):
    N = len(probs)
    settings = solver.default_settings(**st)
    Fa = solver.Fleet(probs, settings=settings, matrix_updates=True)
    Fb = solver.Fleet(probs, settings=settings)
    L = solver.lib()
    Fa.solve(results=False); Fb.solve(results=False)
    assert np.array_equal(Fa.info_view()["status_val"], Fb.info_view()["status_val"]), "cold solve: statuses differ"
    rows = []
    for k in range(1, steps + 1):
        img, arr, Qa, Aa, entries = data[(k, fraction)]
        sb = Fb.info_view()["status_val"].copy()
        xs = [None if sb[i] in (-3, -4, -10, -99) else Fb.outs[i][0].copy() for i in range(N)]
        ys = [None if sb[i] in (-3, -4, -10, -99) else Fb.outs[i][1].copy() for i in range(N)]
        xp, kx = Fb._ptrs(xs, ("x", 0))
        yp, ky = Fb._ptrs(ys, ("y", 1))

        def path_b():
            t0 = time.perf_counter()
            L.qpdo_amd_fleet_destroy(Fb._h)
            Fb._h = L.qpdo_amd_fleet_create(N, arr, C.byref(settings))
            assert Fb._h, L.qpdo_amd_last_error()
            t1 = time.perf_counter()
            assert L.qpdo_amd_fleet_warm_start(Fb._h, xp, yp) == 0
            assert L.qpdo_amd_fleet_solve(Fb._h, Fb._xp, Fb._yp, Fb._info) == 0
            return time.perf_counter() - t0, t1 - t0

        def path_a():
            t0 = time.perf_counter()
            assert L.qpdo_amd_fleet_update_matrices(Fa._h, Qa, Aa) == 0, L.qpdo_amd_last_error()
            t1 = time.perf_counter()
            assert L.qpdo_amd_fleet_warm_start_last(Fa._h) == 0
            assert L.qpdo_amd_fleet_solve(Fa._h, Fa._xp, Fa._yp, Fa._info) == 0
            return time.perf_counter() - t0, t1 - t0

        if (k + first) % 2:
            (tb, tb_c), (ta, ta_m) = path_b(), path_a()
        else:
            (ta, ta_m), (tb, tb_c) = path_a(), path_b()
        ms = Fa.matrix_stats()
        fa, fb = Fa.info_view(), Fb.info_view()
        capped = (fa["iterations"] >= st["max_iter"]) | (fb["iterations"] >= st["max_iter"])
        differ = fa["status_val"] != fb["status_val"]
        # every item: (a) is the workspace (b) sets up, bit for bit -- when all items change the two paths are the same computation
        if fraction == 1.0:
            assert not differ.any() and np.array_equal(fa["iterations"], fb["iterations"]), "step %d: the two paths differ" % k
            assert all(np.array_equal(Fa.outs[i][0], Fb.outs[i][0], equal_nan=True) for i in range(N)), "step %d: x differs" % k
        else:
            assert not (differ & ~capped).any(), "step %d: statuses differ below the pass limit" % k
        rows.append(dict(a=ta, a_mat=ta_m, a_kernel=ms["last_kernel_seconds"], a_bytes=ms["value_bytes_uploaded_last_call"], items=ms["items_last_call"],
                         b=tb, b_create=tb_c, b_bytes=Fb.stats()["matrix_bytes_uploaded"], passes=int(fa["iterations"].sum())))
    extra = Fa.matrix_stats()["resident_extra_bytes"]
    Fa.close(); Fb.close()
    return rows, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="label for the table (default: git rev-parse of this tree)")
    a = ap.parse_args()
    probs = [problems.config_qp("C3", i) for i in range(a.count)]
    N = len(probs)
    st = dict(verbose=0, max_iter=a.max_iter)
    commit = a.commit
    try:
        if commit is None:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), text=True,
                                             stderr=subprocess.DEVNULL).strip() + " (+ working tree)"
    except Exception:
        commit = "unknown"
    # the host images of every step, for both paths, outside the timed region; the 1 % row changes the same items every step (cumulatively)
    shape = solver.Fleet.__new__(solver.Fleet)
    shape._h, shape.count, shape.dims, shape._qstype = None, N, [(p["n"], p["m"]) for p in probs], [int(p.get("Qstype", -1)) for p in probs]
    some = set(range(0, N, 100))
    data = {}
    for fraction, idx in ((1.0, set(range(N))), (0.01, some)):
        for k in range(1, a.steps + 1):
            vals = [step_values(p, k) if i in idx else None for i, p in enumerate(probs)]
            newp = [p if v is None else dict(p, Q=v[0], A=v[1]) for p, v in zip(probs, vals)]
            img = solver.Batch(newp)
            arr = (C.POINTER(solver.QPDOData) * N)(*[img.items[i].data for i in range(N)])
            Qa, kq = shape._mat_ptrs([None if v is None else v[0] for v in vals], "Q")
            Aa, ka = shape._mat_ptrs([None if v is None else v[1] for v in vals], "A")
            entries = sum(v[0].nnz + v[1].nnz for v in vals if v is not None)
            data[(k, fraction)] = (img, arr, Qa, Aa, (entries, kq, ka))
            print("host images of step %d prepared (fraction %g)" % (k, fraction), file=sys.stderr, flush=True)
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    lines = ["re-linearised step over %d config_qp('C3', i) items, %d steps after the cold solve, max_iter %d; commit %s" % (N, a.steps, a.max_iter, commit),
             "(a) update_matrices + warm_start_last + solve on a fleet with matrix_updates;  (b) destroy + create on the new data + warm_start(x, y from the host) + solve",
             "median per step over the steps of a run; times in ms, wall clock around the C calls; the order of the two paths alternates per step and per run.",
             "all items change: both paths must return the same statuses, pass counts and x bits (asserted)"]
    verdicts = []
    for fraction in (1.0, 0.01):
        lines.append("")
        lines.append("items that change per step: %s" % ("all" if fraction == 1.0 else "1 %% (%d items)" % len(some)))
        lines.append("%-4s | %9s %9s %9s %12s %6s | %9s %9s %12s | %8s" % ("run", "(a) step", "matrices", "kernel", "bytes up", "items", "(b) step", "create", "bytes up", "passes"))
        am, bm, ks = [], [], []
        for r in range(a.repeats):
            rows, extra = run(probs, a.steps, st, fraction, r, data)
            print("run %d of %d done (fraction %g)" % (r + 1, a.repeats, fraction), file=sys.stderr, flush=True)
            am.append(med(rows, "a")); bm.append(med(rows, "b")); ks.append(med(rows, "a_kernel"))
            lines.append("%-4d | %9.3f %9.3f %9.3f %12d %6d | %9.3f %9.3f %12d | %8d" % (
                r, 1e3 * med(rows, "a"), 1e3 * med(rows, "a_mat"), 1e3 * med(rows, "a_kernel"), int(med(rows, "a_bytes")), int(med(rows, "items")),
                1e3 * med(rows, "b"), 1e3 * med(rows, "b_create"), int(med(rows, "b_bytes")), int(med(rows, "passes"))))
        spread = max(bm) - min(bm)
        ma, mb = float(np.median(am)), float(np.median(bm))
        lines.append("(b) step: median of runs %.3f ms, run-to-run spread (max - min of %d runs) %.3f ms;  (a) step: %.3f ms, spread %.3f ms;  (b) / (a) = %.2f" % (
            1e3 * mb, a.repeats, 1e3 * spread, 1e3 * ma, 1e3 * (max(am) - min(am)), mb / ma))
        ok = ma <= mb + spread
        verdicts.append(ok)
        lines.append("claim '(a) is not slower than (b) (margin: (b)'s spread)': %s" % ("HOLDS" if ok else "FAILS"))
        if fraction == 1.0:
            g, z = kernel_bytes(probs, 10)
            kt = float(np.median(ks))
            lines.append("k_small_fleet_matrices, all items: %.3f ms (HIP events).  Algorithmic bytes (caches ignored): gather %d = staging 8 (nnzA + nnzQ stored) + maps" % (1e3 * kt, g))
            lines.append("  4 (nnzA + nnzQ full) + the three CSR value arrays and their unscaled copies 16 (2 nnzA + nnzQ full) + q, l, u 16 (n + 2m); setup %d = state and D, E" % z)
            lines.append("  vectors + 10 Ruiz iterations x (norms 16 nnzA, scaling 56 nnzA, vectors) + Q and cost scaling 36 nnzQ full.  Sum %d B -> %.1f GB/s = %.1f %% of %.0f TB/s;" % (
                g + z, (g + z) / kt * 1e-9, 100.0 * (g + z) / kt / HBM_BYTES_PER_S, HBM_BYTES_PER_S * 1e-12))
            lines.append("  the gather alone is %.1f %% of those bytes: the launch is the Ruiz iterations (each a handful of barriers on one workgroup per item), not a stream." % (100.0 * g / (g + z)))
            lines.append("resident_extra_bytes of the flag: %d (%.1f KB per item)" % (extra, extra / N / 1024.0))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
