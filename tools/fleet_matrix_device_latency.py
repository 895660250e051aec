#!/usr/bin/env python3
"""What does the host boundary of the fleet's MATRIX call cost a caller whose Jacobians and Hessians live on the GPU?  One
real-time-iteration step over a fleet of C3-shaped QPs (n = 120, m = 360) -- new Q and A values for all items -> update q, l, u ->
warm_start_last -> solve -> x available to a following torch op -- measured twice:

  host    the value tensors and q, l, u are copied to the host, the values wrapped into per-item scipy matrices in the create-time pattern,
          Fleet.update_matrices / update / warm_start_last / solve (each uploads, launches and waits), x uploaded again as one tensor
  device  the same tensors handed to Fleet.update_matrices_device / update_device / warm_start_last_device / solve_device on torch's
          current stream

    python tools/fleet_matrix_device_latency.py [--counts 256,4096] [--steps 12] [--warmup 3] [--max-iter 300] [--out profiles/fleet_matrix_device_latency.txt]

Both paths get the same data every step and must return the same x bits (asserted).  A step's time is the host wall clock from the first
call to the return of a final torch.cuda.synchronize() behind a torch op that reads x; the inputs are complete on the device before the
window opens.  Which path goes first alternates per step; `warmup` steps run untimed; the figure is the median over `steps`.  No speed-up
is fixed in advance: the claim the table supports or refutes is "the device step is not slower than the host step", the margin being the
host step's own min ... max spread in the same run.  No GPU: the tool fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch  # (before qpdo_amd loads its library: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402


def measure(count, steps, warmup, max_iter):
    probs = [problems.config_qp("C3", i) for i in range(count)]
    st = dict(verbose=0, max_iter=max_iter)
    H, D = solver.Fleet(probs, matrix_updates=True, **st), solver.Fleet(probs, matrix_updates=True, **st)
    no, mo = D.packed_layout()
    qoff, aoff = D.packed_matrix_layout()
    # the create-time patterns (sorted CSC, as the create path stores them) and their values in the packed layout
    Qs, As = [sp.csc_matrix(p["Q"]) for p in probs], [sp.csc_matrix(p["A"]) for p in probs]
    for M in Qs + As:
        M.sort_indices()
    qv, av, _ = D.pack_matrix_values(Q=Qs, A=As)
    Q0, A0 = torch.from_numpy(qv).cuda(), torch.from_numpy(av).cuda()
    q0 = torch.from_numpy(np.concatenate([p["q"] for p in probs])).cuda()
    l0 = torch.from_numpy(np.concatenate([np.clip(p["l"], -1e20, 1e20) for p in probs])).cuda()
    u0 = torch.from_numpy(np.concatenate([np.clip(p["u"], -1e20, 1e20) for p in probs])).cuda()
    iq = torch.arange(q0.numel(), device=q0.device, dtype=torch.float64)
    ia = torch.arange(A0.numel(), device=q0.device, dtype=torch.float64)
    free = l0 < u0                                       # equality rows stay equalities
    H.solve(results=False); D.solve_device()
    th, td, passes = [], [], []

    def host_step(Qx, Ax, q, l, u):
        t0 = time.perf_counter()
        Qh, Ah, qh, lh, uh = Qx.cpu().numpy(), Ax.cpu().numpy(), q.cpu().numpy(), l.cpu().numpy(), u.cpu().numpy()
        H.update_matrices(Q=[sp.csc_matrix((Qh[qoff[i]:qoff[i + 1]], Qs[i].indices, Qs[i].indptr), shape=Qs[i].shape) for i in range(count)],
                          A=[sp.csc_matrix((Ah[aoff[i]:aoff[i + 1]], As[i].indices, As[i].indptr), shape=As[i].shape) for i in range(count)])
        H.update(q=[qh[no[i]:no[i + 1]] for i in range(count)], l=[lh[mo[i]:mo[i + 1]] for i in range(count)],
                 u=[uh[mo[i]:mo[i + 1]] for i in range(count)])
        H.warm_start_last()
        H.solve(results=False)
        x = torch.from_numpy(np.concatenate([o[0] for o in H.outs])).cuda()
        s = x.sum()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x, s

    def device_step(Qx, Ax, q, l, u):
        t0 = time.perf_counter()
        D.update_matrices_device(Qx, Ax)
        D.update_device(q, l, u)
        D.warm_start_last_device()
        x = D.solve_device()["x"]
        s = x.sum()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x, s

    for k in range(1, warmup + steps + 1):
        ph = 0.37 * k
        Qx = Q0 * (1.0 + 0.05 * float(np.sin(ph)))       # (one positive factor: Q stays symmetric in bits and convex)
        Ax = A0 * (1.0 + 0.02 * torch.sin(ph + 0.1 * ia))
        q = q0 * (1.0 + 0.05 * torch.sin(ph + 0.1 * iq))
        w = 0.02 * (1.0 + float(np.sin(ph)))
        l, u = torch.where(free, l0 - w, l0), torch.where(free, u0 + w, u0)
        torch.cuda.synchronize()                         # the inputs are complete before either window opens
        if k % 2:
            (a, xh, _), (b, xd, _) = host_step(Qx, Ax, q, l, u), device_step(Qx, Ax, q, l, u)
        else:
            (b, xd, _), (a, xh, _) = device_step(Qx, Ax, q, l, u), host_step(Qx, Ax, q, l, u)
        assert np.array_equal(xh.cpu().numpy().view(np.int64), xd.cpu().numpy().view(np.int64)), "step %d: the two paths returned different x bits" % k
        if k > warmup:
            th.append(a); td.append(b); passes.append(int(H.info_view()["iterations"].sum()))
    host_matrix_kernel = H.matrix_stats()["last_kernel_seconds"]
    D.sync()
    H.close(); D.close()
    return dict(count=count, host=float(np.median(th)), device=float(np.median(td)), host_min=min(th), host_max=max(th), dev_min=min(td), dev_max=max(td),
                matrix_kernel=host_matrix_kernel, passes=int(np.median(passes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="256,4096")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="label for the table (default: git rev-parse of this tree)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fleet_matrix_device_latency: no GPU visible; this measurement has no CPU form")
    commit = a.commit
    try:
        if commit is None:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), text=True,
                                             stderr=subprocess.DEVNULL).strip() + " (+ working tree)"
    except Exception:
        commit = "unknown"
    lines = ["one real-time-iteration step (new Q and A values for all items -> update q, l, u -> warm_start_last -> solve -> x read by a torch op) over "
             "config_qp('C3', i) items, max_iter %d; commit %s" % (a.max_iter, commit),
             "inputs are torch tensors on the GPU; host = copy down, per-item scipy matrices, Fleet.update_matrices / update / warm_start_last / solve, x uploaded again; "
             "device = Fleet.*_device on torch's stream",
             "median of %d steps after %d untimed ones; ms, host wall clock closed by torch.cuda.synchronize(); the order of the two paths alternates per step; same x bits (asserted)" % (a.steps, a.warmup),
             "%-6s | %10s %10s %10s | %10s %10s %10s | %8s | %13s %9s" % ("count", "host", "min", "max", "device", "min", "max", "host/dev", "matrix.kernel", "passes")]
    verdicts = []
    for count in [int(c) for c in a.counts.split(",")]:
        r = measure(count, a.steps, a.warmup, a.max_iter)
        lines.append("%-6d | %10.3f %10.3f %10.3f | %10.3f %10.3f %10.3f | %8.2f | %13.3f %9d" % (
            r["count"], 1e3 * r["host"], 1e3 * r["host_min"], 1e3 * r["host_max"], 1e3 * r["device"], 1e3 * r["dev_min"], 1e3 * r["dev_max"],
            r["host"] / r["device"], 1e3 * r["matrix_kernel"], r["passes"]))
        slower = r["device"] > r["host"] + (r["host_max"] - r["host_min"])
        verdicts.append("%d items: the device step (median %.3f ms) is %s the host step (median %.3f ms, min ... max spread %.3f ms)" % (
            r["count"], 1e3 * r["device"], "SLOWER than" if slower else "not slower than", 1e3 * r["host"], 1e3 * (r["host_max"] - r["host_min"])))
    lines.append("matrix.kernel: HIP-event duration of k_small_fleet_matrices in the last HOST step (the device step runs the same kernel behind its gather)")
    lines.append("; ".join(verdicts) + ".")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
