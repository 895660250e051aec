#!/usr/bin/env python3
"""What does the host boundary of a fleet cost a caller whose data lives on the GPU?  One closed-loop control step over a fleet of
C3-shaped QPs (n = 120, m = 360) -- update q, l, u -> warm_start_last -> solve -> x available to a following torch op -- measured twice:

  host    q, l, u are torch tensors on the GPU: copied to the host, split into per-item numpy arrays, Fleet.update / warm_start_last /
          solve (each uploads, launches and waits), x gathered from the per-item outputs and uploaded again as one tensor
  device  the same tensors handed to Fleet.update_device / warm_start_last_device / solve_device on torch's current stream

    python tools/fleet_device_latency.py [--counts 256,4096] [--steps 12] [--warmup 3] [--max-iter 300] [--out profiles/fleet_device_io_latency.txt]

Both paths get the same data every step and must return the same x bits (asserted after the timed window).  A step's time is the host
wall clock from the first call to the return of a final torch.cuda.synchronize() behind a torch op that reads x; the inputs are complete
on the device before the window opens.  Which path goes first alternates per step; `warmup` steps run untimed; the figure is the median
over `steps`.  The host calls are unchanged by the device entry points, so the host figure is the baseline.  No GPU: the tool fails."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch  # (before qpdo_amd loads its library: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402


def measure(count, steps, warmup, max_iter):
    probs = [problems.config_qp("C3", i) for i in range(count)]
    st = dict(verbose=0, max_iter=max_iter)
    H, D = solver.Fleet(probs, **st), solver.Fleet(probs, **st)
    no, mo = D.packed_layout()
    q0 = torch.from_numpy(np.concatenate([p["q"] for p in probs])).cuda()
    l0 = torch.from_numpy(np.concatenate([np.clip(p["l"], -1e20, 1e20) for p in probs])).cuda()
    u0 = torch.from_numpy(np.concatenate([np.clip(p["u"], -1e20, 1e20) for p in probs])).cuda()
    iq = torch.arange(q0.numel(), device=q0.device, dtype=torch.float64)
    free = l0 < u0                                       # equality rows stay equalities
    H.solve(results=False); D.solve_device()
    th, td, passes = [], [], []

    def host_step(q, l, u):
        t0 = time.perf_counter()
        qh, lh, uh = q.cpu().numpy(), l.cpu().numpy(), u.cpu().numpy()
        H.update(q=[qh[no[i]:no[i + 1]] for i in range(count)], l=[lh[mo[i]:mo[i + 1]] for i in range(count)],
                 u=[uh[mo[i]:mo[i + 1]] for i in range(count)])
        H.warm_start_last()
        H.solve(results=False)
        x = torch.from_numpy(np.concatenate([o[0] for o in H.outs])).cuda()
        s = x.sum()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x, s

    def device_step(q, l, u):
        t0 = time.perf_counter()
        D.update_device(q, l, u)
        D.warm_start_last_device()
        x = D.solve_device()["x"]
        s = x.sum()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x, s

    for k in range(1, warmup + steps + 1):
        ph = 0.37 * k
        q = q0 * (1.0 + 0.05 * torch.sin(ph + 0.1 * iq))
        w = 0.02 * (1.0 + float(np.sin(ph)))
        l, u = torch.where(free, l0 - w, l0), torch.where(free, u0 + w, u0)
        torch.cuda.synchronize()                         # the inputs are complete before either window opens
        if k % 2:
            (a, xh, _), (b, xd, _) = host_step(q, l, u), device_step(q, l, u)
        else:
            (b, xd, _), (a, xh, _) = device_step(q, l, u), host_step(q, l, u)
        assert np.array_equal(xh.cpu().numpy().view(np.int64), xd.cpu().numpy().view(np.int64)), "step %d: the two paths returned different x bits" % k
        if k > warmup:
            th.append(a); td.append(b); passes.append(int(H.info_view()["iterations"].sum()))
    D.sync()                                             # (refreshes last_kernel_seconds from the last device solve)
    kernel = D.stats()["last_kernel_seconds"]
    H.close(); D.close()
    return dict(count=count, host=float(np.median(th)), device=float(np.median(td)), host_min=min(th), host_max=max(th), dev_min=min(td), dev_max=max(td),
                kernel=kernel, passes=int(np.median(passes)))


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
        sys.exit("fleet_device_latency: no GPU visible; this measurement has no CPU form")
    commit = a.commit
    try:
        if commit is None:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), text=True,
                                             stderr=subprocess.DEVNULL).strip() + " (+ working tree)"
    except Exception:
        commit = "unknown"
    lines = ["one control step (update q, l, u -> warm_start_last -> solve -> x read by a torch op) over config_qp('C3', i) items, max_iter %d; commit %s" % (a.max_iter, commit),
             "inputs are torch tensors on the GPU; host = copy down, Fleet.update / warm_start_last / solve, x uploaded again; device = Fleet.*_device on torch's stream",
             "median of %d steps after %d untimed ones; ms, host wall clock closed by torch.cuda.synchronize(); the order of the two paths alternates per step; same x bits (asserted)" % (a.steps, a.warmup),
             "%-6s | %10s %10s %10s | %10s %10s %10s | %8s | %10s %9s" % ("count", "host", "min", "max", "device", "min", "max", "host/dev", "dev.kernel", "passes")]
    for count in [int(c) for c in a.counts.split(",")]:
        r = measure(count, a.steps, a.warmup, a.max_iter)
        lines.append("%-6d | %10.3f %10.3f %10.3f | %10.3f %10.3f %10.3f | %8.2f | %10.3f %9d" % (
            r["count"], 1e3 * r["host"], 1e3 * r["host_min"], 1e3 * r["host_max"], 1e3 * r["device"], 1e3 * r["dev_min"], 1e3 * r["dev_max"],
            r["host"] / r["device"], 1e3 * r["kernel"], r["passes"]))
    lines.append("dev.kernel: HIP-event duration of the last device step's solve launch; what remains of a device step is the gather, update, warm-start and scatter launches")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
