#!/usr/bin/env python3
"""What do many right-hand sides per factorization save?  A fleet of C3 items (n = 120, m = 360), both scalings; per nrhs in 1, 8, 32, 120:

  multi     HIP-event time of ONE Fleet.adjoint_many_device call with nrhs right-hand sides (k_small_fleet_sens, gy = None, no matrix outputs)
  G = 1     the same call on a second fleet of the same items created with QPDO_AMD_FLEET_RHS_GROUP=1: its right-hand sides follow one
            another (step 1), where the first fleet carries rhs_group() of them at once (step 2) -- the step-1 / step-2 comparison
  singles   the same right-hand sides as nrhs Fleet.adjoint_device calls back to back (k_small_fleet_adjoint): the baseline, what the
            library offered for the same result before the multi call existed; the code that runs them is unchanged
  tangent   ONE Fleet.tangent_device call with nrhs perturbations of q

    python tools/fleet_sensitivity_latency.py [--count 4096] [--reps 20] [--reps-120 6] [--warmup 5] [--max-iter 300] [--out profiles/fleet_sensitivity_latency.txt]

The multi call and the single calls run in the same process, in alternating order (multi first in even rounds, singles first in odd ones),
after `warmup` untimed rounds; median (min ... max) of `reps` rounds, `reps-120` at nrhs = 120.  Every round asserts that the multi call's
dq, dl, du, status and residual equal the single calls' bit for bit.  The two claims are stated against the single-call path's own
min ... max spread; nothing else is asserted.  Last, unasserted: the error of the first-order prediction x + dx for a perturbed q against a
warm re-solve at that q on the items whose flags did not change, beside the re-solve's time.  No GPU: the tool fails."""
import argparse
import os
import sys

import numpy as np
import torch  # (before qpdo_amd loads its library: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402

NRHS = (1, 8, 32, 120)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def stat(ts):
    return float(np.median(ts)), min(ts), max(ts)


def same_bits(a, b):
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return bool(torch.equal(a, b))


def measure(count, scaling, reps, reps120, warmup, max_iter):
    probs = [problems.config_qp("C3", i) for i in range(count)]
    F = solver.Fleet(probs, adjoint=True, verbose=0, max_iter=max_iter, scaling=scaling)
    os.environ["QPDO_AMD_FLEET_RHS_GROUP"] = "1"           # (read at create: the same fleet with its right-hand sides one after another, step 1)
    try:
        F1 = solver.Fleet(probs, adjoint=True, verbose=0, max_iter=max_iter, scaling=scaling)
    finally:
        del os.environ["QPDO_AMD_FLEET_RHS_GROUP"]
    try:
        assert F1.rhs_group() == 1
        F1.solve()
        no, mo = F.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        dev = torch.device("cuda", F._device)
        rng = np.random.default_rng(1)
        cold = F.solve()
        solved = sum(r["info"]["status_val"] == 1 for r in cold)
        rows = []
        for R in NRHS:
            gx = torch.from_numpy(rng.standard_normal((R, N))).to(dev)
            tq = torch.from_numpy(rng.standard_normal((R, N))).to(dev)
            e = lambda *s, dt=torch.float64: torch.empty(s, dtype=dt, device=dev)
            mo_ = dict(dq=e(R, N), dl=e(R, M), du=e(R, M), active=e(M, dt=torch.int32), status=e(R, count, 3, dt=torch.int64), residual=e(R, count))
            m1 = {k: torch.empty_like(v) for k, v in mo_.items()}
            so = dict(dq=e(R, N), dl=e(R, M), du=e(R, M), status=e(R, count, 3, dt=torch.int64), residual=e(R, count))
            sact = e(M, dt=torch.int32)
            to = dict(dx=e(R, N), dy=e(R, M), active=e(M, dt=torch.int32), status=e(R, count, 3, dt=torch.int64), residual=e(R, count))
            souts = [dict({k: v[r] for k, v in so.items()}, active=sact) for r in range(R)]

            def multi():
                F.adjoint_many_device(gx, out=mo_)

            def multi1():
                F1.adjoint_many_device(gx, out=m1)

            def singles():
                for r in range(R):
                    F.adjoint_device(gx[r], out=souts[r])

            def tangent():
                F.tangent_device(tq=tq, out=to)

            n_rounds = reps120 if R == 120 else reps
            tm, ts, tt, t1 = [], [], [], []
            for k in range(warmup + n_rounds):
                for v in list(mo_.values()) + list(so.values()) + list(m1.values()):
                    v.fill_(-7) if v.dtype != torch.float64 else v.fill_(-7.5)
                first, second = (multi, singles) if k % 2 == 0 else (singles, multi)
                a, b = window(first), window(second)
                c = window(tangent)
                c1 = window(multi1)
                for key in so:
                    assert same_bits(m1[key], so[key]), "scaling %d nrhs %d round %d: %s differs between the one-after-another multi call and the single calls" % (scaling, R, k, key)
                    assert same_bits(mo_[key], so[key]), "scaling %d nrhs %d round %d: %s differs between the multi call and the single calls" % (scaling, R, k, key)
                if k >= warmup:
                    tm.append(a if first is multi else b); ts.append(b if first is multi else a); tt.append(c); t1.append(c1)
            codes = mo_["status"][:, :, 0]
            rows.append(dict(R=R, rounds=n_rounds, multi=stat(tm), singles=stat(ts), tangent=stat(tt), multi1=stat(t1), accepted=int((codes == 0).sum()), refused=int((codes == 1).sum()),
                             t_accepted=int((to["status"][:, :, 0] == 0).sum())))
        # ---- the first-order prediction against a re-solve (changes the fleet's state: last)
        q0 = torch.from_numpy(np.concatenate([p["q"] for p in probs])).to(dev)
        x0 = F.solve_device()["x"].clone()
        tq1 = 0.01 * torch.from_numpy(rng.standard_normal(N)).to(dev)
        d = F.tangent_device(tq=tq1)
        dx, f0, c0 = d["dx"].clone(), d["active"].clone(), d["status"][:, 0].clone()
        F.update_device(q=q0 + tq1)
        F.warm_start_last_device()
        box = {}
        t_resolve = window(lambda: box.update(o=F.solve_device()))
        x1, st1 = box["o"]["x"].clone(), box["o"]["status"][:, 0].clone()
        f1 = F.tangent_device(tq=tq1)["active"].clone()
        torch.cuda.synchronize()
        f0, f1, c0, st1 = f0.cpu().numpy(), f1.cpu().numpy(), c0.cpu().numpy(), st1.cpu().numpy()
        x0, x1, dx = x0.cpu().numpy(), x1.cpu().numpy(), dx.cpu().numpy()
        errs, moves, steps, kept = [], [], [], 0
        for i in range(count):
            sn, sm = slice(int(no[i]), int(no[i + 1])), slice(int(mo[i]), int(mo[i + 1]))
            if c0[i] == 0 and st1[i] == 1 and np.array_equal(f0[sm], f1[sm]):
                kept += 1
                errs.append(np.abs(x0[sn] + dx[sn] - x1[sn]).max()); moves.append(np.abs(x1[sn] - x0[sn]).max()); steps.append(np.abs(dx[sn]).max())
        pred = dict(kept=kept, err_med=float(np.median(errs)) if errs else float("nan"), err_max=float(np.max(errs)) if errs else float("nan"),
                    move_med=float(np.median(moves)) if moves else float("nan"), step_med=float(np.median(steps)) if steps else float("nan"),
                    step_max=float(np.max(steps)) if steps else float("nan"), resolve=t_resolve)
        return dict(scaling=scaling, count=count, solved=int(solved), rows=rows, pred=pred, G=F.rhs_group(), layout=F.factor_layout(),
                    scratch=F.sensitivity_stats()["scratch_bytes"])
    finally:
        F.close(); F1.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-120", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fleet_sensitivity_latency: no GPU visible; this measurement has no CPU form")
    f = lambda t: "%9.3f (%8.3f ... %8.3f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])
    lines = ["many right-hand sides per factorization: %d config_qp('C3', i) items (n = 120, m = 360), max_iter %d; HIP events on the caller's stream; median (min ... max) in ms "
             "of %d rounds (%d at nrhs = 120) after %d untimed ones; multi and singles alternate in order; equal bits asserted every round" % (
                 a.count, a.max_iter, a.reps, a.reps_120, a.warmup)]
    for scaling in (10, 0):
        r = measure(a.count, scaling, a.reps, a.reps_120, a.warmup, a.max_iter)
        lines.append("scaling %d: %d of %d items solved; layout of K %d; rhs_group G = %d; scratch_bytes %d" % (scaling, r["solved"], r["count"], r["layout"], r["G"], r["scratch"]))
        lines.append("%5s %6s | %-32s | %-32s | %-32s | %-32s | %13s | %s" % ("nrhs", "rounds", "one adjoint_multi_dev (G at once)", "the same, G = 1 (step 1)", "nrhs x adjoint_dev (baseline)",
                                                                                 "one tangent_dev", "singles/multi", "claim"))
        for w in r["rows"]:
            m, s = w["multi"], w["singles"]
            spread = s[2] - s[1]
            if w["R"] == 1:
                claim = "multi within the single call's spread: |%.3f - %.3f| = %.3f ms %s spread %.3f ms" % (
                    1e3 * m[0], 1e3 * s[0], 1e3 * abs(m[0] - s[0]), "<=" if abs(m[0] - s[0]) <= spread else ">", 1e3 * spread)
            else:
                claim = "multi not slower than the singles by more than their spread: %.3f %s %.3f + %.3f ms" % (
                    1e3 * m[0], "<=" if m[0] <= s[0] + spread else ">", 1e3 * s[0], 1e3 * spread)
            lines.append("%5d %6d | %s | %s | %s | %s | %13.2f | %s" % (w["R"], w["rounds"], f(m), f(w["multi1"]), f(s), f(w["tangent"]), s[0] / m[0], claim))
        p = r["pred"]
        lines.append("   prediction x + dx for q + tq (tq = 0.01 randn) against a warm re-solve at q + tq, %d items with unchanged flags: |x + dx - x_resolve|inf median %.3e, max %.3e "
                     "(|dx|inf median %.3e, max %.3e; the re-solve moved x by a median of %.3e); the re-solve launch took %.3f ms" % (
                         p["kept"], p["err_med"], p["err_max"], p["step_med"], p["step_max"], p["move_med"], 1e3 * p["resolve"]))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
