"""Wall times of qpdo_amd_adjoint / qpdo_amd_tangent on the two band kinds the calls take since the wide-band and coupled routes were added
(DESIGN.md 3.7), through solver.QPDO, in one process:

    python tools/workspace_band_sens_latency.py [--out profiles/workspace_band_sens_latency.txt] [--configs wide,coupled] [--n 20000]

wide:    problems.banded_random_qp(1, n, 256) under QPDO_LINSOLVE=band (half-bandwidth 256: the tiled solver of dev/band_wide.inc);
coupled: tests/band_coupled_ref.coupled_banded_qp(11, n, 5, 8) under QPDO_LINSOLVE=band, QPDO_BAND_COUPLING=64; the free problem behind the
         coupling rows' bounds is solved on the device's default path (solve=, as tools/band_coupled_latency.py does).
Per configuration THREE workspaces on the one problem: the default one, one set up with QPDO_AMD_RHS_GROUP=1 (the right-hand sides one after
the other) and one set up with QPDO_LINSOLVE=dense -- what the refusal the two kinds used to get told the caller to do; it is the baseline.
Every call ends in a stream synchronise, so the host clock around it is the call's time.  Per line: 3 untimed calls, then the median and
min .. max of 12, the workspaces of a line ALTERNATING call by call: the adjoint (gx, gy), the adjoint with gy = None (recorded only: a
random gy on every active row is not a consistent right-hand side where active rows are dependent, and such a right-hand side runs to
max_sweeps on every route) and the tq-only tangent, at nrhs = 8 and at nrhs = 1.
Condition 1 (exit status 1 on a miss, no margin): for both configurations and both calls the median of the default workspace's nrhs = 8
call is below the median of the QPDO_AMD_RHS_GROUP=1 workspace's nrhs = 8 call of the same alternating run.
Recorded without a threshold: band route against dense route in time and in memory (QPDOAmdGroupStats.scratch_bytes + the adjoint's and the
tangent's scratch_bytes + the factor's arrays, from the factor's geometry), the sweep counts, the cost of a further right-hand side inside
a group ((nrhs 8 - nrhs 1) / 7), and the factorization's share: a call with gx = 0, which is accepted at sweep 0 and so runs everything but
solves -- the keep / restore, the classification, the factorization and one residual."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from qpdo_amd import problems, solver  # noqa: E402

WARM, REPS = 3, 12
KINDS = ("adjoint", "adjoint gx", "tangent")          # the adjoint with (gx, gy) and with gy = None (a loss of x alone), the tq-only tangent
SWITCHES = ("QPDO_AMD_RHS_GROUP", "QPDO_LINSOLVE", "QPDO_BAND_COUPLING", "QPDO_BAND_ORDER")


def timed(*calls):
    """the calls alternate, one after the other per repetition; per call (median, min, max)"""
    for _ in range(WARM):
        for c in calls:
            c()
    t = [[] for _ in calls]
    for _ in range(REPS):
        for i, c in enumerate(calls):
            t0 = time.perf_counter()
            c()
            t[i].append(time.perf_counter() - t0)
    return [(float(np.median(v)), float(min(v)), float(max(v))) for v in t]


def fmt(t):
    return "%9.3f ms  (%.3f .. %.3f)" % (1e3 * t[0], 1e3 * t[1], 1e3 * t[2])


def setup(p, **env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    qp = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p["Qstype"], c=p.get("c", 0.0), verbose=0, max_iter=2000)
    for k in SWITCHES:
        os.environ.pop(k, None)
    t0 = time.perf_counter()
    r = qp.solve()
    dt = time.perf_counter() - t0
    assert r["info"]["status_val"] == 1, r["info"]
    return qp, dt


def default_path_x(p):
    for k in SWITCHES:
        os.environ.pop(k, None)
    res = solver.solve_problem(p, verbose=0)
    if res["info"]["status_val"] != 1:
        raise RuntimeError("instance generation: the free problem ended with status %d" % res["info"]["status_val"])
    return res["x"]


def factor_bytes(qp):
    """the factor's arrays as the host allocates them (host_band.inc band_alloc / band_wide_alloc, host_dense.inc), from the geometry"""
    st, g = qp.stats(), qp.factor_geometry()
    if st["linsolve"] == 1:
        return 8 * (g["ld"] * g["ld"] + g["ld"] + 2 * g["nb"] * 4096)
    npad, b = g["np"], g["b"]
    if b > 127:
        nbc, w = npad // 64, (b + 63) // 64
        return 8 * ((nbc * (w + 1) + 3 * nbc) * 4096 + 2 * npad)
    r = st["coupled_rows"]
    return 8 * (2 * npad * (b + 1) + npad + (3 * npad * r + 2 * 64 * 64 + 64 + npad + 2 * qp.m if r else 0))


def sweeps_of(o):
    sw = np.atleast_2d(o["status"])[:, 1]
    return "%d" % sw[0] if len(sw) == 1 else "%d .. %d" % (sw.min(), sw.max())


def run(name, p, env, out):
    n, m = p["n"], p["m"]
    made = [("default", setup(p, QPDO_LINSOLVE="band", **env)), ("RHS_GROUP=1", setup(p, QPDO_LINSOLVE="band", QPDO_AMD_RHS_GROUP="1", **env)),
            ("dense route", setup(p, QPDO_LINSOLVE="dense"))]
    ws = [(w, q) for w, (q, _) in made]
    ok = True
    lines = []
    try:
        rng = np.random.default_rng(1)
        gx, gy, tq = rng.standard_normal((8, n)), rng.standard_normal((8, m)), rng.standard_normal((8, n))
        lines.append("%s: n = %d, m = %d; %s" % (name, n, m, "; ".join("%s: linsolve %d, b = %d, coupled rows %d, group size %d, qpdo_solve %.3f s"
                     % (w, q.stats()["linsolve"], q.factor_geometry()["b"], q.stats()["coupled_rows"], q.rhs_group(), dt) for w, (q, dt) in made)))
        med = {}
        for R in (8, 1):
            for kind in KINDS:
                def call_on(q):
                    if kind == "adjoint":
                        return (lambda: q.adjoint(gx[0], gy[0])) if R == 1 else (lambda: q.adjoint(gx[:R], gy[:R]))
                    if kind == "adjoint gx":
                        return (lambda: q.adjoint(gx[0], None)) if R == 1 else (lambda: q.adjoint(gx[:R], None))
                    return (lambda: q.tangent(tq=tq[0])) if R == 1 else (lambda: q.tangent(tq=tq[:R]))
                info = [call_on(q)() for _, q in ws]
                assert all((np.atleast_2d(o["status"])[:, 0] != 3).all() for o in info), (name, kind, R)
                times = timed(*[call_on(q) for _, q in ws])
                for (w, _), t, o in zip(ws, times, info):
                    med[(kind, R, w)] = t[0]
                    lines.append("  %-10s nrhs = %-2d  %-12s %s   sweeps %s, accepted %d of %d"
                                 % (kind, R, w, fmt(t), sweeps_of(o), int((np.atleast_2d(o["status"])[:, 0] == 0).sum()), R))
        zero = timed(*[(lambda q=q: q.adjoint(np.zeros(n), None)) for _, q in ws])
        for (w, _), t in zip(ws, zero):
            med[("zero", 1, w)] = t[0]
            lines.append("  adjoint    gx = 0     %-12s %s   (accepted at sweep 0: the factorization and everything else but solves)" % (w, fmt(t)))
        for kind in ("adjoint", "tangent"):
            a, b = med[(kind, 8, "default")], med[(kind, 8, "RHS_GROUP=1")]
            hit = a < b
            ok = ok and hit
            lines.append("  condition 1, %s: median(default, nrhs 8) / median(RHS_GROUP=1, nrhs 8) = %.3f < 1: %s" % (kind, a / b, "PASS" if hit else "FAIL"))
        for kind in KINDS:
            for w, _ in ws:
                t8, t1 = med[(kind, 8, w)], med[(kind, 1, w)]
                lines.append("  %-10s %-12s a further right-hand side %.3f ms ((nrhs 8 - nrhs 1) / 7); the gx = 0 call is %.0f %% of the nrhs = 1 call, %.0f %% of nrhs = 8"
                             % (kind, w, 1e3 * (t8 - t1) / 7, 100 * med[("zero", 1, w)] / t1, 100 * med[("zero", 1, w)] / t8))
            lines.append("  %-10s band route / dense route: nrhs 1 %.3f, nrhs 8 %.3f" % (kind, med[(kind, 1, "default")] / med[(kind, 1, "dense route")],
                                                                                        med[(kind, 8, "default")] / med[(kind, 8, "dense route")]))
        for w, q in ws:
            sb = q.group_stats()["scratch_bytes"] + q.adjoint_stats()["scratch_bytes"] + q.tangent_stats()["scratch_bytes"]
            lines.append("  memory %-12s scratch_bytes (group + adjoint + tangent) %.1f MB, factor %.1f MB" % (w, sb * 1e-6, factor_bytes(q) * 1e-6))
    finally:
        for _, q in ws:
            q.delete()
    for ln in lines:
        print(ln, flush=True)
        out.write(ln + "\n")
    out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "workspace_band_sens_latency.txt"))
    ap.add_argument("--configs", default="wide,coupled")
    ap.add_argument("--n", type=int, default=20000)
    a = ap.parse_args()
    import band_coupled_ref as bref

    make = {"wide": (lambda: problems.banded_random_qp(1, a.n, 256), {}),
            "coupled": (lambda: dict(bref.coupled_banded_qp(11, a.n, 5, 8, solve=default_path_x), Qstype=-1), {"QPDO_BAND_COUPLING": "64"})}
    with open(a.out, "w") as out:
        out.write("qpdo_amd_adjoint / qpdo_amd_tangent on a wide-band and on a coupled band workspace, beside QPDO_AMD_RHS_GROUP=1 and beside the dense "
                  "route, wall times in one process: %d untimed calls, then median (min .. max) of %d, the workspaces alternating call by call\n" % (WARM, REPS))
        ok = [run(name, make[name][0](), make[name][1], out) for name in a.configs.split(",")]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
