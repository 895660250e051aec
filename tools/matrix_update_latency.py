"""Latency of qpdo_amd_update_matrices against a fresh qpdo_cleanup + qpdo_setup, and of one re-solve step of an SQP-like loop both ways.

    python tools/matrix_update_latency.py [--configs C3,C1,n1000,n4000,C2] [--reps 7] [--steps 5]
    python tools/matrix_update_latency.py --kernel-only C2 --reps 20      (for rocprofv3 --kernel-trace --stats: updates only)

Per configuration: the median wall time of update_matrices(Q, A) (1 % value perturbation) and of cleanup + setup on the same data (the
Python front end included; c_*_ms: the C calls alone, as info->setup_time records them); then
`steps` SQP-like steps (1 % perturbation, warm start from the previous solution, solve) through update_matrices and through a fresh
setup.  The algorithmic bytes of k_update_values (one launch: copy of A's values into CSR(A'), gather into CSR(A) through the 4-byte
map, gather of the stored Q triangle into the full storage) are printed for the kernel-time line of the profile.  One JSON line per
configuration."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qpdo_amd import problems, solver  # noqa: E402

CONFIGS = {
    "C3": lambda: problems.config_qp("C3"),
    "C1": lambda: problems.config_qp("C1"),
    "n1000": lambda: problems.random_qp(31, 1000, 2000, 0.01, 0),
    "n4000": lambda: problems.random_qp(32, 4000, 8000, 0.005, 0),
    "C2": lambda: problems.config_qp("C2"),
    "C4": lambda: problems.config_qp("C4"),
}


def perturb(M, rng):
    M = sp.csc_matrix(M, copy=True)
    M.data = M.data * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, len(M.data)))
    return M


def perturb_Q(Qf, rng):
    Qf = sp.csc_matrix(Qf, copy=True)
    s = 1.0 + 0.01 * rng.uniform(-1.0, 1.0, Qf.shape[0])
    cols = np.repeat(np.arange(Qf.shape[1]), np.diff(Qf.indptr))
    Qf.data = Qf.data * s[Qf.indices] * s[cols]
    return sp.tril(Qf).tocsc()


def kernel_bytes(p):
    """algorithmic bytes of one k_update_values launch on a scaled workspace (raw copies kept): A: read raw (8) + write At (8) + read map
    (4) + gathered read (8) + write Ar (8) per entry; Q (stored triangle, stype -1): read map (4) + gathered read (8) + write raw (8) +
    write Qf (8) per entry of the full storage"""
    nA = p["A"].nnz
    nQf = problems.full_Q(p).nnz
    return 36 * nA + 28 * nQf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C1,n1000,n4000,C2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-only", default=None)
    a = ap.parse_args()
    st = dict(verbose=0)
    if a.kernel_only:
        p = CONFIGS[a.kernel_only]()
        rng = np.random.default_rng(0)
        Qf = problems.full_Q(p)
        w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], **st)
        mats = [(perturb_Q(Qf, rng), perturb(p["A"], rng)) for _ in range(2)]
        for k in range(a.reps):
            w.update_matrices(Q=mats[k % 2][0], A=mats[k % 2][1])
        w.delete()
        print(json.dumps(dict(config=a.kernel_only, updates=a.reps, nnzA=int(p["A"].nnz), nnzQf=int(Qf.nnz), kernel_alg_bytes=kernel_bytes(p))))
        return
    for name in a.configs.split(","):
        p = CONFIGS[name]()
        rng = np.random.default_rng(1)
        Qf = problems.full_Q(p)
        Ql, A = p["Q"], p["A"]
        w = solver.QPDO().setup(Ql, p["q"], A, p["l"], p["u"], **st)
        r = w.solve()
        mats = [(perturb_Q(Qf, rng), perturb(A, rng)) for _ in range(2)]
        t_upd, t_setup, c_upd, c_setup = [], [], [], []
        for k in range(a.reps):
            Qn, An = mats[k % 2]
            t0 = time.perf_counter(); w.update_matrices(Q=Qn, A=An); t_upd.append(time.perf_counter() - t0)
            c_upd.append(w.info()["setup_time"])                  # the C call alone (qpdo_amd_update_matrices)
            t0 = time.perf_counter()
            w2 = solver.QPDO().setup(Qn, p["q"], An, p["l"], p["u"], **st)
            c_setup.append(w2.info()["setup_time"])               # qpdo_setup alone
            w2.delete()
            t_setup.append(time.perf_counter() - t0)
        # SQP-like loop: perturb, re-solve warm-started, both ways (each way from the same starting point and the same sequence)
        seq = []
        Qc, Ac = Qf, A
        for _ in range(a.steps):
            Qc = sp.csc_matrix(Qc, copy=True)
            s = 1.0 + 0.01 * rng.uniform(-1.0, 1.0, Qc.shape[0])
            cols = np.repeat(np.arange(Qc.shape[1]), np.diff(Qc.indptr))
            Qc.data = Qc.data * s[Qc.indices] * s[cols]
            Ac = perturb(Ac, rng)
            seq.append((sp.tril(Qc).tocsc(), Ac))
        step_upd, step_setup, iters = [], [], []
        x, y = r["x"], r["y"]
        for Qn, An in seq:
            t0 = time.perf_counter()
            w.update_matrices(Q=Qn, A=An); w.warm_start(x, y); rr = w.solve()
            step_upd.append(time.perf_counter() - t0)
            x, y = rr["x"], rr["y"]; iters.append(int(rr["info"]["iterations"]))
        w.delete()
        x, y = r["x"], r["y"]
        ws = None
        for Qn, An in seq:
            t0 = time.perf_counter()
            if ws is not None:
                ws.delete()
            ws = solver.QPDO().setup(Qn, p["q"], An, p["l"], p["u"], **st); ws.warm_start(x, y); rr = ws.solve()
            step_setup.append(time.perf_counter() - t0)
            x, y = rr["x"], rr["y"]
        ws.delete()
        med = lambda v: float(np.median(v)) * 1e3  # noqa: E731
        print(json.dumps(dict(config=name, n=int(p["n"]), m=int(p["m"]), nnzA=int(A.nnz), nnzQf=int(Qf.nnz),
                              update_ms=med(t_upd), cleanup_setup_ms=med(t_setup), ratio=med(t_upd) / med(t_setup),
                              c_update_ms=med(c_upd), c_setup_ms=med(c_setup),
                              sqp_step_update_ms=med(step_upd), sqp_step_setup_ms=med(step_setup), sqp_iters=iters,
                              kernel_alg_bytes=kernel_bytes(p))), flush=True)


if __name__ == "__main__":
    main()
