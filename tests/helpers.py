import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "oracle_golden.json")

# stated fp64 tolerances of the parity tests (BASELINE.json north_star: iteration count and status
# bit-identical, iterates and KKT residuals within a stated fp64 tolerance)
ITERATE_RTOL = 1e-9      # |x - x_ref|inf <= ITERATE_RTOL * max(1, |x_ref|inf)   (dense LDL' solver)
ITERATE_RTOL_PCG = 1e-8  # same bound for the Jacobi-PCG solver: its stopping rule is a relative residual of 1e-12 on
                         # systems whose condition number reaches 1e12 late in a solve (weights 1/mu up to 1e9)
KKT_ATOL = 1e-10         # |KKT residual - reference KKT residual| <= KKT_ATOL
# per-pass trace (one record per loop pass of qpdo_solve, reference src/qpdo.c:343-449), HIP path vs oracle.  The
# bounds are set one order of magnitude above the largest deviation MEASURED on the MI355X over the golden cases, the
# random instances of test_gpu_parity.py and the production-size fixtures (tools/trace_dev.py, round 2): late in a solve
# the Newton matrix has weights 1/mu up to 1e9 against sigma = 1e-7, and both the direction and the breakpoint root
# inherit eps * kappa.
TAU_RTOL = 1e-8          # |tau - tau_ref| <= TAU_RTOL * max(1, |tau_ref|)   dense LDL' (measured max 1.4e-9: full-size C2, pass 44)
TAU_RTOL_PCG = 1e-7      # PCG to a 1e-12 relative residual                  (measured max 1.1e-8 over everything but the case below)
TAU_RTOL_PCG_C4_FULL = 3e-7  # the complete C4 record only: measured 5.7e-8 on ONE late pass (weights 1/mu up to 1e9 against sigma = 1e-7:
                         # kappa(K) > 1e12, the step length inherits eps * kappa from either implementation's direction); 5x that, so that a
                         # compiler or clock change cannot turn the headline fixture red for no algorithmic reason.  Every other pass of that
                         # record, and every other fixture, stays on TAU_RTOL_PCG.
NORM_RTOL = 1e-8         # the four residual norms of a pass: |v - v_ref| <= NORM_RTOL * |v_ref| + NORM_ATOL
NORM_RTOL_PCG = 1e-6
NORM_ATOL = 1e-9         # a residual is a difference of O(1..100) quantities, its error is absolute (measured max 2.7e-10)
NORM_ATOL_PCG = 1e-8     # (measured max 4.5e-9, reset_newton_iter=3 / inner_max_iter=6 instance)
TAU_NOISE_FLOOR = 1e-13  # a Newton pass that starts with both inner residual norms below this is already inner-optimal to
                         # rounding: its direction is rounding noise and so is the step length (seen on the 2-variable KATs,
                         # pass 1); tau is not compared there, everything else is


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def golden_problem(spec):
    from qpdo_amd import problems
    if "kat" in spec:
        return problems.infeasibility_kat(spec["kat"])
    if "cfg" in spec:
        return problems.config_qp(spec["cfg"], spec["index"])
    if "banded" in spec:
        seed, n, kw = spec["banded"]
        return problems.banded_qp(seed, n, **kw)
    seed, n, m, dens, neq = spec["rand"]
    return problems.random_qp(seed, n, m, dens, neq)


def close_vec(a, b, rtol=ITERATE_RTOL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if np.isnan(b).all():
        return bool(np.isnan(a).all())
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    return bool(np.abs(a - b).max() <= rtol * scale) if b.size else True


def assert_same_trace(got, ref, pcg=False, tau_rtol=None, norm_rtol=None, norm_atol=None):
    """Per-pass comparison of the HIP path's trace with the oracle's (lists of dicts with the TraceRec fields of
    oracle/qpdo_oracle.c:92-100 = QPDOAmdTraceRec of include/qpdo_amd_ext.h).  Integer fields (pass kind, active-set
    size, rows entering / leaving, factor branch) must be IDENTICAL; sigma and eps_in are products of settings
    constants and must be identical bit for bit; tau and the four residual norms within the stated tolerances."""
    tau_rtol = tau_rtol if tau_rtol is not None else (TAU_RTOL_PCG if pcg else TAU_RTOL)
    norm_rtol = norm_rtol if norm_rtol is not None else (NORM_RTOL_PCG if pcg else NORM_RTOL)
    norm_atol = norm_atol if norm_atol is not None else (NORM_ATOL_PCG if pcg else NORM_ATOL)
    assert len(got) == len(ref), (len(got), len(ref))
    for k, (g, r) in enumerate(zip(got, ref)):
        for f in ("kind", "n_active", "n_enter", "n_leave", "factor_branch"):
            assert int(g[f]) == int(r[f]), (k, f, g[f], r[f])
        for f in ("sigma", "eps_in"):
            assert float(g[f]) == float(r[f]), (k, f, g[f], r[f])
        if int(r["kind"]) == 0 and max(r["res_prim_in"], r["res_dual_in"]) > TAU_NOISE_FLOOR:
            assert abs(g["tau"] - r["tau"]) <= tau_rtol * max(1.0, abs(r["tau"])), (k, "tau", g["tau"], r["tau"])
        for f in ("res_prim", "res_dual", "res_prim_in", "res_dual_in"):
            assert abs(g[f] - r[f]) <= norm_rtol * abs(r[f]) + norm_atol, (k, f, g[f], r[f])


def trace_from_npz(z):
    """list of per-pass dicts from a tests/golden/big_*.npz fixture"""
    fields = [k[3:] for k in z.files if k.startswith("tr_")]
    n = len(z["tr_kind"])
    return [{f: z["tr_" + f][i] for f in fields} for i in range(n)]


def same_trace_counts(got, ref):
    """integer part of the per-pass trace only (pass kind, active-set size, rows entering / leaving, factor branch)"""
    return len(got) == len(ref) and all(
        int(g[f]) == int(r[f]) for g, r in zip(got, ref) for f in ("kind", "n_active", "n_enter", "n_leave", "factor_branch"))


# ---- runs that crawl to max_iter (tests/test_gpu_sweep.py) ------------------------------------------------------------------------------
# A run the oracle itself ends at max_iter (-5) may differ from the device's in the per-pass integers after ~100-250 passes.  Round 4
# read those as rows sitting exactly on a bound; measured (tools/sweep_knife_edges.py, profiles/r05_sweep_knife_edges.txt: the 10 + 13
# such runs among 720 instances, dense and PCG) that is true of about half of them (margins min(|w - l|, |u - w|) / max(1, |w|) of 0 to
# 1e-8 at the first differing pass), while on the others -- inner_max_iter of 2-4 passes, mu_min = 1e-12 or no proximal term -- the two
# iterates have separated by 1e-2 .. 1e3 by then although every integer of the first 80-260 passes still agreed: the iteration is not
# contracting there and amplifies rounding differences, and no margin bound explains the eventual flip.  What CAN be asserted for such a
# run, and is (device_active_count_consistent): at the first pass whose integers differ, the device's own active-set count is the count of
# rows with w <= l or w >= u in the w the device itself computed for that pass (reference src/newton.c:96-107) -- the device's integers
# follow from its iterate; an active-set bug cannot hide behind the max_iter exemption.


def first_integer_mismatch(got, ref):
    for k, (g, r) in enumerate(zip(got, ref)):
        if any(int(g[f]) != int(r[f]) for f in ("kind", "n_active", "n_enter", "n_leave", "factor_branch")):
            return k
    return None if len(got) == len(ref) else min(len(got), len(ref))


def knife_edge_margins(prob, settings, k):
    """margins min(|w - l|, |u - w|) / max(1, |w|) of every row in the ORACLE's state entering loop pass k (its first k passes re-run)"""
    from oracle import binding as ob
    o = ob.OracleSolver(prob, ob.default_settings(**dict(settings, max_iter=k)))
    o.solve()
    # (store_solution leaves y multiplied by 1/c in place, termination.c:85 -- undo it)
    y = o.vec("y") * (o.info()["scaling_c"] if settings.get("scaling", 10) > 0 else 1.0)
    w = o.vec("Ax") + o.vec("mu") * (o.vec("ybar") - 0.5 * y)
    l, u = o.vec("l"), o.vec("u")
    o.close()
    return np.minimum(np.abs(w - l), np.abs(u - w)) / np.maximum(1.0, np.abs(w))


def device_active_count_consistent(prob, settings, k):
    """the device's n_active of loop pass k (a Newton pass) against the rows with w <= l or w >= u in the device's own w of that pass
    (the run is repeated with max_iter = k + 1, so that pass k is the last one that ran and its w is what the workspace holds)"""
    from qpdo_amd import solver
    s = solver.QPDO().setup(prob["Q"], prob["q"], prob["A"], prob["l"], prob["u"], Qstype=prob.get("Qstype", -1), verbose=0, **dict(settings, max_iter=k + 1))
    s.solve()
    tr = s.trace()
    w, l, u = s.download("w"), s.download("l"), s.download("u")
    s.delete()
    return len(tr) == k + 1 and int(tr[k]["kind"]) == 0 and int(tr[k]["n_active"]) == int(((w <= l) | (w >= u)).sum())


# ---- the direct solvers as linear solvers (tests/test_direct_solver_checks_cpu.py, tests/test_gpu_direct_solvers.py) ----------------------
# The reference is K = Q + sigma I + A' diag(dw) A in extended precision (np.longdouble) from the problem's sparse data; the checks are the
# textbook ones for an LDL' of an SPD matrix without pivoting and for a backward-stable solve, with u the unit roundoff of float64.
U64 = np.finfo(np.float64).eps / 2


def _coo(M):
    import scipy.sparse as sp
    M = sp.coo_matrix(M)
    return M.row.astype(np.int64), M.col.astype(np.int64), M.data.astype(np.longdouble)


def newton_matrix(Qfull, A, sigma, dw):
    """dense K = Q + sigma I + A' diag(dw) A in np.longdouble (Qfull: the full symmetric Q; one outer product per row of A)"""
    import scipy.sparse as sp
    n = Qfull.shape[0]
    K = np.zeros((n, n), np.longdouble)
    qr, qc, qv = _coo(Qfull)
    np.add.at(K, (qr, qc), qv)
    K[np.arange(n), np.arange(n)] += np.longdouble(sigma)
    A = sp.csr_matrix(A)
    dw = np.asarray(dw, np.longdouble)
    for r in range(A.shape[0]):
        if dw[r] == 0:
            continue
        c = A.indices[A.indptr[r]:A.indptr[r + 1]]
        v = A.data[A.indptr[r]:A.indptr[r + 1]].astype(np.longdouble)
        K[np.ix_(c, c)] += dw[r] * np.outer(v, v)
    return K


def newton_residual(Qfull, A, sigma, dw, x, b):
    """b - K x in np.longdouble in O(nnz), K never formed; also |K|inf (exact when no entry of K is a sum of terms of both signs, an upper
    bound otherwise -- which only makes eta smaller than the true backward error by that cancellation)"""
    n = Qfull.shape[0]
    xl = np.asarray(x, np.longdouble)
    qr, qc, qv = _coo(Qfull)
    Kx = np.zeros(n, np.longdouble)
    np.add.at(Kx, qr, qv * xl[qc])
    Kx += np.longdouble(sigma) * xl
    rowabs = np.zeros(n, np.longdouble)
    np.add.at(rowabs, qr, np.abs(qv))
    rowabs += abs(np.longdouble(sigma))
    m = A.shape[0]
    if m:
        ar, ac, av = _coo(A)
        dwl = np.asarray(dw, np.longdouble)
        Ax = np.zeros(m, np.longdouble)
        np.add.at(Ax, ar, av * xl[ac])
        np.add.at(Kx, ac, av * (dwl * Ax)[ar])
        Aabs1 = np.zeros(m, np.longdouble)
        np.add.at(Aabs1, ar, np.abs(av))
        np.add.at(rowabs, ac, np.abs(av) * (np.abs(dwl) * Aabs1)[ar])
    return np.asarray(b, np.longdouble) - Kx, float(rowabs.max()) if n else 0.0


def backward_error(Qfull, A, sigma, dw, x, b, K=None):
    """normwise backward error of a solve: |b - K x|inf / (|K|inf |x|inf + |b|inf); K (dense, optional) gives the exact |K|inf"""
    r, kinf = newton_residual(Qfull, A, sigma, dw, x, b)
    if K is not None:
        kinf = float(np.abs(K).sum(axis=1).max())
    den = kinf * float(np.abs(x).max()) + float(np.abs(b).max())
    return float(np.abs(r).max()) / den if den > 0 else float(np.abs(r).max())


def ldl_elementwise_ratio(K, L, D, c=4.0):
    """max over the lower triangle of |K - L D L'| / (c n u |L| |D| |L'|): <= 1 is the textbook componentwise bound of an LDL' without
    pivoting of an SPD matrix (Higham, Accuracy and Stability of Numerical Algorithms, 10.1); c = 4 covers the check's own rounding (the
    product is evaluated in float64 BLAS).  An entry whose bound is 0 must be reproduced exactly (else the ratio is inf)."""
    n = K.shape[0]
    L = np.asarray(L, np.float64)
    D = np.asarray(D, np.float64)
    LD = L * D[None, :]
    E = np.abs(np.asarray(K, np.longdouble) - (LD @ L.T).astype(np.longdouble)).astype(np.float64)
    bound = c * n * U64 * ((np.abs(LD)) @ np.abs(L).T)
    low = np.tril(np.ones((n, n), bool))
    zero = low & (bound == 0)
    if np.any(E[zero] != 0):
        return float("inf")
    nz = low & (bound > 0)
    return float((E[nz] / bound[nz]).max()) if nz.any() else 0.0


def ldl_normwise_ratio(K, L, D, c=4.0):
    """max |K - L D L'| / (c n u max |L| |D| |L'|) over the lower triangle: the normwise form of the bound above"""
    n = K.shape[0]
    L = np.asarray(L, np.float64)
    LD = L * np.asarray(D, np.float64)[None, :]
    E = np.abs(np.asarray(K, np.longdouble) - (LD @ L.T).astype(np.longdouble)).astype(np.float64)
    bound = c * n * U64 * float(np.tril(np.abs(LD) @ np.abs(L).T).max())
    return float(np.tril(E).max()) / bound if bound > 0 else float(np.tril(E).max())


def blocked_ldl_with_inverse(K, nb=64):
    """a right-looking blocked LDL' whose panels are C L_jj^-T / D_j with the explicit inverse of the unit-lower diagonal block -- the
    scheme of the device's factorizations (k_ldl_panel, k_mid_factor), for the CPU comparison of its componentwise accuracy"""
    A = np.array(K, np.float64)
    n = A.shape[0]
    L, D = np.eye(n), np.zeros(n)
    for j0 in range(0, n, nb):
        j1 = min(n, j0 + nb)
        Lb, Db = ldl_numpy(A[j0:j1, j0:j1])
        L[j0:j1, j0:j1], D[j0:j1] = Lb, Db
        X = A[j1:, j0:j1] @ np.linalg.inv(Lb).T
        L[j1:, j0:j1] = X / Db[None, :]
        A[j1:, j1:] -= X @ L[j1:, j0:j1].T
    return L, D


def ldl_numpy(K):
    """a plain right-looking LDL' without pivoting (float64): unit-lower L and D with K = L D L'"""
    A = np.array(K, np.float64)
    n = A.shape[0]
    L = np.eye(n)
    D = np.zeros(n)
    for j in range(n):
        D[j] = A[j, j]
        L[j + 1:, j] = A[j + 1:, j] / D[j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], A[j + 1:, j])
    return L, D


def tiled_factor_image(L, D, tile=64):
    """the dense solver's storage of a factor (include/qpdo_amd_ext.h, qpdo_amd_download_factor): ld x ld, L strictly below the diagonal,
    its transposed copy in the upper triangle of every off-diagonal tile, identity padding; and D padded with ones"""
    n = L.shape[0]
    ld = (n + tile - 1) // tile * tile
    Kd = np.eye(ld)
    Kd[:n, :n] = np.tril(L, -1)
    blk = np.arange(ld) // tile
    off = blk[:, None] != blk[None, :]
    up = np.triu(off, 1)
    Kd[up] = Kd.T[up]
    Dg = np.ones(ld)
    Dg[:n] = D
    return Kd, Dg


def factor_from_image(Kd, Dg, n):
    """L (unit lower, n x n) and D from the dense solver's storage"""
    return np.tril(Kd[:n, :n], -1) + np.eye(n), np.asarray(Dg[:n], np.float64)


def transposed_copy_mismatch(Kd, tile=64):
    """number of entries of the off-diagonal tiles whose upper-triangle copy is not bit for bit the lower-triangle L"""
    ld = Kd.shape[0]
    blk = np.arange(ld) // tile
    low = blk[:, None] > blk[None, :]
    lo = Kd[low]
    cp = Kd.T[low]
    return int(np.count_nonzero(lo.view(np.uint64) != cp.view(np.uint64)))


def solve_with_image(Kd, Dg, b, tile=64):
    """x = K^-1 b the way the device's triangular solves read the storage: forward with L below the diagonal, backward with the
    transposed copies of the off-diagonal tiles (and the diagonal tiles' own L, as the stored inverses are)"""
    ld = Kd.shape[0]
    n = len(b)
    z = np.zeros(ld)
    z[:n] = b
    Lfwd = np.tril(Kd, -1) + np.eye(ld)
    blk = np.arange(ld) // tile
    same = blk[:, None] == blk[None, :]
    Ubwd = np.where(same, np.tril(Kd, -1).T, np.triu(Kd, 1)) + np.eye(ld)       # upper: L' from the copies, the diagonal tiles' own L'
    import scipy.linalg as sla
    y = sla.solve_triangular(Lfwd, z, lower=True, unit_diagonal=True)
    y /= Dg
    x = sla.solve_triangular(Ubwd, y, lower=False, unit_diagonal=True)
    return x[:n]
