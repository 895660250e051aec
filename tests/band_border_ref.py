"""Chain QPs with a few coupling VARIABLES (QPDO_BAND_BORDER; dev/band.inc, the bordered mode): a numpy statement of the detection rule of
qpdo_amd/csrc/band_border.c, the core-only problem whose plain band factor the bordered workspace must reproduce bit for bit, a float64
emulation of the block elimination the device runs -- K = [B C; C' D], Z = B^-1 C, S = D - C'Z, x = [z0 - Z t; t] with z0 = B^-1 rhs_1 and
t = S^-1 (rhs_2 - C'z0) -- and the oracle's Newton systems pass by pass.  Shared by tests/test_band_border_cpu.py and
tests/test_gpu_band_border.py."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle import binding as ob
from qpdo_amd import problems

BAND_MAX_B = 127        # dev/band.inc: T of the rule

# oracle at seed 11, default settings: (n_core, bw, c) -> (status, iterations, outer iterations)
ORACLE_SEED = 11
ORACLE_RESULTS = {(600, 5, 1): (1, 24, 6), (600, 5, 3): (1, 24, 6), (520, 12, 8): (1, 31, 7), (700, 17, 64): (1, 36, 8), (2100, 3, 2): (1, 42, 8)}
# instances on which some border variable lies more than 1e-3 off its bound 0 at the oracle's solution (a border pinned at zero tests
# little): the largest eps is 7.6e-3, 1.3e-2, 1.9e-2 and 2.8e-2 there, and zero on (600, 5, 1)
BORDER_OFF_BOUND = [(600, 5, 3), (520, 12, 8), (700, 17, 64), (2100, 3, 2)]

_CACHE = {}


def bordered_qp(key):
    """problems.bordered_banded_qp(ORACLE_SEED, *key), built once; every caller gets copies of its own"""
    if key not in _CACHE:
        _CACHE[key] = problems.bordered_banded_qp(ORACLE_SEED, *key)
    p = _CACHE[key]
    return dict(p, A=p["A"].copy(), Q=p["Q"].copy(), q=p["q"].copy(), l=p["l"].copy(), u=p["u"].copy())


def detect(Q, A, stype=-1, T=BAND_MAX_B):
    """(n_core, c, b_core) by the rule: n_core starts at n; a stored entry (i, j) of Q (the triangle stype names) with |i - j| > T sets
    n_core <= max(i, j); a row of A with ascending columns c1 < c2 < ... sets n_core <= the first column that exceeds c1 + T.
    b_core: the half-bandwidth of the pattern restricted to the columns < n_core, at least 3."""
    Q = sp.coo_matrix(Q)
    n = Q.shape[0]
    keep = np.ones(Q.nnz, bool) if stype == 0 else (Q.row >= Q.col if stype < 0 else Q.row <= Q.col)
    qi, qj = Q.row[keep].astype(np.int64), Q.col[keep].astype(np.int64)
    n_core = n
    wide = np.abs(qi - qj) > T
    if wide.any():
        n_core = min(n_core, int(np.maximum(qi, qj)[wide].min()))
    rows = []
    if A is not None and A.shape[0]:
        A = sp.csr_matrix(A)
        for r in range(A.shape[0]):
            cols = np.sort(A.indices[A.indptr[r]:A.indptr[r + 1]].astype(np.int64))
            rows.append(cols)
            if len(cols) and (cols > cols[0] + T).any():
                n_core = min(n_core, int(cols[cols > cols[0] + T][0]))
    b = 0
    inside = (qi < n_core) & (qj < n_core)
    if inside.any():
        b = int(np.abs(qi - qj)[inside].max())
    for cols in rows:
        cols = cols[cols < n_core]
        if len(cols):
            b = max(b, int(cols[-1] - cols[0]))
    return n_core, n - n_core, max(3, b)


def core_problem(p, n_core):
    """p with the border columns deleted: the same rows (a row of border variables alone stays, empty), the same weights fit"""
    Q = sp.csc_matrix(sp.csr_matrix(sp.csc_matrix(p["Q"])[:, :n_core])[:n_core])
    A = sp.csc_matrix(sp.csc_matrix(p["A"])[:, :n_core])
    Q.sort_indices(); A.sort_indices()
    return dict(p, n=n_core, Q=Q, A=A, q=np.asarray(p["q"])[:n_core].copy())


def eliminate_solve(K, n_core, rhs):
    """K x = rhs in float64 by the device's elimination: B = K[:n_core, :n_core] factored, Z = B^-1 C, S = D - C'Z factored (both without
    pivoting: Cholesky), z0 = B^-1 rhs_1, t = S^-1 (rhs_2 - C'z0), x = [z0 - Z t; t]"""
    K = np.asarray(K, np.float64)
    rhs = np.asarray(rhs, np.float64)
    cB = sla.cho_factor(K[:n_core, :n_core], lower=True)
    C, D = K[:n_core, n_core:], K[n_core:, n_core:]
    Z = sla.cho_solve(cB, C)
    cS = sla.cho_factor(D - C.T @ Z, lower=True)
    z0 = sla.cho_solve(cB, rhs[:n_core])
    t = sla.cho_solve(cS, rhs[n_core:] - C.T @ z0)
    return np.concatenate([z0 - Z @ t, t])


def dense_backward_error(K, x, b):
    """tests/helpers.backward_error for a K that is only known as a dense float64 matrix: |b - K x|inf / (|K|inf |x|inf + |b|inf), the
    residual in np.longdouble"""
    Kl, xl = np.asarray(K, np.longdouble), np.asarray(x, np.longdouble)
    r = np.asarray(b, np.longdouble) - Kl @ xl
    den = float(np.abs(Kl).sum(axis=1).max()) * float(np.abs(xl).max()) + float(np.abs(b).max())
    return float(np.abs(r).max()) / den if den > 0 else float(np.abs(r).max())


def oracle_newton_systems(p, **settings):
    """One dict per Newton pass of the oracle's run on p, in float64 and in the oracle's (scaled) space: K as a dense matrix from the
    oracle's own K_apply with the pass's (sigma_f, d), rhs = -res_dual_in - A't with t the multiplier step the pass starts from, dx = the
    oracle's direction.  The run is repeated with max_iter cut behind each Newton pass, so that the pass is the last one that ran
    (tests/band_coupled_ref.py has the same construction)."""
    n = p["n"]
    total = ob.OracleSolver(p, ob.default_settings(**settings))
    total.solve()
    trace = total.trace()
    total.close()
    L = ob.lib()
    eye, col = np.eye(n), np.zeros(n)
    Acsr = sp.csr_matrix(p["A"])
    for k, rec in enumerate(trace):
        if int(rec["kind"]) != 0:
            continue
        o = ob.OracleSolver(p, ob.default_settings(**dict(settings, max_iter=k + 1)))
        o.solve()
        As = (sp.diags(o.vec("E")) @ Acsr @ sp.diags(o.vec("D"))).tocsr()          # the oracle's scaled A
        w, lo, up = o.vec("w"), o.vec("l"), o.vec("u")
        t = o.vec("res_prim_in") / o.vec("mu")
        t[~((w <= lo) | (w >= up))] *= 2.0
        rhs = -o.vec("res_dual_in") - As.T @ t
        dx = o.vec("dx")
        K = np.zeros((n, n))
        for j in range(n):
            L.oracle_K_apply(o.h, ob._dp(eye[j]), ob._dp(col), 0)
            K[:, j] = col
        o.close()
        yield dict(pass_no=k, K=K, rhs=rhs, dx=dx)
