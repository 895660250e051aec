"""Chain QPs with a few dense coupling rows (QPDO_BAND_COUPLING; dev/band.inc): the instance generator and a float64 numpy reference of the
solve the device runs -- K = B + U W U' with B banded, x = z0 - Z S^-1 (U' z0), z0 = B^-1 v, Z = B^-1 U, S = W^-1 + U' Z, as the inner
solver of an iterative refinement on the true K under the acceptance rule of host_dense.inc (dense_refine_checked, WB_RES_TOL).  Shared by
tests/test_band_coupled_cpu.py (the reference itself, and the pass-by-pass emulation on the oracle's Newton systems) and
tests/test_gpu_band_coupled.py."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle import binding as ob
from qpdo_amd import problems

BAND_MAX_B = 127        # dev/band.inc: a row of A with a wider column span is a coupling row
WB_RES_TOL = 1e-13      # host_dense.inc: relative inf-norm residual accepted
WB_MAX_REFINE = 5

# oracle at seed 11, default settings: (n, bw, r) -> (status, iterations, outer iterations)
ORACLE_SEED = 11
ORACLE_RESULTS = {(600, 5, 1): (1, 24, 7), (600, 5, 3): (1, 26, 7), (520, 12, 8): (1, 26, 7), (700, 17, 64): (1, 22, 6), (2100, 3, 2): (1, 41, 8)}


def coupling_rows(seed, n, r):
    """the r coupling rows as a dense r x n array: even ones all ones, odd ones random on about half the columns, first and last set"""
    rng = np.random.default_rng(seed + 7919)
    U = np.zeros((r, n))
    for k in range(r):
        if k % 2 == 0:
            U[k] = 1.0
        else:
            v = rng.standard_normal(n) * (rng.random(n) < 0.5)
            v[0], v[n - 1] = 1.0, -1.0
            U[k] = v
    return U


def append_rows(p, U, l, u):
    """problem p with the rows of U (dense, zeros dropped) behind its own"""
    A = sp.vstack([sp.csr_matrix(p["A"]), sp.csr_matrix(U)]).tocsc()
    A.sort_indices()
    return dict(p, m=A.shape[0], A=A, l=np.concatenate([p["l"], l]), u=np.concatenate([p["u"], u]))


_CACHE = {}


def _oracle_x(p):
    o = ob.OracleSolver(p, ob.default_settings())
    x = o.solve()["x"]
    o.close()
    return x


def coupled_banded_qp(seed, n, bw, r, solve=_oracle_x):
    """problems.banded_random_qp(seed, n, bw) with r coupling rows behind its rows; their bounds are set from their activity ax at the
    solution of the problem with these rows free: every third one an equality at 0, the others 0.3 ax on the side ax lies (x = 0 stays
    feasible).  solve(problem) -> x gives that solution: the oracle (the tests), or a solver that reaches orders the oracle's dense
    factorization does not (tools/band_coupled_latency.py)."""
    key = (seed, n, bw, r)
    if key not in _CACHE:
        base = problems.banded_random_qp(seed, n, bw)
        U = coupling_rows(seed, n, r)
        ax = U @ solve(append_rows(base, U, np.full(r, -1e20), np.full(r, 1e20)))
        l, u = np.full(r, -1e20), np.full(r, 1e20)
        for k in range(r):
            if k % 3 == 2:
                l[k] = u[k] = 0.0
            elif ax[k] > 0:
                u[k] = 0.3 * ax[k]
            else:
                l[k] = 0.3 * ax[k]
        _CACHE[key] = append_rows(base, U, l, u)
    p = _CACHE[key]
    return dict(p, A=p["A"].copy(), Q=p["Q"].copy(), q=p["q"].copy(), l=p["l"].copy(), u=p["u"].copy())


def classify(Qfull, A):
    """(coupling row numbers ascending, b_core) as band_detect derives them from the pattern: span = last - first column of a row"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    spans = np.array([A.indices[A.indptr[i + 1] - 1] - A.indices[A.indptr[i]] if A.indptr[i + 1] > A.indptr[i] else 0 for i in range(A.shape[0])])
    Qc = sp.coo_matrix(Qfull)
    qb = int(np.abs(Qc.row - Qc.col).max()) if Qc.nnz else 0
    rows = np.nonzero(spans > BAND_MAX_B)[0]
    core = spans[spans <= BAND_MAX_B]
    return rows, max(3, qb, int(core.max()) if core.size else 0)


def woodbury_refine_solve(B, U, w, Kmul, rhs, tol=WB_RES_TOL, max_refine=WB_MAX_REFINE):
    """K x = rhs in float64.  B: dense band part (SPD), U: n x k columns of the weighted coupling rows, w: their k weights, Kmul(x) = K x
    on the true K.  Returns (x, sweeps, accepted, relative residuals per sweep); the acceptance rule is dense_refine_checked's."""
    cB = sla.cho_factor(B, lower=True)
    k = U.shape[1]
    if k:
        Z = sla.cho_solve(cB, U)
        cS = sla.cho_factor(np.diag(1.0 / np.asarray(w, float)) + U.T @ Z, lower=True)

    def inner(v):
        z0 = sla.cho_solve(cB, v)
        return z0 - Z @ sla.cho_solve(cS, U.T @ z0) if k else z0

    nb = float(np.abs(rhs).max())
    x = inner(rhs)
    rel, prev, ok = [], 0.0, False
    for it in range(max_refine + 1):
        if it > 0:
            x = x + inner(res)
        res = rhs - Kmul(x)
        nr = float(np.abs(res).max())
        rel.append(nr / nb if nb > 0 else nr)
        if nr <= tol * nb:
            ok = True
            break
        if it > 0 and not nr < 0.25 * prev:
            ok = nr <= 1e3 * tol * nb
            break
        prev = nr
    return x, len(rel), ok, rel


def oracle_newton_systems(p, **settings):
    """One dict per Newton pass of the oracle's run on p, everything in float64 and in the oracle's (scaled) space: K and B as dense
    matrices from the oracle's own K_apply -- K with the pass's (sigma_f, d) as the run left them, B with the coupling rows' weights
    zeroed --, U = the scaled coupling rows with a nonzero weight as columns, w = their weights, rhs = -res_dual_in - A't with t the
    multiplier step the pass starts from (the oracle's right-hand side; its Atdy is overwritten with the final dy's), dx = the oracle's
    direction.  The run is repeated with max_iter cut behind each Newton pass, so that the pass is the last one that ran."""
    n = p["n"]
    rows, _ = classify(problems.full_Q(p), p["A"])
    total = ob.OracleSolver(p, ob.default_settings(**settings))
    total.solve()
    trace = total.trace()
    total.close()
    L = ob.lib()
    eye, col = np.eye(n), np.zeros(n)
    Acsr = sp.csr_matrix(p["A"])

    def dense(o):
        out = np.zeros((n, n))
        for j in range(n):
            L.oracle_K_apply(o.h, ob._dp(eye[j]), ob._dp(col), 0)
            out[:, j] = col
        return out

    for k, rec in enumerate(trace):
        if int(rec["kind"]) != 0:
            continue
        o = ob.OracleSolver(p, ob.default_settings(**dict(settings, max_iter=k + 1)))
        o.solve()
        d = o.vec("d")
        As = (sp.diags(o.vec("E")) @ Acsr @ sp.diags(o.vec("D"))).tocsr()          # the oracle's scaled A
        w, lo, up = o.vec("w"), o.vec("l"), o.vec("u")
        t = o.vec("res_prim_in") / o.vec("mu")
        t[~((w <= lo) | (w >= up))] *= 2.0
        rhs = -o.vec("res_dual_in") - As.T @ t
        dx = o.vec("dx")
        K = dense(o)
        dcore = d.copy()
        dcore[rows] = 0.0
        # (every Newton pass factors with the current sigma: a change of sigma forces a full factorization, newton_direction)
        L.oracle_set_factor_state(o.h, float(rec["sigma"]), ob._dp(np.ascontiguousarray(dcore)))
        B = dense(o)
        o.close()
        act = rows[d[rows] != 0.0]
        U = As[act].toarray().T.reshape(n, len(act))
        yield dict(pass_no=k, K=K, B=B, U=U, w=d[act], rhs=rhs, dx=dx)
