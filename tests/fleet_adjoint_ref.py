"""The reference of the fleet's adjoint call (qpdo_amd_fleet_adjoint_dev, include/qpdo_amd_ext.h): pure numpy, no GPU, no library.

Item:  min 1/2 x'Qx + q'x  s.t.  l <= Ax <= u,  solved to x, y with Qx + q + A'y ~ 0.  With t = Ax + y, row i is upper-active (+1) when
t_i >= u_i, else lower-active (-1) when t_i <= l_i, else inactive (0); a bound of magnitude >= 1e20 is never reached.  S: the flagged
rows.  Given gx = dL/dx and gy = dL/dy the adjoint system is

    [ Q    A_S' ] [vx]   [ gx   ]
    [ A_S  0    ] [vy] = [ gy_S ]

and  dL/dq = -vx,  dL/du_i = vy_i on +1 rows,  dL/dl_i = vy_i on -1 rows,  dL/dA_ij = -(y_i vx_j + vy_i x_j) on flagged rows,
dL/dQ_ab = -vx_a x_b (stype 0), -(vx_a x_b + vx_b x_a) (an off-diagonal stored entry, stype +-1), -vx_a x_a (diagonal).
Everything is evaluated in np.longdouble; matrices are dense (the items are small)."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
INFTY = 1e20


def dense(M):
    return np.asarray(M.todense() if sp.issparse(M) else M, dtype=np.float64)


def full_Q(Q, stype):
    """the dense symmetric matrix a stored Q of the given stype stands for"""
    Qd = dense(Q)
    if stype == 0:
        return Qd
    T = np.tril(Qd) if stype < 0 else np.triu(Qd)
    return T + T.T - np.diag(np.diag(T))


def row_t(x, y, A):
    """t = Ax + y in longdouble"""
    A = dense(A).astype(LD)
    return A @ np.asarray(x, LD) + np.asarray(y, LD)


def classify(x, y, A, l, u):
    """the flags (+1 upper-active, -1 lower-active, 0 inactive; int32), evaluated in longdouble"""
    t = row_t(x, y, A)
    l, u = np.asarray(l, LD), np.asarray(u, LD)
    up = (t >= u) & (np.abs(u) < INFTY)
    lo = ~up & (t <= l) & (np.abs(l) < INFTY)
    return (up.astype(np.int32) - lo.astype(np.int32)).astype(np.int32)


def margins(x, y, A, l, u):
    """distance of t_i from the nearer finite bound, divided by (1 + |that bound|); inf for a row without a finite bound"""
    t = row_t(x, y, A)
    out = np.full(len(t), np.inf)
    for b in (np.asarray(l, float), np.asarray(u, float)):
        fin = np.abs(b) < INFTY
        d = np.abs(t - b.astype(LD)).astype(np.float64) / (1.0 + np.abs(b))
        out = np.where(fin & (d < out), d, out)
    return out


def kkt(Q, A, flags):
    """the (n + k) x (n + k) matrix of the adjoint system for the dense full symmetric Q (longdouble) and the row indices of S"""
    Q, A = np.asarray(Q, LD), np.asarray(A, LD)
    n = Q.shape[0]
    S = np.flatnonzero(np.asarray(flags) != 0)
    k = len(S)
    M = np.zeros((n + k, n + k), LD)
    M[:n, :n] = Q
    if k:
        M[:n, n:] = A[S].T
        M[n:, :n] = A[S]
    return M, S


def solve_ref(M, rhs, max_refine=50):
    """M v = rhs: float64 LU (least squares when that fails), refined in longdouble until the longdouble residual stalls.
    Returns v (longdouble) and the final residual's inf-norm."""
    M, rhs = np.asarray(M, LD), np.asarray(rhs, LD)
    M64 = M.astype(np.float64)

    def lin(b):
        try:
            return np.linalg.solve(M64, b.astype(np.float64)).astype(LD)
        except np.linalg.LinAlgError:
            return np.linalg.lstsq(M64, b.astype(np.float64), rcond=None)[0].astype(LD)

    if M.shape[0] == 0:
        return np.zeros(0, LD), 0.0
    v = lin(rhs)
    best = np.abs(rhs - M @ v).max()
    for _ in range(max_refine):
        r = rhs - M @ v
        w = v + lin(r)
        rn = np.abs(rhs - M @ w).max()
        if not rn < best:
            break
        v, best = w, rn
    return v, float(best)


def adjoint(Qfull, A, flags, gx, gy=None):
    """(vx, vy over all m rows with 0 off S, M, S) of the adjoint system, longdouble"""
    A = dense(A)
    n, m = Qfull.shape[0], A.shape[0]
    M, S = kkt(Qfull, A, flags)
    rhs = np.zeros(n + len(S), LD)
    rhs[:n] = np.asarray(gx, LD)
    if gy is not None and len(S):
        rhs[n:] = np.asarray(gy, LD)[S]
    v, _ = solve_ref(M, rhs)
    vy = np.zeros(m, LD)
    vy[S] = v[n:]
    return v[:n], vy, M, S


def gradients(Q, stype, A, flags, x, y, vx, vy):
    """dict(dq, dl, du, dQ_values, dA_values): the formulas above in longdouble.  Q, A: scipy CSC as stored (sorted indices); dQ_values /
    dA_values follow the order of their .data (the fleet's packed value layout, item by item)."""
    Q, A = sp.csc_matrix(Q), sp.csc_matrix(A)
    Q.sort_indices(); A.sort_indices()
    flags = np.asarray(flags)
    x, y, vx, vy = (np.asarray(v, LD) for v in (x, y, vx, vy))
    m = A.shape[0]
    dl, du = np.zeros(m, LD), np.zeros(m, LD)
    du[flags > 0] = vy[flags > 0]
    dl[flags < 0] = vy[flags < 0]
    ai, aj = A.indices, np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    dA = np.where(flags[ai] != 0, -(y[ai] * vx[aj] + vy[ai] * x[aj]), LD(0.0)) if A.nnz else np.zeros(0, LD)
    qa, qb = Q.indices, np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))
    if Q.nnz == 0:
        dQ = np.zeros(0, LD)
    elif stype == 0:
        dQ = -(vx[qa] * x[qb])
    else:
        dQ = np.where(qa == qb, -(vx[qa] * x[qa]), -(vx[qa] * x[qb] + vx[qb] * x[qa]))
    return dict(dq=-vx, dl=dl, du=du, dQ_values=dQ, dA_values=dA)


def matrix_terms(Q, stype, A, flags, x, y, vx, vy):
    """per stored entry, the sum of the absolute values of the terms of its formula (the scale of its rounding error)"""
    Q, A = sp.csc_matrix(Q), sp.csc_matrix(A)
    Q.sort_indices(); A.sort_indices()
    flags = np.asarray(flags)
    x, y, vx, vy = (np.abs(np.asarray(v, LD)) for v in (x, y, vx, vy))
    ai, aj = A.indices, np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    tA = np.where(flags[ai] != 0, y[ai] * vx[aj] + vy[ai] * x[aj], LD(0.0)) if A.nnz else np.zeros(0, LD)
    qa, qb = Q.indices, np.repeat(np.arange(Q.shape[1]), np.diff(Q.indptr))
    if Q.nnz == 0:
        tQ = np.zeros(0, LD)
    elif stype == 0:
        tQ = vx[qa] * x[qb]
    else:
        tQ = np.where(qa == qb, vx[qa] * x[qa], vx[qa] * x[qb] + vx[qb] * x[qa])
    return tQ, tA
