"""The reference of the fleet's tangent call (qpdo_amd_fleet_tangent_dev, include/qpdo_amd_ext.h): pure numpy, no GPU, no library, built on
tests/fleet_adjoint_ref.py (kkt, solve_ref).

With S the flagged rows of the last solve, b = u on +1 rows and l on -1 rows, and (tq, tl, tu, tQ, tA) a perturbation of the item's data,
the first-order change of the solution at the fixed active set solves

    [ Q    A_S' ] [dx  ]   [ -(tq + tQ x + tA_S' y_S) ]
    [ A_S  0    ] [dy_S] = [  tb_S - tA_S x           ]

tQ_values / tA_values follow the order of the stored Q's / A's CSC .data (the fleet's packed value layout).  tQ acts as the symmetric matrix
its stored entries stand for: under stype +-1 the named triangle mirrored (the other triangle's entries contribute nothing); under stype 0
row a is evaluated from the stored entries of COLUMN a, which is the same thing for the symmetric perturbation the caller is to pass.
Everything is evaluated in np.longdouble; matrices are dense (the items are small)."""
import numpy as np
import scipy.sparse as sp

import fleet_adjoint_ref as ref

LD = ref.LD


def _stored(Mx, values):
    """(dense longdouble matrix of the stored entries with the given values, boolean pattern); values None: zeros"""
    Mx = sp.csc_matrix(Mx)
    Mx.sort_indices()
    D, pat = np.zeros(Mx.shape, LD), np.zeros(Mx.shape, bool)
    rows, cols = Mx.indices, np.repeat(np.arange(Mx.shape[1]), np.diff(Mx.indptr))
    pat[rows, cols] = True
    if values is not None:
        values = np.asarray(values, LD)
        assert len(values) == Mx.nnz
        D[rows, cols] = values
    return D, pat


def tq_operator(Q, stype, tQ_values):
    """(T, pattern): (tQ x)_a = sum_b T[a, b] x_b as the call evaluates it"""
    D, pat = _stored(Q, tQ_values)
    if stype == 0:
        return D.T.copy(), pat.T.copy()
    tri, ptri = (np.tril(D), np.tril(pat)) if stype < 0 else (np.triu(D), np.triu(pat))
    return tri + tri.T - np.diag(np.diag(tri)), ptri | ptri.T


def tangent_rhs(Q, stype, A, flags, x, y, tq=None, tl=None, tu=None, tQ_values=None, tA_values=None):
    """dict(rx (n), ry (k, over S), S, T (n + k: per component the sum of the absolute values of the formation's terms), L (the number of
    terms of the formation's longest row)), longdouble"""
    A = sp.csc_matrix(A)
    m, n = A.shape
    flags = np.asarray(flags)
    S = np.flatnonzero(flags != 0)
    x, y = np.asarray(x, LD), np.asarray(y, LD)
    TQ, patQ = tq_operator(Q, stype, tQ_values)
    TA, patA = _stored(A, tA_values)
    tqv = np.zeros(n, LD) if tq is None else np.asarray(tq, LD)
    tb = np.zeros(m, LD)
    if tu is not None:
        tb[flags > 0] = np.asarray(tu, LD)[flags > 0]
    if tl is not None:
        tb[flags < 0] = np.asarray(tl, LD)[flags < 0]
    useQ, useA = tQ_values is not None, tA_values is not None
    rx = -(tqv + (TQ @ x if useQ else 0) + (TA[S].T @ y[S] if useA and len(S) else 0))
    ry = tb[S] - (TA[S] @ x if useA and len(S) else 0)
    Tx = np.abs(tqv) + (np.abs(TQ) @ np.abs(x) if useQ else 0) + (np.abs(TA[S]).T @ np.abs(y[S]) if useA and len(S) else 0)
    Ty = np.abs(tb[S]) + (np.abs(TA[S]) @ np.abs(x) if useA and len(S) else 0)
    Lx = 1 + (patQ.sum(axis=1) if useQ else 0) + (patA[S].sum(axis=0) if useA and len(S) else 0)
    Ly = 1 + (patA[S].sum(axis=1) if useA and len(S) else np.zeros(len(S), int))
    L = int(max(np.max(Lx) if np.ndim(Lx) else Lx, np.max(Ly) if len(S) else 0))
    return dict(rx=np.asarray(rx, LD), ry=np.asarray(ry, LD), S=S, T=np.concatenate([np.asarray(Tx, LD) + np.zeros(n, LD), np.asarray(Ty, LD)]), L=L)


def tangent(Qfull, A, flags, rx, ry):
    """(dx, dy over all m rows with 0 off S, M, S) of the tangent system for the right-hand side (rx, ry over S), longdouble"""
    A = ref.dense(A)
    n, m = Qfull.shape[0], A.shape[0]
    M, S = ref.kkt(Qfull, A, flags)
    d, _ = ref.solve_ref(M, np.concatenate([np.asarray(rx, LD), np.asarray(ry, LD)]))
    dy = np.zeros(m, LD)
    dy[S] = d[n:]
    return d[:n], dy, M, S


def duality_sides(g, d, v, r):
    """(<g, d>, <v, r>, |g|.|d| + |v|.|r|) in longdouble: g, r the right-hand sides and v, d the solutions of the adjoint and tangent systems,
    all over the n + k unknowns"""
    g, d, v, r = (np.asarray(a, LD) for a in (g, d, v, r))
    return g @ d, v @ r, np.abs(g) @ np.abs(d) + np.abs(v) @ np.abs(r)
