"""numpy restatement of the in-place up/downdate of a kept LDL' factor (qpdo_amd/csrc/dev/updown.inc): K' = K + delta a a' changes
K = L D L' (L unit lower) into K' = L' D' L'.  Method C1 of Gill, Golub, Murray and Saunders (Math. Comp. 28, 1974), its running
quantity written as a prefix sum:
    p = L^-1 a,   t_0 = 1 / delta,   t_{j+1} = t_j + p_j^2 / D_j,   D'_j = D_j t_{j+1} / t_j,   beta_j = (p_j / D_j) / t_{j+1}
    row r, s = a_r, for j < r in order:   s -= p_j L_rj,   L'_rj = L_rj + beta_j s
The scan comes first and refuses the row (ok = False, L and D returned as they were) if a D'_j is not a positive finite number."""
import numpy as np
import scipy.linalg as sla


def updown_scan(p, D, delta):
    """(D', beta, ok)"""
    q = p / D
    with np.errstate(all="ignore"):
        t = 1.0 / delta + np.concatenate([[0.0], np.cumsum(p * q)])
        Dn = D * (t[1:] / t[:-1])
        beta = q / t[1:]
    ok = bool(np.all(np.isfinite(Dn)) and np.all(Dn > 0) and np.all(np.isfinite(beta)))
    return Dn, beta, ok


def updown_apply(L, p, beta, a, beta_sign=1.0, skip_diagonal_tiles=False, tile=64):
    """the pass over L (column by column over all rows at once: per row the recurrence above).  beta_sign = -1 and skip_diagonal_tiles
    are the two WRONG variants the tests use to show that their checks notice."""
    n = len(a)
    s = np.array(a, np.float64)
    Ln = L.copy()
    for j in range(n - 1):
        s[j + 1:] -= p[j] * L[j + 1:, j]
        lo = (j // tile + 1) * tile if skip_diagonal_tiles else j + 1           # (wrong: rows of column j inside its diagonal tile keep the old L)
        Ln[lo:, j] = L[lo:, j] + beta_sign * beta[j] * s[lo:]
    return Ln


def updown_row(L, D, a, delta, **wrong):
    """(L', D', ok) for one changed row; ok = False: the scan refused it and L, D come back untouched"""
    p = sla.solve_triangular(L, a, lower=True, unit_diagonal=True)
    Dn, beta, ok = updown_scan(p, D, delta)
    if not ok:
        return L, D, False
    return updown_apply(L, p, beta, a, **wrong), Dn, True


def ldl_solve(L, D, b):
    y = sla.solve_triangular(L, b, lower=True, unit_diagonal=True) / D
    return sla.solve_triangular(L.T, y, lower=False, unit_diagonal=True)
