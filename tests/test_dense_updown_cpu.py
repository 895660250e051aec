"""The in-place up/downdate of a kept LDL' factor (QPDO_DENSE_UPDOWN, qpdo_amd/csrc/dev/updown.inc), restated in numpy
(tests/updown_ref.py), against K assembled in extended precision: on the well-conditioned family of tests/test_gpu_direct_solvers.py five
successive changes keep the factor inside the project's bounds for a FRESH factorization (normwise factor ratio <= 1, backward error of a
solve <= 4 n u; measured: 0.012 and 0.007 n u); the same checks miss a sign-flipped beta and an update that leaves the diagonal tiles
alone by three orders of magnitude or more; and a downdate that makes K indefinite is refused by the scan, before L changes.
tests/test_gpu_dense_updown.py holds the device's kernels to the same bounds."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import U64, backward_error, ldl_normwise_ratio, ldl_numpy, newton_matrix
from test_gpu_direct_solvers import matrix, rhs_set
from updown_ref import ldl_solve, updown_row

MARGIN = 1e3


def changes(rng, dw, k, step):
    """k rows and their new weights: signs mixed, and one weight set to 0 on step 2"""
    rows = rng.choice(len(dw), k, replace=False)
    new = dw[rows] * np.where(rng.random(k) < 0.5, 0.2 + 0.6 * rng.random(k), 1.5 + 3.0 * rng.random(k))
    new = np.where(dw[rows] == 0.0, 1.0 + rng.random(k), new)          # (a weight an earlier step set to 0 comes back: every chosen row changes)
    if step == 2:
        new[0] = 0.0
    return rows, new


def apply_rows(L, D, A, dw, rows, new, **wrong):
    dw = dw.copy()
    for r, w in zip(rows, new):
        a = np.asarray(A[r].todense()).ravel()
        L, D, ok = updown_row(L, D, a, w - dw[r], **wrong)
        assert ok, (r, w, dw[r])
        dw[r] = w
    return L, D, dw


def eta_max(Qf, A, sigma, dw, K, L, D, n):
    return max(backward_error(Qf, A, sigma, dw, ldl_solve(L, D, b), b, K=K) for b in rhs_set(Qf, A, sigma, dw, n)) / (n * U64)


@pytest.mark.parametrize("n", [65, 207, 369, 1008])
def test_five_successive_changes_stay_inside_the_bounds_of_a_fresh_factor(n):
    Qf, A, sigma, dw = matrix("well", n)
    A = sp.csr_matrix(A)
    rng = np.random.default_rng(n)
    L, D = ldl_numpy(newton_matrix(Qf, A, sigma, dw).astype(np.float64))
    worst = [0.0, 0.0]
    for step in range(5):
        rows, new = changes(rng, dw, 1 + step % 3, step)
        L, D, dw = apply_rows(L, D, A, dw, rows, new)
        assert np.all(D > 0) and np.all(np.isfinite(D))
        K = newton_matrix(Qf, A, sigma, dw)
        ratio, eta = ldl_normwise_ratio(K, L, D), eta_max(Qf, A, sigma, dw, K, L, D, n)
        worst = [max(worst[0], ratio), max(worst[1], eta)]
        assert ratio <= 1.0, (step, ratio)
        assert eta <= 4.0, (step, eta)
    print("n = %d: normwise factor ratio %.3g, eta / (n u) %.3g" % (n, *worst))


@pytest.mark.parametrize("wrong", [{"beta_sign": -1.0}, {"skip_diagonal_tiles": True}])
def test_the_checks_catch_a_wrong_update(wrong):
    n = 207
    Qf, A, sigma, dw = matrix("well", n)
    A = sp.csr_matrix(A)
    rng = np.random.default_rng(5)
    L, D = ldl_numpy(newton_matrix(Qf, A, sigma, dw).astype(np.float64))
    rows, new = changes(rng, dw, 3, 0)
    Lg, Dg, dw1 = apply_rows(L, D, A, dw, rows, new)
    Lb, Db, _ = apply_rows(L, D, A, dw, rows, new, **wrong)
    K = newton_matrix(Qf, A, sigma, dw1)
    assert ldl_normwise_ratio(K, Lg, Dg) <= 1.0 and eta_max(Qf, A, sigma, dw1, K, Lg, Dg, n) <= 4.0
    assert ldl_normwise_ratio(K, Lb, Db) >= MARGIN
    assert eta_max(Qf, A, sigma, dw1, K, Lb, Db, n) >= 4.0 * MARGIN


def test_a_downdate_that_makes_K_indefinite_is_refused_before_L_changes():
    n = 207
    Qf, A, sigma, dw = matrix("well", n)
    A = sp.csr_matrix(A)
    K = newton_matrix(Qf, A, sigma, dw).astype(np.float64)
    L, D = ldl_numpy(K)
    r = int(np.argmax(np.asarray(A.multiply(A).sum(axis=1)).ravel()))
    a = np.asarray(A[r].todense()).ravel()
    delta = -dw[r] - 2.0 / float(a @ np.linalg.solve(K - dw[r] * np.outer(a, a), a))      # removes more weight than the row has
    assert np.linalg.eigvalsh(K + delta * np.outer(a, a))[0] < 0
    L0, D0 = L.copy(), D.copy()
    L1, D1, ok = updown_row(L, D, a, delta)
    assert not ok
    assert np.array_equal(L1, L0) and np.array_equal(D1, D0)
