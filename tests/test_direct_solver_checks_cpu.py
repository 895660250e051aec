"""The checks of tests/test_gpu_direct_solvers.py have teeth: on the CPU, a plain LDL' of a random SPD matrix passes the elementwise factor
check and the backward-error check of a solve through the dense solver's tiled storage, and each of the errors a wrong kernel would make --
one rank-64 contribution left out of one 64 x 64 block of L, L rounded to float32, a transposed copy that is not L' in one tile -- fails
them by three orders of magnitude or more."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import (U64, backward_error, blocked_ldl_with_inverse, factor_from_image, ldl_elementwise_ratio, ldl_normwise_ratio, ldl_numpy,
                     newton_matrix, solve_with_image, tiled_factor_image, transposed_copy_mismatch)

N = 200          # four block columns (the last one partial): tiles below, beside and on the diagonal
MARGIN = 1e3     # a perturbed factor must miss the bound by at least this much


def _problem(seed=7, n=N, m=300):
    rng = np.random.default_rng(seed)
    Q = sp.random(n, n, density=0.02, random_state=rng)
    Q = Q + Q.T + sp.diags(1.0 + rng.random(n))
    A = sp.random(m, n, density=0.05, random_state=rng, format="csr")
    A = sp.vstack([A, sp.csr_matrix(rng.standard_normal((1, n)))]).tocsr()     # one dense row: every tile of K is nonzero
    dw = 0.1 + 10 * rng.random(m + 1)
    sigma = 1.0
    K = newton_matrix(Q, A, sigma, dw)
    assert np.all(np.linalg.eigvalsh(K.astype(np.float64)) > 0)
    return Q, A, sigma, dw, K


def _solves(Q, A, sigma, dw, K, Kd, Dg):
    rng = np.random.default_rng(3)
    n = K.shape[0]
    xt = rng.standard_normal(n)
    bs = [rng.standard_normal(n), np.eye(n)[0], (K @ xt.astype(np.longdouble)).astype(np.float64)]
    return max(backward_error(Q, A, sigma, dw, solve_with_image(Kd, Dg, b), b, K=K) for b in bs) / (4 * n * U64)


def test_plain_ldl_passes_both_checks():
    Q, A, sigma, dw, K = _problem()
    L, D = ldl_numpy(K.astype(np.float64))
    assert np.all(D > 0)
    assert ldl_elementwise_ratio(K, L, D) <= 1.0
    Kd, Dg = tiled_factor_image(L, D)
    assert transposed_copy_mismatch(Kd) == 0
    L2, D2 = factor_from_image(Kd, Dg, N)
    assert np.array_equal(L2, L) and np.array_equal(D2, D)
    assert _solves(Q, A, sigma, dw, K, Kd, Dg) <= 1.0


def test_a_block_missing_one_rank64_contribution_fails():
    Q, A, sigma, dw, K = _problem()
    L, D = ldl_numpy(K.astype(np.float64))
    # block (2, 1) of L: L21 = (K21 - sum_{k<1} L2k D_k L1k') L11^-T / D_1; leave the k = 0 term out
    r, c = slice(128, 192), slice(64, 128)
    L1k, L2k, Dk = L[64:128, 0:64], L[128:192, 0:64], D[0:64]
    bad = L.copy()
    bad[r, c] = L[r, c] + ((L2k * Dk) @ L1k.T) @ np.linalg.inv(L[c, c]).T / D[c][None, :]
    assert ldl_elementwise_ratio(K, bad, D) >= MARGIN
    Kd, Dg = tiled_factor_image(bad, D)
    assert _solves(Q, A, sigma, dw, K, Kd, Dg) >= MARGIN


def test_a_factor_rounded_to_float32_fails():
    Q, A, sigma, dw, K = _problem()
    L, D = ldl_numpy(K.astype(np.float64))
    bad = L.astype(np.float32).astype(np.float64)
    assert ldl_elementwise_ratio(K, bad, D) >= MARGIN
    Kd, Dg = tiled_factor_image(bad, D)
    assert _solves(Q, A, sigma, dw, K, Kd, Dg) >= MARGIN


@pytest.mark.parametrize("tile", [(1, 0), (3, 2)])
def test_a_transposed_copy_that_is_not_L_transposed_in_one_tile_fails(tile):
    Q, A, sigma, dw, K = _problem()
    L, D = ldl_numpy(K.astype(np.float64))
    Kd, Dg = tiled_factor_image(L, D)
    bi, bj = tile
    # the copy of tile (bi, bj) never stored: its place keeps the assembled K, as the upper triangle holds before the factorization
    ld = Kd.shape[0]
    Kfull = np.eye(ld)
    Kfull[:N, :N] = K.astype(np.float64)
    rows, cols = slice(64 * bj, 64 * bj + 64), slice(64 * bi, 64 * bi + 64)
    Kd[rows, cols] = Kfull[rows, cols]
    assert transposed_copy_mismatch(Kd) > 0
    L2, D2 = factor_from_image(Kd, Dg, N)
    assert ldl_elementwise_ratio(K, L2, D2) <= 1.0          # L itself is right: only the copy check and the solves see it
    assert _solves(Q, A, sigma, dw, K, Kd, Dg) >= MARGIN


def test_the_devices_blocked_scheme_is_normwise_not_componentwise_accurate_on_solver_like_matrices():
    """why tests/test_gpu_direct_solvers.py holds the solver-like family to the normwise factor bound: with weights 1e9 / 0 / 1e-2 against
    sigma = 1e-7 (cond(K) ~ 1e11), panels formed with the explicit inverse of the diagonal block -- as the device does -- miss the
    componentwise bound by orders of magnitude, while a plain LDL' meets it; both meet the normwise one"""
    from test_gpu_direct_solvers import matrix
    Q, A, sigma, dw = matrix("solver", 319)
    K = newton_matrix(Q, A, sigma, dw)
    L, D = ldl_numpy(K.astype(np.float64))
    Lb, Db = blocked_ldl_with_inverse(K.astype(np.float64))
    assert ldl_elementwise_ratio(K, L, D) <= 1.0 and ldl_normwise_ratio(K, L, D) <= 1.0
    assert ldl_elementwise_ratio(K, Lb, Db) >= MARGIN
    assert ldl_normwise_ratio(K, Lb, Db) <= 1.0
