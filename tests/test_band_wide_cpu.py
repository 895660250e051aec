"""The checks of tests/test_gpu_band_wide.py, shown on the CPU (no GPU needed): a numpy restatement of the tiled band LDL'
(tests/band_wide_ref.py: 64-blocks, panels formed with the explicit inverse of the diagonal block, right-looking updates restricted to the
band) meets the two bounds the device's factor is held to on the same matrix family -- |K - L D L'| <= 4 n u |L| |D| |L'| elementwise and
a backward error of every solve <= 4 n u --, its fill never leaves the band, the Wb / Wd image round-trips exactly, and three deliberately
wrong variants (the last tile of a block column dropped from the update, D not applied in the update, w computed as b // 64) each miss a
bound by three orders of magnitude or more."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_wide_ref as bw
from helpers import U64, backward_error, ldl_elementwise_ratio, newton_matrix
from qpdo_amd import problems


def family(b, n):
    """the matrices of the factor test: banded_random_qp, weights 0.1 + 9.9 U(0, 1), sigma = 1"""
    p = problems.banded_random_qp(300 + b, n, b)
    Ql = sp.csr_matrix(p["Q"])
    Qf, A = (Ql + sp.tril(Ql, -1).T).tocsr(), sp.csr_matrix(p["A"])
    dw = 0.1 + 9.9 * np.random.default_rng(b + n).random(p["m"])
    return Qf, A, 1.0, dw


CASES = [(b, n) for b in (128, 129, 191, 192, 193) for n in (bw.orders(b)[0], bw.orders(b)[2])]


def test_geometry_and_orders():
    assert bw.geometry(516, 128) == (576, 9, 2) and bw.geometry(520, 129) == (576, 9, 3) and bw.geometry(768, 191)[2] == 3
    assert bw.geometry(772, 192)[2] == 3 and bw.geometry(776, 193)[2] == 4 and bw.geometry(4133, 1023) == (4160, 65, 16)
    assert bw.orders(128) == [516, 517, 575, 576] and bw.orders(191) == [768, 769, 831, 832]


@pytest.mark.parametrize("b,n", CASES)
def test_model_meets_both_bounds_and_keeps_the_band(b, n):
    Qf, A, sigma, dw = family(b, n)
    K = newton_matrix(Qf, A, sigma, dw)
    L, D, invs = bw.blocked_band_ldl(K.astype(np.float64), b)
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    i, j = np.indices((n, n))
    assert np.count_nonzero(L[(i - j > b) | (i < j)]) == 0                   # fill never leaves the band
    assert ldl_elementwise_ratio(K, L, D) <= 1.0
    bs = bw.rhs_set(Qf, A, sigma, dw, n)
    eta = max(backward_error(Qf, A, sigma, dw, bw.blocked_band_solve(L, D, invs, b, r), r, K=K) for r in bs) / (n * U64)
    assert eta <= 4.0, eta
    # the image: exact round trip, zeros where the layout promises them
    Wb, Wd = bw.pack(L, D, b)
    assert bw.outside_band_nonzeros(Wb, b) == 0
    L2, D2 = bw.unpack(Wb, Wd, n, b)
    assert np.array_equal(L2.view(np.uint64), L.view(np.uint64)) and np.array_equal(D2.view(np.uint64), D.view(np.uint64))
    npad = bw.geometry(n, b)[0]
    assert np.all(Wd[n:] == 1.0) and all(Wb[q // 64, 0, q % 64, q % 64] == 1.0 for q in range(n, npad))


def test_outside_band_check_sees_a_stray_entry():
    b, n = 129, 520
    Wb, Wd = bw.pack(np.eye(n), np.ones(n), b)
    assert bw.outside_band_nonzeros(Wb, b) == 0
    Wb[2, 3, 0, 63] = 1e-300                                                # element (63, 0) of tile (5, 2): i - j = 255 > b
    Wb[8, 1, 5, 5] = 1.0                                                    # a tile below the matrix
    Wb[0, 0, 7, 3] = 1.0                                                    # above the diagonal
    assert bw.outside_band_nonzeros(Wb, b) == 3


@pytest.mark.parametrize("variant,b", [("drop_last_tile", 128), ("drop_last_tile", 193), ("no_D", 129), ("w_floor", 129), ("w_floor", 191)])
def test_wrong_variants_miss_a_bound_by_three_orders(variant, b):
    n = bw.orders(b)[2]
    Qf, A, sigma, dw = family(b, n)
    K = newton_matrix(Qf, A, sigma, dw)
    L, D, invs = bw.blocked_band_ldl(K.astype(np.float64), b, variant=variant)
    elem = ldl_elementwise_ratio(K, L, D)
    r = bw.rhs_set(Qf, A, sigma, dw, n)[0]
    eta = backward_error(Qf, A, sigma, dw, bw.blocked_band_solve(L, D, invs, b, r), r, K=K) / (n * U64)
    assert elem >= 1e3 or not np.isfinite(elem), elem
    assert eta >= 4e3 or not np.isfinite(eta), eta
