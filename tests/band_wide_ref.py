"""A numpy restatement of the tiled band LDL' of dev/band_wide.inc (half-bandwidths 128 .. 1023) and of its storage, for
tests/test_band_wide_cpu.py and tests/test_gpu_band_wide.py.

Geometry: np = n rounded up to 64, nbc = np / 64 block columns, w = (b + 63) // 64 tiles below the diagonal one.
Storage (qpdo_amd_download_factor, arrays 7 and 8): Wb[J, s, c, r] = element (r, c) of tile (J + s, J) of the unit-lower L (diagonal tiles:
1 on the diagonal, 0 above it; identity padding behind n; tiles whose block row is >= nbc are zero), Wd = D padded with ones.
Scheme: right-looking over the block columns; the diagonal tile is factored, the panel tiles are A L_kk^-T / D with the EXPLICIT inverse
of the unit-lower diagonal block, and only the tiles (k + i, k + j), 1 <= j <= i <= w, are updated -- everything else lies outside the
band."""
import numpy as np

from helpers import ldl_numpy, newton_residual

T = 64


def geometry(n, b):
    npad = (n + T - 1) // T * T
    return npad, npad // T, (b + T - 1) // T


def pack(L, D, b):
    """the Wb / Wd image of a unit-lower L (n x n, zero outside the band) and D"""
    n = L.shape[0]
    npad, nbc, w = geometry(n, b)
    Lp = np.eye(npad)
    Lp[:n, :n] = np.tril(L)
    Wb = np.zeros((nbc, w + 1, T, T))
    for J in range(nbc):
        for s in range(min(w, nbc - 1 - J) + 1):
            Wb[J, s] = Lp[(J + s) * T:(J + s + 1) * T, J * T:(J + 1) * T].T
    Wd = np.ones(npad)
    Wd[:n] = D
    return Wb, Wd


def unpack(Wb, Wd, n, b):
    """L (unit lower, n x n) and D from the image"""
    npad, nbc, w = geometry(n, b)
    assert Wb.shape == (nbc, w + 1, T, T) and Wd.shape == (npad,)
    Lp = np.zeros((npad, npad))
    for J in range(nbc):
        for s in range(min(w, nbc - 1 - J) + 1):
            Lp[(J + s) * T:(J + s + 1) * T, J * T:(J + 1) * T] = Wb[J, s].T
    return Lp[:n, :n].copy(), np.asarray(Wd[:n], np.float64).copy()


def outside_band_nonzeros(Wb, b):
    """entries of the image that must be exact zeros and are not: i - j > b, above the diagonal, tiles below the matrix"""
    nbc, w1 = Wb.shape[:2]
    bad = 0
    r, c = np.arange(T)[None, :], np.arange(T)[:, None]          # Wb[J, s][c, r]
    for J in range(nbc):
        for s in range(w1):
            d = s * T + r - c                                     # i - j of element (r, c) of tile (J + s, J)
            must = (d > b) | (d < 0) | (J + s >= nbc)
            bad += int(np.count_nonzero(Wb[J, s][must]))
    return bad


def blocked_band_ldl(K, b, variant=None):
    """the tiled scheme on a dense symmetric K (float64) of half-bandwidth b.  Returns L, D, and the list of the diagonal blocks' inverses.
    variant: None, or one of the deliberately wrong ones -- "drop_last_tile" (the last tile of a block column left out of the update),
    "no_D" (D not applied in the update), "w_floor" (w = b // 64)."""
    n = K.shape[0]
    npad, nbc, w = geometry(n, b)
    if variant == "w_floor":
        w = b // T
    A = np.eye(npad)
    A[:n, :n] = np.asarray(K, np.float64)
    L, D, invs = np.eye(npad), np.ones(npad), []
    blk = lambda i: slice(i * T, (i + 1) * T)
    for k in range(nbc):
        Lkk, Dk = ldl_numpy(A[blk(k), blk(k)])
        inv = np.linalg.inv(Lkk)
        invs.append(inv)
        L[blk(k), blk(k)], D[blk(k)] = Lkk, Dk
        wk = min(w, nbc - 1 - k)
        for s in range(1, wk + 1):
            L[blk(k + s), blk(k)] = (A[blk(k + s), blk(k)] @ inv.T) / Dk[None, :]
        top = wk - 1 if (variant == "drop_last_tile" and wk == w) else wk
        for i in range(1, top + 1):
            for j in range(1, i + 1):
                Li = L[blk(k + i), blk(k)] if variant == "no_D" else L[blk(k + i), blk(k)] * Dk[None, :]
                A[blk(k + i), blk(k + j)] -= Li @ L[blk(k + j), blk(k)].T
    return L[:n, :n].copy(), D[:n].copy(), invs


def blocked_band_solve(L, D, invs, b, rhs):
    """both sweeps the way k_bw_solve makes them: z_J = L_JJ^-1 (r_J - sum_s L_{J,J-s} z_{J-s}), / D, and the mirror image"""
    n = L.shape[0]
    npad, nbc, w = geometry(n, b)
    Lp = np.eye(npad)
    Lp[:n, :n] = L
    Dp = np.ones(npad)
    Dp[:n] = D
    blk = lambda i: slice(i * T, (i + 1) * T)
    r = np.zeros(npad)
    r[:n] = rhs
    z = np.zeros(npad)
    for J in range(nbc):
        t = r[blk(J)].copy()
        for s in range(1, min(w, J) + 1):
            t -= Lp[blk(J), blk(J - s)] @ z[blk(J - s)]
        z[blk(J)] = invs[J] @ t
    y = z / Dp
    x = np.zeros(npad)
    for J in range(nbc - 1, -1, -1):
        t = y[blk(J)].copy()
        for s in range(1, min(w, nbc - 1 - J) + 1):
            t -= Lp[blk(J + s), blk(J)].T @ x[blk(J + s)]
        x[blk(J)] = invs[J].T @ t
    return x[:n]


def rhs_set(Qfull, A, sigma, dw, n, seed=5):
    """a random right-hand side, e_1, and K x_true"""
    rng = np.random.default_rng(seed)
    xt = rng.standard_normal(n)
    r, _ = newton_residual(Qfull, A, sigma, dw, xt, np.zeros(n))
    e1 = np.zeros(n)
    e1[0] = 1.0
    return [rng.standard_normal(n), e1, (-r).astype(np.float64)]


def orders(b):
    """the orders of the factor test: the smallest the band solver accepts, the next one, and the two around the next multiple of 64"""
    n0 = 4 * (b + 1)
    M = ((n0 + 1) // T + 1) * T
    return [n0, n0 + 1, M - 1, M]
