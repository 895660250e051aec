"""Plain numpy / scipy reference of the pieces of the PCG linear-solve path (dev/host_pcg.inc, dev/pcg_kernels.inc, the compaction kernels
of dev/spmv.inc), the checks that tests/test_gpu_pcg_pieces.py applies to what the device returns (qpdo_amd_pcg_probe,
qpdo_amd_download_compact), and the test systems both share.  tests/test_pcg_checks_cpu.py shows on the CPU that every check passes on
the reference's own output and fails on a mutant of it.

K = Q + sigma I + A' diag(dw) A.  A row is weighted when dw_i != 0.0 (-0.0 is not, a subnormal is).  Exact parts (index space, compact
matrices, slab tables) are integers and copied values: compared with np.array_equal.  Floating-point parts are compared with a
np.longdouble evaluation under bounds derived from the summation lengths, u = 2^-53."""
import numpy as np
import scipy.sparse as sp

from helpers import U64, newton_residual

PCG_TOL = 1e-12          # the device's default relative stopping tolerance (state.inc pcg_tol)
# c of the residual bound ||b - K x||_2 <= PCG_TOL ||b||_2 + c u ||K||_2 ||x||_2: twice the largest ratio of the fp64 reference CG below on
# the systems of solve_cases(), and at least 4 (tests/test_pcg_checks_cpu.py measures the reference's ratio and holds it to c / 2)
C_RESID = 4.0


def gamma(k):
    return k * U64 / (1.0 - k * U64)


# ---- the compact index space ------------------------------------------------------------------------------------------------------
def index_space(dw):
    """rows, cidx (weighted rows before row i), the flags as 64-bit words and cidx at the word starts"""
    dw = np.asarray(dw, np.float64)
    m = len(dw)
    flag = dw != 0.0
    rows = np.flatnonzero(flag).astype(np.int32)
    cidx = (np.cumsum(flag) - flag).astype(np.int32)
    words = (m + 63) // 64
    padded = np.zeros(words * 64, np.uint64)
    padded[:m] = flag
    bits = (padded.reshape(words, 64) << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64) if words else np.zeros(0, np.uint64)
    wprefix = np.concatenate([cidx, np.zeros(words * 64 - m, np.int32)])[::64][:words].astype(np.int32) if m else np.zeros(0, np.int32)
    return dict(rows=rows, cidx=cidx, flag_bits=bits, flag_wprefix=wprefix, k=len(rows), dc=dw[rows])


def _csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def compact_matrices(A, dw):
    """A_c = A[rows] and A_c' = CSR(A') restricted to the weighted columns, renumbered through cidx; (rp, ci, val) each"""
    A = _csr(A)
    ix = index_space(dw)
    rows = ix["rows"]
    Ac = A[rows] if len(rows) else sp.csr_matrix((0, A.shape[1]))
    Ac = _csr(Ac)
    arc = dict(nrows=len(rows), ncols=A.shape[1], rp=Ac.indptr.astype(np.int32), ci=Ac.indices.astype(np.int32), val=Ac.data.astype(np.float64))
    At = _csr(sp.csc_matrix(A).T)
    keep = (np.asarray(dw)[At.indices] != 0.0) if At.nnz else np.zeros(0, bool)
    csum = np.concatenate([[0], np.cumsum(keep)])
    atc = dict(nrows=A.shape[1], ncols=len(rows), rp=csum[At.indptr].astype(np.int32), ci=ix["cidx"][At.indices[keep]].astype(np.int32),
               val=At.data[keep].astype(np.float64))
    return ix, arc, atc


def slab_tables(rp, ci, nslabs, W):
    """ci mod W and sp[r, s] = first position of row r whose column is >= s W (sp[r, nslabs] = the row's end)"""
    nrows = len(rp) - 1
    spt = np.zeros((nrows, nslabs + 1), np.int32)
    row_of = np.repeat(np.arange(nrows), np.diff(rp))
    for s in range(nslabs):
        below = np.zeros(nrows, np.int64)
        np.add.at(below, row_of, ci < s * W)         # rows are column-sorted: the count of smaller columns is the searchsorted position
        spt[:, s] = rp[:-1] + below
    spt[:, nslabs] = rp[1:]
    return (ci % W).astype(np.uint16), spt


def compaction_mismatch(got, ref_ix, ref_arc, ref_atc):
    """name and first index of the first array of the device's compact structures that is not bit for bit the reference's; None if all
    are.  got: dict with rowlist, cidx, dc, flag_bits, flag_wprefix, k and the matrices Arc / Atc (None when k = 0) as dicts"""
    def diff(name, a, b, as_bits=False):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return "%s: shape %s, expected %s" % (name, a.shape, b.shape)
        if as_bits:
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a.ravel() != b.ravel())[0])
            return "%s[%d] = %r, expected %r" % (name, i, a.ravel()[i], b.ravel()[i])
        return None
    if got["k"] != ref_ix["k"]:
        return "k = %d, expected %d" % (got["k"], ref_ix["k"])
    checks = [("rowlist", got["rowlist"], ref_ix["rows"], False), ("cidx", got["cidx"], ref_ix["cidx"], False), ("dc", got["dc"], ref_ix["dc"], True),
              ("flag_bits", got["flag_bits"], ref_ix["flag_bits"], False), ("flag_wprefix", got["flag_wprefix"], ref_ix["flag_wprefix"], False)]
    for name, M, R in (("Arc", got.get("Arc"), ref_arc), ("Atc", got.get("Atc"), ref_atc)):
        if ref_ix["k"] == 0:
            continue
        if M is None:
            return name + " is missing"
        if (M["nrows"], M["ncols"], M["nnz"]) != (R["nrows"], R["ncols"], len(R["ci"])):
            return "%s geometry %r" % (name, (M["nrows"], M["ncols"], M["nnz"]))
        checks += [(name + ".rp", M["rp"], R["rp"], False), (name + ".ci", M["ci"], R["ci"], False), (name + ".val", M["val"], R["val"], True)]
        if M.get("use_slab"):
            c16, spt = slab_tables(R["rp"], R["ci"], M["nslabs"], M["W"])
            if M["W"] % 64 or M["nslabs"] < 1 or M["nslabs"] * M["W"] < M["ncols"]:
                return "%s slab geometry nslabs = %d, W = %d for %d columns" % (name, M["nslabs"], M["W"], M["ncols"])
            checks.append((name + ".sp", M["sp"], spt, False))
            if M.get("ci16") is not None:
                checks.append((name + ".ci16", M["ci16"], c16, False))
    for c in checks:
        bad = diff(*c)
        if bad:
            return bad
    return None


# ---- K p, the diagonals ----------------------------------------------------------------------------------------------------------------
def _absvec(Qf, A, sigma, dw, p):
    """(|Q| + sigma I + |A|' diag(|dw|) |A|) |p| in longdouble"""
    r, _ = newton_residual(abs(sp.csr_matrix(Qf)), abs(sp.csr_matrix(A)), abs(sigma), np.abs(dw), np.abs(p), np.zeros(len(p)))
    return -r


def row_lengths(Qf, A):
    rq = int(np.diff(sp.csr_matrix(Qf).indptr).max()) if Qf.shape[0] else 0
    ra = int(np.diff(sp.csr_matrix(A).indptr).max()) if A.shape[0] else 0
    rat = int(np.diff(sp.csc_matrix(A).indptr).max()) if A.shape[0] and A.shape[1] else 0
    return rq, ra, rat


def K_product(Qf, A, sigma, dw, p):
    """K p in longdouble, the vector b = (|Q| + sigma I + |A|' D |A|) |p| and r = r_Q + r_A + r_A' + 4: |fl(K p) - K p| <= r u b per component
    (A p: gamma_rA; the weight: one rounding; the A' product: gamma_rA'; Q p + sigma p: gamma_(rQ + 1); the two additions)"""
    r, _ = newton_residual(Qf, A, sigma, dw, p, np.zeros(len(p)))
    return -r, _absvec(Qf, A, sigma, dw, p), sum(row_lengths(Qf, A)) + 4


def underflow_term(A, r):
    """below the normal range a rounding error is absolute, eta = 2^-1074 per operation, not relative: a product with a subnormal weight
    carries it, the A' product multiplies it by |A_ij| and sums it.  r max(1, max |A|) eta bounds that; it only matters where the
    relative bound itself is of that size (the subnormal weights of the tests)"""
    amax = float(abs(sp.csr_matrix(A)).max()) if sp.csr_matrix(A).nnz else 0.0
    return r * max(1.0, amax) * np.longdouble(5e-324)


def K_product_ratio(Kp, ref, absvec, r, eta=0.0):
    """max_j |Kp_j - ref_j| / (r u b_j + eta); a component whose bound is 0 must be exact (else inf).  eta: underflow_term"""
    err = np.abs(np.asarray(Kp, np.longdouble) - ref)
    bound = r * U64 * absvec + np.where(absvec > 0, np.longdouble(eta), 0)
    if np.any(err[bound == 0] != 0):
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def pKp_ratio(partials, p, ref, absvec, r):
    """|sum of the partials - p'Kp| / (gamma_(n + r) |p|' b): the error of Kp (r u b) through |p|, and a sum of n terms in any order"""
    n = len(p)
    pl = np.asarray(p, np.longdouble)
    bound = gamma(n + r) * (np.abs(pl) @ absvec)
    err = abs(np.sum(np.asarray(partials, np.longdouble)) - pl @ ref)          # (longdouble throughout: not rounded to fp64 first)
    return float(err / bound) if bound > 0 else (0.0 if err == 0 else float("inf"))


def jacobi_diagonal(Qf, A, sigma, dw):
    """Q_jj + sigma + sum_i A_ij^2 dw_i in longdouble, and the number of weighted entries of each column"""
    A = sp.csc_matrix(A)
    n = Qf.shape[0]
    q = np.asarray(sp.csr_matrix(Qf).diagonal(), np.longdouble) + np.longdouble(sigma)
    dwl = np.asarray(dw, np.longdouble)
    s = np.zeros(n, np.longdouble)
    cols = np.repeat(np.arange(n), np.diff(A.indptr))
    v = A.data.astype(np.longdouble)
    np.add.at(s, cols, v * v * dwl[A.indices])
    cnt = np.zeros(n, np.int64)
    np.add.at(cnt, cols, np.asarray(dw)[A.indices] != 0.0)
    return q + s, cnt


def schur_diagonals(Qf, A, sigma, dw):
    """Dq = Q_jj + sigma and Sd_i = 1 / d_i + sum_j A_ij^2 / Dq_j over the weighted rows (longdouble), and their row lengths"""
    A = _csr(A)
    dq = np.asarray(sp.csr_matrix(Qf).diagonal(), np.longdouble) + np.longdouble(sigma)
    rows = np.flatnonzero(np.asarray(dw) != 0.0)
    Ac = _csr(A[rows])
    v = Ac.data.astype(np.longdouble)
    s = np.zeros(len(rows), np.longdouble)
    np.add.at(s, np.repeat(np.arange(len(rows)), np.diff(Ac.indptr)), v * v / dq[Ac.indices])
    return dq, 1 / np.asarray(dw, np.longdouble)[rows] + s, np.diff(Ac.indptr)


def diagonal_ratio(got, ref, lengths):
    """max |got - ref| / ((length + 3) u ref): every term is non-negative, so the bound is relative to the sum itself"""
    err = np.abs(np.asarray(got, np.longdouble) - ref)
    bound = (np.asarray(lengths) + 3) * U64 * np.abs(ref)
    return float((err / bound).max()) if len(err) else 0.0


# ---- the solves ------------------------------------------------------------------------------------------------------------------------
def K_sparse(Qf, A, sigma, dw):
    A = sp.csr_matrix(A)
    return (sp.csr_matrix(Qf) + sigma * sp.identity(Qf.shape[0]) + A.T @ sp.diags(np.asarray(dw, np.float64)) @ A).tocsr()


def pcg(K, Minv, b, tol=PCG_TOL, maxit=100000):
    """textbook fp64 preconditioned CG with the device's stopping rule ||r||_2 <= tol ||b||_2 on the recursive residual, checked after
    every update; Minv: callable.  Returns x and the iteration count (0 for b = 0)."""
    x = np.zeros(len(b))
    bn = float(np.sqrt(b @ b))
    if bn == 0.0:
        return x, 0
    r = b.copy()
    z = Minv(r)
    p = z.copy()
    rz = r @ z
    for it in range(1, maxit + 1):
        Kp = K @ p
        alpha = rz / (p @ Kp)
        x += alpha * p
        r -= alpha * Kp
        if np.sqrt(r @ r) <= tol * bn:
            return x, it
        z = Minv(r)
        rz2 = r @ z
        p = z + (rz2 / rz) * p
        rz = rz2
    return x, maxit


def jacobi_pcg(Qf, A, sigma, dw, b, tol=PCG_TOL):
    K = K_sparse(Qf, A, sigma, dw)
    dg = np.asarray(jacobi_diagonal(Qf, A, sigma, dw)[0], np.float64)
    return pcg(K, lambda r: r / dg, b, tol)


def schur_pcg(Qf, A, sigma, dw, b, tol=PCG_TOL):
    """the outer iteration of the Schur-complement mode with its preconditioner M = Dq + A_c' D A_c applied exactly (sparse LU)"""
    import scipy.sparse.linalg as spla
    K = K_sparse(Qf, A, sigma, dw)
    A = sp.csr_matrix(A)
    M = (sp.diags(sp.csr_matrix(Qf).diagonal() + sigma) + A.T @ sp.diags(np.asarray(dw, np.float64)) @ A).tocsc()
    lu = spla.splu(M)
    return pcg(K, lu.solve, b, tol)


def norm2(K):
    import scipy.sparse.linalg as spla
    if K.shape[0] <= 2:
        return float(np.linalg.norm(K.toarray(), 2))
    return float(spla.eigsh(K, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0])


def residual_ratio(Qf, A, sigma, dw, x, b, knorm, tol=PCG_TOL):
    """(||b - K x||_2 - tol ||b||_2) / (u ||K||_2 ||x||_2) with the residual in longdouble: the c the bound would need (<= 0: none)"""
    r, _ = newton_residual(Qf, A, sigma, dw, x, b)
    rn = float(np.sqrt(np.sum(r * r)))
    bn, xn = float(np.linalg.norm(b)), float(np.linalg.norm(x))
    den = U64 * knorm * xn
    return (rn - tol * bn) / den if den > 0 else (0.0 if rn <= tol * bn else float("inf"))


def iterations_close(dev, ref):
    """Jacobi route: the same algorithm with the same preconditioner, only the summation order differs"""
    return abs(dev - ref) <= 2 + 0.02 * ref


# ---- test systems ------------------------------------------------------------------------------------------------------------------
def dominant_Q(rng, n, per_row=3, off=0.05):
    """symmetric, unit-order diagonal, |off-diagonal| row sums <= ~2 per_row off: strongly diagonally dominant"""
    if n == 1:
        return sp.csr_matrix(np.array([[1.5]]))
    B = sp.random(n, n, density=min(1.0, per_row / n), random_state=rng, format="csr", data_rvs=lambda s: off * rng.standard_normal(s))
    B = sp.triu(B, 1)
    B = B + B.T
    return _csr(B + sp.diags(1.0 + rng.random(n)))


def sparse_A(rng, m, n, per_row=3, empty_row=None):
    if m == 0:
        return sp.csr_matrix((0, n))
    A = sp.random(m, n, density=min(1.0, per_row / n), random_state=rng, format="lil", data_rvs=rng.standard_normal)
    if empty_row is not None and m > 2:
        A[empty_row, :] = 0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    return _csr(A)


def system(n, m, seed, per_row=3, empty_row=None):
    rng = np.random.default_rng(seed * 1009 + 7 * n + m)
    return dominant_Q(rng, n), sparse_A(rng, m, n, per_row, empty_row)


def weight_patterns(m, seed=0):
    """name -> dw.  Values in [0.1, 10] on the weighted rows unless the name says otherwise"""
    rng = np.random.default_rng(1000 + seed + m)
    val = 0.1 + 9.9 * rng.random(m)
    i = np.arange(m)

    def on(mask):
        return np.where(mask, val, 0.0)
    pats = {"none": np.zeros(m), "all": val.copy(), "row0": on(i == 0), "last": on(i == m - 1), "every64": on(i % 64 == 0),
            "words_alternate": on((i // 64) % 2 == 0), "random30": on(rng.random(m) < 0.3)}
    e = on(rng.random(m) < 0.2)
    if m > 2:
        e[m // 2] = 2.5                                     # the row that system(..., empty_row = m // 2) leaves without entries
    pats["empty_row_weighted"] = e
    z = on(rng.random(m) < 0.5)
    z[z == 0.0] = -0.0                                       # -0.0: not weighted
    pats["negative_zero"] = z
    s = on(rng.random(m) < 0.3)
    s[m // 3] = 5e-324                                       # a subnormal: weighted
    if m > 1:
        s[m - 1] = 2.0 ** -1040
    pats["subnormal"] = s
    late = np.zeros(m)                                       # late-pass family of the direct-solver tests (with sigma = 1e-7)
    r = rng.random(m)
    late[r < 0.4] = 1e9
    late[(r >= 0.4) & (r < 0.45)] = 1e-2
    pats["late_pass"] = late
    return pats


def probe_vectors(n, seed=3):
    rng = np.random.default_rng(seed + n)
    e1 = np.zeros(n)
    e1[0] = 1.0
    return {"random": rng.standard_normal(n), "e1": e1, "spread": rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)}


def k_weights(m, k, seed, lo=0.1, hi=10.0):
    """exactly k weighted rows, weights in [lo, hi]"""
    rng = np.random.default_rng(seed)
    dw = np.zeros(m)
    dw[rng.choice(m, k, replace=False)] = lo + (hi - lo) * rng.random(k)
    return dw


# name -> (n, m, k, environment, route): the solves of tests/test_gpu_pcg_pieces.py; tests/test_pcg_checks_cpu.py runs the reference on them
SOLVE_CASES = {
    "jacobi_k200": (400, 500, 200, {}, "jacobi"),
    "jacobi_k255": (400, 500, 255, {}, "jacobi"),
    "schur_k256": (400, 500, 256, {}, "schur"),
    "schur_k320": (400, 500, 320, {}, "schur"),                      # k = 0.8 n
    "jacobi_k321": (400, 500, 321, {}, "jacobi"),
    "jacobi_schur_off": (1000, 1200, 600, {"QPDO_PCG_SCHUR": "0"}, "jacobi"),
    "schur_k600": (1000, 1200, 600, {}, "schur"),
    "schur_k2000": (3000, 3600, 2000, {}, "schur"),
}


def solve_case(name):
    n, m, k, env, route = SOLVE_CASES[name]
    Qf, A = system(n, m, 11)
    dw = k_weights(m, k, 5 + k)
    return Qf, A, 1.0, dw, env, route


def deflation_case():
    """k = 1500 > 4 x 256 weighted rows (below that the host code does not deflate), 40 of them at 2^16 and the rest at 1"""
    n, m, k = 3000, 2500, 1500
    Qf, A = system(n, m, 13)
    rng = np.random.default_rng(17)
    rows = rng.choice(m, k, replace=False)
    dw = np.zeros(m)
    dw[rows] = 1.0
    dw[rows[:40]] = 2.0 ** 16
    return Qf, A, 1.0, dw


def solve_rhs(Qf, A, sigma, dw, seed=5):
    n = Qf.shape[0]
    rng = np.random.default_rng(seed)
    xt = rng.standard_normal(n)
    r, _ = newton_residual(Qf, A, sigma, dw, xt, np.zeros(n))
    e1 = np.zeros(n)
    e1[0] = 1.0
    return {"random": rng.standard_normal(n), "e1": e1, "K x_true": (-r).astype(np.float64), "zero": np.zeros(n)}


def deflation_threshold(dc):
    """the threshold dev/host_pcg.inc defl_build derives: rows above dmax / 2^(kb + 1), kb the last bucket of the power-of-two histogram
    whose cumulative count is still <= 256; None when nothing is deflated"""
    dc = np.asarray(dc, np.float64)
    dmax = dc.max()
    hist = np.zeros(32, np.int64)
    for v in dc[dc > 0]:
        b, t = 0, dmax
        while b < 31 and v <= t * 0.5:
            t *= 0.5
            b += 1
        hist[b] += 1
    cum, kb = 0, -1
    for b in range(32):
        if cum + hist[b] > 256:
            break
        cum += hist[b]
        kb = b
    if kb < 2 or cum == 0:
        return None
    return dmax * 2.0 ** -(kb + 1)


def deflation_S(A, dw, rows_compact, heavy, P):
    """S = D_h^-1 + A_h P^-1 A_h' (longdouble) for the heavy compact rows `heavy`; P: the remainder diagonal the device used"""
    A = _csr(A)
    Ah = A[np.asarray(rows_compact)[heavy]].toarray().astype(np.longdouble)
    Pl = np.asarray(P, np.longdouble)
    return np.diag(1 / np.asarray(dw, np.longdouble)[np.asarray(rows_compact)[heavy]]) + (Ah / Pl[None, :]) @ Ah.T
