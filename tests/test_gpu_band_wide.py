"""The band direct solver for half-bandwidths 128 .. 1023 (dev/band_wide.inc): the band as 64 x 64 tiles, a right-looking LDL' on the
fp64 matrix cores with two launches per block column, both triangular solves in one launch.  As a linear solver it is held to the bounds
of the narrow band and the dense solvers on the same matrix family (tests/test_gpu_direct_solvers.py): |K - L D L'| <= 4 n u |L| |D| |L'|
elementwise on the downloaded factor, a backward error <= 4 n u for every right-hand side, D > 0, exact zeros outside the band, the same
bits from the same call twice.  As the solver of whole QPs (QPDO_LINSOLVE=band) it follows the CPU oracle like the other direct solvers.
tests/test_band_wide_cpu.py shows on the CPU that the two bounds catch a dropped tile, a missing D and a wrong tile count."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_wide_ref as bw
from helpers import ITERATE_RTOL, U64, assert_same_trace, backward_error, close_vec, ldl_elementwise_ratio, newton_matrix
from oracle import binding as ob
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QPDO_LINSOLVE", "QPDO_DENSE_MID", "QPDO_DENSE_LOOKAHEAD", "QPDO_DENSE_SOLVE", "QPDO_DENSE_LOWRANK", "QPDO_HYBRID",
            "QPDO_DENSE_MAX_N", "QPDO_SMALL_FUSED", "QPDO_PCG_MAXIT", "QPDO_PCG_DENSE_FALLBACK", "QPDO_PCG_SCHUR")


def _clean(monkeypatch, linsolve=None):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if linsolve:
        monkeypatch.setenv("QPDO_LINSOLVE", linsolve)


def _full_Q(p):
    Ql = sp.csr_matrix(p["Q"])
    return (Ql + sp.tril(Ql, -1).T).tocsr()


def _linear_workspace(p):
    return solver.QPDO().setup(p["Q"], np.zeros(p["n"]), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)


# ---- 1. factor and solves as a linear solver ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("b", [128, 129, 191, 192, 193])
def test_wide_band_factor_and_solves(b, which, gpu_required, monkeypatch):
    n = bw.orders(b)[which]
    p = problems.banded_random_qp(300 + b, n, b)
    Qf, A = _full_Q(p), sp.csr_matrix(p["A"])
    dw = 0.1 + 9.9 * np.random.default_rng(b + n).random(p["m"])
    sigma = 1.0
    _clean(monkeypatch, "band")
    ws = _linear_workspace(p)
    try:
        assert ws.stats()["linsolve"] == 3
        s0 = ws.stats()
        bs = bw.rhs_set(Qf, A, sigma, dw, n)
        xs = [ws.direct_solve(dw, sigma, r, refactor=True) for r in bs]
        g = ws.factor_geometry()
        assert g["b"] == b and g["np"] == (n + 63) // 64 * 64, g
        Wb, Wd = ws.download_factor("Wb"), ws.download_factor("Wd")
        x_again = ws.direct_solve(dw, sigma, bs[0], refactor=True)
        assert np.array_equal(x_again.view(np.uint64), xs[0].view(np.uint64))
        assert np.array_equal(ws.download_factor("Wb").view(np.uint64), Wb.view(np.uint64))
        d = ws.stats()["factor_count"] - s0["factor_count"]
        assert d == 4, d
        x_kept = ws.direct_solve(dw, sigma, bs[1], refactor=False)           # the kept factor, the solve on its own
        assert np.array_equal(x_kept.view(np.uint64), xs[1].view(np.uint64))
        assert ws.stats()["factor_count"] - s0["factor_count"] == 4
    finally:
        ws.delete()
    assert Wb.shape == (g["np"] // 64, (b + 63) // 64 + 1, 64, 64)
    assert bw.outside_band_nonzeros(Wb, b) == 0
    L, D = bw.unpack(Wb, Wd, n, b)
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    assert np.all(np.isfinite(L)) and np.all(np.diag(L) == 1.0) and np.all(Wd[n:] == 1.0)
    K = newton_matrix(Qf, A, sigma, dw)
    elem = ldl_elementwise_ratio(K, L, D)
    eta = max(backward_error(Qf, A, sigma, dw, x, r, K=K) for x, r in zip(xs, bs)) / (n * U64)
    print("wide band b=%d n=%d: elementwise %.3g, eta / (n u) %.3g" % (b, n, elem, eta))
    assert elem <= 1.0, elem
    assert eta <= 4.0, eta


# ---- 2. the widest bands: solves only --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [512, 1023])
def test_widest_band_solves(b, gpu_required, monkeypatch):
    n = 4 * (b + 1) + 37
    p = problems.banded_random_qp(400 + b, n, b)
    Qf, A = _full_Q(p), sp.csr_matrix(p["A"])
    dw = 0.1 + 9.9 * np.random.default_rng(b).random(p["m"])
    _clean(monkeypatch, "band")
    ws = _linear_workspace(p)
    try:
        assert ws.stats()["linsolve"] == 3
        bs = bw.rhs_set(Qf, A, 1.0, dw, n)
        xs = [ws.direct_solve(dw, 1.0, bs[0], refactor=True)] + [ws.direct_solve(dw, 1.0, r, refactor=False) for r in bs[1:]]
        g = ws.factor_geometry()
        assert g["b"] == b and g["np"] == (n + 63) // 64 * 64, g
        Wd = ws.download_factor("Wd")
    finally:
        ws.delete()
    assert np.all(np.isfinite(Wd)) and np.all(Wd > 0)
    eta = max(backward_error(Qf, A, 1.0, dw, x, r) for x, r in zip(xs, bs)) / (n * U64)
    print("wide band b=%d n=%d: eta / (n u) %.3g" % (b, n, eta))
    assert eta <= 4.0, eta


# ---- 3. whole solves against the oracle ------------------------------------------------------------------------------------------------------
def oracle_run(p, **st):
    o = ob.OracleSolver(p, ob.default_settings(**st))
    ro = o.solve(); tr = o.trace(); o.close()
    return ro, tr


def check(r, ro, tro, p):
    gi, oi = r["info"], ro["info"]
    assert (gi["status_val"], gi["iterations"], gi["oterations"]) == (oi["status_val"], oi["iterations"], oi["oterations"]), (gi, oi)
    assert_same_trace(r["trace"], tro)
    assert close_vec(r["x"], ro["x"], ITERATE_RTOL) and close_vec(r["y"], ro["y"], ITERATE_RTOL)
    rp, rd = problems.kkt_residuals(p, r["x"], r["y"])
    assert abs(rp - gi["res_prim_norm"]) <= 1e-9 and abs(rd - gi["res_dual_norm"]) <= 1e-9


@pytest.mark.parametrize("seed,n,bwid,win", [(428, 516, 128, None), (429, 521, 129, 130), (492, 835, 192, None), (600, 2048, 300, 64)])
def test_wide_band_solver_matches_the_oracle(seed, n, bwid, win, gpu_required, monkeypatch):
    p = problems.banded_random_qp(seed, n, bwid, win=win)
    _clean(monkeypatch, "band")
    r = solver.solve_problem(p, verbose=0)
    assert r["stats"]["linsolve"] == 3 and r["stats"]["factor_count"] > 0 and r["stats"]["lin_iters"] == 0 and r["stats"]["band_fallbacks"] == 0
    ro, tro = oracle_run(p)
    assert ro["info"]["status_val"] == 1
    check(r, ro, tro, p)
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    rd = solver.solve_problem(p, verbose=0)
    assert rd["stats"]["linsolve"] == 1
    assert np.abs(r["x"] - rd["x"]).max() <= 1e-9 * max(1.0, np.abs(rd["x"]).max())


# ---- 4. selection ----------------------------------------------------------------------------------------------------------------------------
def test_wide_band_selection_rules(gpu_required, monkeypatch):
    _clean(monkeypatch)
    p = problems.banded_random_qp(7, 2400, 128, win=4)
    # the automatic rule is unchanged: half-bandwidth 128 takes the dense solver
    assert solver.solve_problem(p, verbose=0, max_iter=5)["stats"]["linsolve"] == 1
    # asked for, the same instance takes the band solver
    monkeypatch.setenv("QPDO_LINSOLVE", "band")
    assert solver.solve_problem(p, verbose=0, max_iter=5)["stats"]["linsolve"] == 3
    # a matrix that is not banded: setup fails, and the message names the cap
    with pytest.raises(RuntimeError) as e:
        solver.solve_problem(problems.random_qp(3, 2500, 3000, 0.01), verbose=0)
    assert "1023" in str(e.value), str(e.value)
    # the narrow arrays do not exist on a wide workspace
    ws = _linear_workspace(p)
    try:
        ws.direct_solve(np.ones(p["m"]), 1.0, np.ones(p["n"]), refactor=True)
        with pytest.raises(RuntimeError):
            ws.download_factor("Kb")
        with pytest.raises(RuntimeError):
            ws.download_factor("Lt")
        assert ws.download_factor("Wd").shape == (2432,)
    finally:
        ws.delete()


# ---- 5. a bad pivot ----------------------------------------------------------------------------------------------------------------------------
def test_singular_wide_banded_matrix_is_latched_and_handed_to_another_solver(gpu_required, monkeypatch):
    """banded_qp's second-difference Q is singular along constants; with proximal = 0 and bounds so wide that no row is active in the
    first pass the first Newton matrix is Q itself, whose last pivot is exactly zero.  One extra row over columns 100 and 229 (never
    active: its weight is zero in every pass) makes the pattern's half-bandwidth 129, so the matrix goes through the tiled kernels:
    workgroup 0 of the last panel launch latches the pivot, the pass is redone by the dense solver -- the outcome of asking for it outright."""
    n = 2304
    p = problems.banded_qp(9, n, box=1e3, rate=1e3)
    extra = sp.csc_matrix(([1.0, 1.0], ([0, 0], [100, 229])), shape=(1, n))
    A = sp.vstack([sp.csc_matrix(p["A"]), extra]).tocsc()
    A.sort_indices()
    p = dict(p, A=A, m=p["m"] + 1, l=np.concatenate([p["l"], [-1e6]]), u=np.concatenate([p["u"], [1e6]]))
    _clean(monkeypatch, "band")
    r = solver.solve_problem(p, verbose=0, proximal=0, max_iter=60)
    assert r["stats"]["band_fallbacks"] == 1 and r["stats"]["linsolve"] == 1, r["stats"]
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    r1 = solver.solve_problem(p, verbose=0, proximal=0, max_iter=60)
    assert r["info"]["status_val"] == r1["info"]["status_val"] and r["info"]["iterations"] == r1["info"]["iterations"]
    # with the proximal term the same instance never meets a bad pivot
    monkeypatch.setenv("QPDO_LINSOLVE", "band")
    r2 = solver.solve_problem(p, verbose=0)
    assert r2["stats"]["band_fallbacks"] == 0 and r2["stats"]["linsolve"] == 3 and r2["info"]["status_val"] == 1


# ---- 6. the rescue above the dense limit -----------------------------------------------------------------------------------------------------
def test_pcg_above_the_dense_limit_is_rescued_by_the_wide_band_solver(gpu_required, monkeypatch):
    p = problems.banded_random_qp(640, 40064, 128, win=8)
    _clean(monkeypatch, "band")
    ref = solver.solve_problem(p, verbose=0)
    assert ref["stats"]["linsolve"] == 3 and ref["info"]["status_val"] == 1
    rp, rd = problems.kkt_residuals(p, ref["x"], ref["y"])
    assert rp <= 1e-6 and rd <= 1e-6 and abs(rp - ref["info"]["res_prim_norm"]) <= 1e-9 and abs(rd - ref["info"]["res_dual_norm"]) <= 1e-9
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_MAXIT", "3")
    # (the cap governs the Jacobi-preconditioned iteration; the Schur-complement mode, which this instance would take, has an inner cap
    # of its own and solves every pass: off, so that the first Newton solve ends at the cap far above 1e-8)
    monkeypatch.setenv("QPDO_PCG_SCHUR", "0")
    r = solver.solve_problem(p, verbose=0)
    st = r["stats"]
    assert st["pcg_rescues"] == 1 and (st["pcg_rescue_kinds"] & 1) and st["linsolve"] == 3, st
    assert (r["info"]["status_val"], r["info"]["iterations"], r["info"]["oterations"]) == \
           (ref["info"]["status_val"], ref["info"]["iterations"], ref["info"]["oterations"])
    assert close_vec(r["x"], ref["x"], 1e-8) and close_vec(r["y"], ref["y"], 1e-8)


# ---- 7. sequences on one workspace -----------------------------------------------------------------------------------------------------------
def test_wide_band_solver_sequences(gpu_required, monkeypatch):
    """warm start, update_bounds, update_q, update_settings and update_matrices on one wide workspace, a solve after each: bit for bit what
    a twin workspace given the same calls computes, with the band solver throughout and a kept factor never reused across an update"""
    _clean(monkeypatch, "band")
    p = problems.banded_random_qp(77, 640, 130, win=40)
    rng = np.random.default_rng(7)
    Q2 = sp.csc_matrix(p["Q"]).copy(); Q2.data = Q2.data * (1.0 + 0.01 * rng.random(Q2.nnz))
    Q2 = (Q2 + sp.diags(np.full(p["n"], 0.5))).tocsc()
    A2 = sp.csc_matrix(p["A"]).copy(); A2.data = A2.data * (1.0 + 0.01 * rng.random(A2.nnz))
    q2 = p["q"] * 1.1 + 0.05
    l2, u2 = p["l"] - 0.05, p["u"] + 0.02

    def run():
        s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
        out = []
        try:
            r = s.solve(); out.append((r, s.trace(), s.stats()))
            s.warm_start(r["x"], r["y"]); r = s.solve(); out.append((r, s.trace(), s.stats()))
            s.update_bounds(l2, u2); r = s.solve(); out.append((r, s.trace(), s.stats()))
            s.update_q(q2); r = s.solve(); out.append((r, s.trace(), s.stats()))
            s.update_settings(eps_abs=1e-8); r = s.solve(); out.append((r, s.trace(), s.stats()))
            s.update_matrices(Q=Q2, A=A2); r = s.solve(); out.append((r, s.trace(), s.stats()))
            g = s.factor_geometry()
            assert g["b"] == 130 and g["np"] == 640
        finally:
            s.delete()
        return out

    a, b = run(), run()
    assert len(a) == len(b) == 6
    for (ra, ta, sa), (rb, tb, sb) in zip(a, b):
        assert sa["linsolve"] == 3 and sa["band_fallbacks"] == 0
        assert ra["info"]["status_val"] == 1, ra["info"]
        assert (ra["info"]["status_val"], ra["info"]["iterations"], ra["info"]["oterations"]) == \
               (rb["info"]["status_val"], rb["info"]["iterations"], rb["info"]["oterations"])
        assert np.array_equal(ra["x"].view(np.uint64), rb["x"].view(np.uint64)) and np.array_equal(ra["y"].view(np.uint64), rb["y"].view(np.uint64))
        assert [t["tau"] for t in ta] == [t["tau"] for t in tb] and sa["factor_count"] == sb["factor_count"]
    # the last solve is the solve of the updated problem: KKT residuals recomputed from the new data
    pn = dict(p, Q=Q2, A=A2, q=q2, l=l2, u=u2)
    rp, rd = problems.kkt_residuals(pn, a[-1][0]["x"], a[-1][0]["y"])
    assert rp <= 1e-6 and rd <= 1e-6
