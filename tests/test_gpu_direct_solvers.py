"""The direct solvers of the Newton system K dx = rhs, K = Q + sigma I + A' diag(d) A, tested as linear solvers (qpdo_amd_direct_solve,
qpdo_amd_download_factor) against K assembled in extended precision from the problem's sparse data (tests/helpers.py; scaling = 0, so
the device's matrices are the caller's).  Every case asserts D > 0 and finite, the transposed copy in the upper triangle of every
off-diagonal tile equal to L' bit for bit, LinvT = Linv' bit for bit, the elementwise bound |K - L D L'| <= 4 n u |L| |D| |L'| where the
factor is downloaded, a normwise backward error eta <= 4 n u for every right-hand side (random, e_1, K x_true), the same bits from the
same call twice, and the solver's counters.  tests/test_direct_solver_checks_cpu.py shows on the CPU that these checks catch a dropped
rank-64 contribution, a float32 factor and a wrong transposed copy by three orders of magnitude or more.

Largest measured ratios on the MI355X (test_zz_report prints them; every bound is <= 1 for the factor, eta <= 4 n u):
  dense, elementwise and solves (180 cases) ........ eta / (n u) 0.53, |K - L D L'| / (4 n u |L| |D| |L'|) 0.26
  dense, solver-like family (75 cases) ............. eta / (n u) 0.55, normwise factor ratio 0.12 (see run_dense_case)
  low-rank update (20 solves) ...................... eta / (n u) 0.0024
  band, elementwise and solves (24 cases) .......... eta / (n u) 0.043, elementwise 0.52
  dense n = 12289 .. 40000, solves only ............ eta / (n u) 2.8e-5;  band n = 2e5, b = 3: 2.7e-6
The whole file runs in about 20 s on the MI355X.
"""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import (U64, backward_error, factor_from_image, ldl_elementwise_ratio, ldl_normwise_ratio, newton_matrix,
                     transposed_copy_mismatch)
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QPDO_LINSOLVE", "QPDO_DENSE_MID", "QPDO_DENSE_LOOKAHEAD", "QPDO_DENSE_SOLVE", "QPDO_DENSE_LOWRANK", "QPDO_HYBRID",
            "QPDO_DENSE_MAX_N", "QPDO_SMALL_FUSED")
# route -> (environment at setup, carry the forward solve in the factorization launch, factorizations through k_mid_factor)
ROUTES = {
    "mid": ({}, False, True),
    "mid_fwd": ({}, True, True),
    "multi_la0": ({"QPDO_DENSE_MID": "0", "QPDO_DENSE_LOOKAHEAD": "0"}, False, False),
    "multi_la1": ({"QPDO_DENSE_MID": "0", "QPDO_DENSE_LOOKAHEAD": "1"}, False, False),
    "steps": ({"QPDO_DENSE_SOLVE": "steps"}, False, False),
}
# n = 1, 2 and one block; n mod 64 in {1, 15, 16, 17, 33, 48, 49, 63} (the partial sub-panel counts of the last diagonal block);
# more block rows than one outer panel; more tiles than resident workgroups
ORDERS = [1, 2, 63, 64, 65, 129, 207, 80, 273, 161, 240, 369, 319, 1008, 2088]
ORDERS_SHORT = [1, 64, 65, 145, 305, 1008, 2088]
REPORT = {}


def _note(group, eta_ratio, elem_ratio=None):
    g = REPORT.setdefault(group, {"eta/(n u)": 0.0, "elementwise": 0.0, "cases": 0})
    g["eta/(n u)"] = max(g["eta/(n u)"], eta_ratio)
    if elem_ratio is not None:
        g["elementwise"] = max(g["elementwise"], elem_ratio)
    g["cases"] += 1


def _workspace(monkeypatch, Qfull, A, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, m = Qfull.shape[0], A.shape[0]
    return solver.QPDO().setup(Qfull, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)


def _spd_Q(rng, n, diag_lo=1.0, off=0.3, density=None):
    density = min(1.0, 4.0 / n) if density is None else density
    B = sp.random(n, n, density=density, random_state=rng, format="csr") * off
    B = sp.triu(B, 1)
    B = B + B.T
    rs = np.asarray(abs(B).sum(axis=1)).ravel()
    return (B + sp.diags(rs + diag_lo + rng.random(n))).tocsr()


def matrix(kind, n, seed=1):
    """(Q full, A, sigma, dw) of one test family"""
    rng = np.random.default_rng(seed * 7919 + n)
    if kind == "well":            # sigma = 1, weights in [0.1, 10]
        m = max(2, n // 2 + 3)
        A = sp.random(m, n, density=min(1.0, 3.0 / n), random_state=rng, format="csr")
        return _spd_Q(rng, n), A, 1.0, 0.1 + 9.9 * rng.random(m)
    if kind == "solver":          # late-pass weights: 1/mu = 1e9 on the active rows, 0 elsewhere, 1e-2 on a few; sigma = 1e-7
        m = max(4, n)
        A = sp.random(m, n, density=min(1.0, 3.0 / n), random_state=rng, format="csr")
        dw = np.zeros(m)
        r = rng.random(m)
        dw[r < 0.4] = 1e9
        dw[(r >= 0.4) & (r < 0.45)] = 1e-2
        return _spd_Q(rng, n, diag_lo=1e-3, off=1e-3), A, 1e-7, dw
    if kind == "zerotiles":       # rows of A and Q confined to 64-blocks: whole tiles of K are zero
        m = max(2, n)
        rows, cols, vals = [], [], []
        for r in range(m):
            b0 = 64 * int(rng.integers(0, (n + 63) // 64))
            c = np.unique(rng.integers(b0, min(n, b0 + 64), 4))
            rows += [r] * len(c); cols += list(c); vals += list(rng.standard_normal(len(c)))
        A = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
        return sp.diags(1.0 + rng.random(n)).tocsr(), A, 1.0, 0.1 + 9.9 * rng.random(m)
    if kind == "nocon":           # m = 0
        return _spd_Q(rng, n), sp.csr_matrix((0, n)), 1.0, np.zeros(0)
    if kind == "dense":           # one dense row with a positive weight: K dense everywhere
        m = max(2, n // 4 + 1)
        A = sp.random(m - 1, n, density=min(1.0, 2.0 / n), random_state=rng, format="csr")
        A = sp.vstack([sp.csr_matrix(rng.standard_normal((1, n))), A]).tocsr()
        return _spd_Q(rng, n), A, 1.0, np.concatenate([[1.0], 0.1 + 9.9 * rng.random(m - 1)])
    raise KeyError(kind)


def rhs_set(Qfull, A, sigma, dw, n, seed=5):
    rng = np.random.default_rng(seed)
    xt = rng.standard_normal(n)
    r, _ = _residual_free_product(Qfull, A, sigma, dw, xt)
    e1 = np.zeros(n)
    e1[0] = 1.0
    return [rng.standard_normal(n), e1, r]


def _residual_free_product(Qfull, A, sigma, dw, x):
    from helpers import newton_residual
    r, kinf = newton_residual(Qfull, A, sigma, dw, x, np.zeros(len(x)))
    return (-r).astype(np.float64), kinf


def check_factor_storage(ws, n):
    """D > 0 and finite, the transposed copies, LinvT = Linv'; returns (L, D, Kd bits)"""
    g = ws.factor_geometry()
    assert g["ld"] == (n + 63) // 64 * 64 and g["nb"] == g["ld"] // 64, g
    Kd, Dg = ws.download_factor("Kd"), ws.download_factor("Dg")
    Li, LiT = ws.download_factor("Linv"), ws.download_factor("LinvT")
    assert np.all(np.isfinite(Dg[:n])) and np.all(Dg[:n] > 0), Dg[:n].min()
    assert transposed_copy_mismatch(Kd) == 0
    nb = g["nb"]
    assert np.array_equal(LiT.reshape(nb, 64, 64).view(np.uint64), Li.reshape(nb, 64, 64).transpose(0, 2, 1).view(np.uint64))
    assert np.all(np.isfinite(Kd[:n, :n]))
    L, D = factor_from_image(Kd, Dg, n)
    return L, D, Kd.copy()


def _stats_delta(a, b):
    return {k: b[k] - a[k] for k in ("factor_count", "onelaunch_factors", "chain_fallbacks", "lowrank_solves", "lowrank_rejects")}


def run_dense_case(monkeypatch, kind, n, route, group):
    env, carry, onelaunch = ROUTES[route]
    Qf, A, sigma, dw = matrix(kind, n)
    K = newton_matrix(Qf, A, sigma, dw)
    if kind == "solver" and n <= 400:
        ev = np.linalg.eigvalsh(K.astype(np.float64))
        assert ev[0] > 0 and ev[-1] / ev[0] < 1e14, ev[-1] / ev[0]          # (1e9 .. 6e11 at these orders: what late passes reach)
    ws = _workspace(monkeypatch, Qf, A, dict(env, QPDO_DENSE_LOWRANK="0"))
    try:
        s0 = ws.stats()
        bs = rhs_set(Qf, A, sigma, dw, n)
        xs = [ws.direct_solve(dw, sigma, b, refactor=True, carry_forward=carry) for b in bs]
        L, D, Kd = check_factor_storage(ws, n)
        Dg, Li = ws.download_factor("Dg"), ws.download_factor("Linv")
        x_again = ws.direct_solve(dw, sigma, bs[0], refactor=True, carry_forward=carry)
        assert np.array_equal(x_again.view(np.uint64), xs[0].view(np.uint64))
        # the factor's bits: L below the diagonal (its copies were checked against it), D, the diagonal blocks' inverses.  (The upper
        # triangle of a diagonal tile is scratch: the multi-launch trailing update writes whole tiles and the assembly rewrites the lower
        # triangle only, so it differs from one factorization to the next.)
        Kd_again = ws.download_factor("Kd")
        assert np.array_equal(np.tril(Kd_again, -1).view(np.uint64), np.tril(Kd, -1).view(np.uint64))
        assert np.array_equal(ws.download_factor("Dg").view(np.uint64), Dg.view(np.uint64))
        assert np.array_equal(ws.download_factor("Linv").view(np.uint64), Li.view(np.uint64))
        x_kept = ws.direct_solve(dw, sigma, bs[1], refactor=False)          # the kept factor, solves on their own
        d = _stats_delta(s0, ws.stats())
        assert d == {"factor_count": 4, "onelaunch_factors": 4 if onelaunch else 0, "chain_fallbacks": 0, "lowrank_solves": 0,
                     "lowrank_rejects": 0}, d
    finally:
        ws.delete()
    eta = max(backward_error(Qf, A, sigma, dw, x, b, K=K) for x, b in zip(xs + [x_kept], bs + [bs[1]])) / (n * U64)
    if kind == "solver":
        # Both factorizations form a panel as C L_jj^-T / D_j with the EXPLICIT inverse of the diagonal block, which is backward stable
        # normwise but not componentwise: on these matrices (D from 1e-3 to 1e9 inside one block) a numpy blocked LDL' that does the same
        # misses the componentwise bound by 1e5 .. 1e12 where the plain LDL' meets it at 0.01 (test_direct_solver_checks_cpu.py).  Here
        # the factor is held to the normwise form of the same bound.
        elem = ldl_normwise_ratio(K, L, D)
        _note(group + " (solver-like: normwise factor check)", eta, elem)
    else:
        elem = ldl_elementwise_ratio(K, L, D)
        _note(group, eta, elem)
    assert elem <= 1.0, elem
    assert eta <= 4.0, eta


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("kind", ["dense", "solver"])
def test_dense_factor_and_solves_every_order(kind, n, route, gpu_required, monkeypatch):
    run_dense_case(monkeypatch, kind, n, route, "dense elementwise + solves")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("n", ORDERS_SHORT)
@pytest.mark.parametrize("kind", ["well", "zerotiles", "nocon"])
def test_dense_factor_and_solves_other_matrices(kind, n, route, gpu_required, monkeypatch):
    run_dense_case(monkeypatch, kind, n, route, "dense elementwise + solves")


# ---- low-rank update of a kept factor (QPDO_DENSE_LOWRANK=1) ---------------------------------------------------------------------------
NLR = 1008


def lowrank_problem(seed=11):
    """m = 700 sparse rows + 2 rows that alone touch the last two columns (where Q is small): a weight of 1e9 there pins them"""
    rng = np.random.default_rng(seed)
    n, m0 = NLR, 700
    A0 = sp.random(m0, n - 2, density=4.0 / n, random_state=rng, format="csr")
    A0 = sp.hstack([A0, sp.csr_matrix((m0, 2))]).tocsr()
    pin = sp.csr_matrix(([1.0, 0.5, 0.5, -1.0], ([0, 0, 1, 1], [n - 2, n - 1, n - 2, n - 1])), shape=(2, n))
    A = sp.vstack([A0, pin]).tocsr()
    q = np.concatenate([1.0 + rng.random(n - 2), [1e-3, 1e-3]])
    Qf = sp.diags(q).tocsr()
    dw0 = 0.1 + 9.9 * rng.random(m0 + 2)
    return Qf, A, dw0, rng


def _lr_solve(ws, Qf, A, sigma, dw, n, refactor, group):
    bs = rhs_set(Qf, A, sigma, dw, n)
    eta = 0.0
    x0 = None
    for b in bs[:1] if not refactor else bs[:1]:
        x0 = ws.direct_solve(dw, sigma, b, refactor=refactor)
        eta = max(eta, backward_error(Qf, A, sigma, dw, x0, b) / (n * U64))
    _note(group, eta)
    assert eta <= 4.0, eta
    return x0


@pytest.mark.parametrize("k", [1, 5, 128, 129, 256, 257])
def test_lowrank_update_of_a_kept_factor(k, gpu_required, monkeypatch):
    Qf, A, dw0, rng = lowrank_problem()
    n, m = NLR, A.shape[0]
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_DENSE_LOWRANK": "1"})
    try:
        _lr_solve(ws, Qf, A, 1.0, dw0, n, True, "low-rank")
        rows = rng.choice(m - 2, k, replace=False)
        dw1 = dw0.copy()
        dw1[rows[: k // 2]] = 0.0                                            # downdates to 0
        dw1[rows[k // 2:]] *= 1.0 + 4.0 * rng.random(k - k // 2)             # updates
        s0 = ws.stats()
        bs = rhs_set(Qf, A, 1.0, dw1, n)
        xs = []
        for b in bs:
            xs.append(ws.direct_solve(dw1, 1.0, b, refactor=False))
        d = _stats_delta(s0, ws.stats())
        if k <= 256:
            # the first solve extends the slot set, the others reuse it: one low-rank solve each, no factorization
            assert d == {"factor_count": 0, "onelaunch_factors": 0, "chain_fallbacks": 0, "lowrank_solves": 3, "lowrank_rejects": 0}, d
        else:
            # more than WB_MAX = 256 rows moved: refactor, then the new factor serves the others as it is
            assert d["factor_count"] == 1 and d["lowrank_solves"] == 0 and d["lowrank_rejects"] == 0 and d["chain_fallbacks"] == 0, d
        x_again = ws.direct_solve(dw1, 1.0, bs[0], refactor=False)
        assert np.array_equal(x_again.view(np.uint64), xs[0].view(np.uint64))
    finally:
        ws.delete()
    eta = max(backward_error(Qf, A, 1.0, dw1, x, b) for x, b in zip(xs, bs)) / (n * U64)
    _note("low-rank", eta)
    assert eta <= 4.0, eta


@pytest.mark.parametrize("k1,k2", [(5, 7), (100, 60)])
def test_lowrank_slot_set_grows_across_calls(k1, k2, gpu_required, monkeypatch):
    Qf, A, dw0, rng = lowrank_problem(seed=12)
    n, m = NLR, A.shape[0]
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_DENSE_LOWRANK": "1"})
    try:
        _lr_solve(ws, Qf, A, 1.0, dw0, n, True, "low-rank")
        rows = rng.choice(m - 2, k1 + k2, replace=False)
        dw1 = dw0.copy(); dw1[rows[:k1]] *= 3.0
        dw2 = dw1.copy(); dw2[rows[k1:]] = 0.0
        s0 = ws.stats()
        _lr_solve(ws, Qf, A, 1.0, dw1, n, False, "low-rank")
        s1 = ws.stats()
        _lr_solve(ws, Qf, A, 1.0, dw2, n, False, "low-rank")                # k_old = k1 > 0
        s2 = ws.stats()
        assert _stats_delta(s0, s2) == {"factor_count": 0, "onelaunch_factors": 0, "chain_fallbacks": 0, "lowrank_solves": 2,
                                         "lowrank_rejects": 0}
        assert s1["lowrank_cols"] - s0["lowrank_cols"] == k1 and s2["lowrank_cols"] - s1["lowrank_cols"] == k2
    finally:
        ws.delete()


def test_lowrank_downdate_that_removes_a_direction_trips_the_pivot_guard(gpu_required, monkeypatch):
    Qf, A, dw0, rng = lowrank_problem(seed=13)
    n, m = NLR, A.shape[0]
    sigma = 1e-7
    dw0 = dw0.copy()
    dw0[m - 2] = 1e9                     # the only row on the last two columns: with Q = 1e-3 there, it alone pins them
    ws = _workspace(monkeypatch, Qf, A, {"QPDO_DENSE_LOWRANK": "1"})
    try:
        _lr_solve(ws, Qf, A, sigma, dw0, n, True, "low-rank")
        dw1 = dw0.copy()
        dw1[m - 2] = 0.0
        s0 = ws.stats()
        _lr_solve(ws, Qf, A, sigma, dw1, n, False, "low-rank")
        d = _stats_delta(s0, ws.stats())
        assert d["lowrank_rejects"] == 1 and d["lowrank_solves"] == 0 and d["factor_count"] == 1 and d["chain_fallbacks"] == 0, d
    finally:
        ws.delete()


# ---- band LDL' (QPDO_LINSOLVE=band) ----------------------------------------------------------------------------------------------------
def _band_workspace(monkeypatch, p):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "band")
    return solver.QPDO().setup(p["Q"], np.zeros(p["n"]), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)


def _full_Q(p):
    Ql = sp.csr_matrix(p["Q"])
    return (Ql + sp.tril(Ql, -1).T).tocsr()


@pytest.mark.parametrize("b", [3, 4, 63, 64, 126, 127])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_band_factor_and_solves(b, extra, gpu_required, monkeypatch):
    n = 4 * (b + 1) + extra                      # the smallest order the band solver accepts, and the next three (np is padded to 4)
    p = problems.banded_random_qp(300 + b, n, b)
    Qf, A = _full_Q(p), sp.csr_matrix(p["A"])
    rng = np.random.default_rng(b + extra)
    dw = 0.1 + 9.9 * rng.random(p["m"])
    sigma = 1.0
    ws = _band_workspace(monkeypatch, p)
    try:
        assert ws.stats()["linsolve"] == 3
        s0 = ws.stats()
        bs = rhs_set(Qf, A, sigma, dw, n)
        xs = [ws.direct_solve(dw, sigma, bb, refactor=True) for bb in bs]
        g = ws.factor_geometry()
        assert g["b"] == b and g["np"] == (n + 3) // 4 * 4, g
        Kb, Lt = ws.download_factor("Kb"), ws.download_factor("Lt")
        x_again = ws.direct_solve(dw, sigma, bs[0], refactor=True)
        assert np.array_equal(x_again.view(np.uint64), xs[0].view(np.uint64))
        assert np.array_equal(ws.download_factor("Kb").view(np.uint64), Kb.view(np.uint64))
        d = ws.stats()["factor_count"] - s0["factor_count"]
        assert d == 4, d
    finally:
        ws.delete()
    D = Kb[:n, 0]
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    L = np.eye(n)
    for t in range(1, b + 1):
        j = np.arange(n - t)
        L[j + t, j] = Kb[j, t]
        # the row-band copy of the backward solve holds the same bits
        assert np.array_equal(Lt[j + t, t].view(np.uint64), Kb[j, t].view(np.uint64)), t
    K = newton_matrix(Qf, A, sigma, dw)
    elem = ldl_elementwise_ratio(K, L, D)
    eta = max(backward_error(Qf, A, sigma, dw, x, bb, K=K) for x, bb in zip(xs, bs)) / (n * U64)
    _note("band elementwise + solves", eta, elem)
    assert elem <= 1.0, elem
    assert eta <= 4.0, eta


# ---- refusals and no trace ------------------------------------------------------------------------------------------------------------
def test_direct_solve_refuses_a_pcg_workspace(gpu_required, monkeypatch):
    Qf, A, sigma, dw = matrix("well", 100)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    ws = solver.QPDO().setup(Qf, np.zeros(100), A, -np.ones(A.shape[0]), np.ones(A.shape[0]), scaling=0, verbose=0)
    try:
        with pytest.raises(RuntimeError) as e:
            ws.direct_solve(dw, sigma, np.ones(100))
        assert not isinstance(e.value, solver.LostProducer)
    finally:
        ws.delete()


@pytest.mark.parametrize("mode", ["dense", "dense_lowrank", "band"])
def test_hook_calls_leave_no_trace_on_the_next_solve(mode, gpu_required, monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    if mode == "band":
        p = problems.banded_random_qp(77, 2048, 5)
        monkeypatch.setenv("QPDO_LINSOLVE", "band")
    else:
        p = problems.random_qp(21, 300, 450, 0.05, 30)
        monkeypatch.setenv("QPDO_LINSOLVE", "dense")
        monkeypatch.setenv("QPDO_DENSE_LOWRANK", "1" if mode == "dense_lowrank" else "0")

    def make():
        return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p.get("Qstype", -1), c=p.get("c", 0.0), verbose=0)

    def run(s):
        r = s.solve()
        return r, s.trace(), s.stats()

    s1 = make()
    r1, t1, st1 = run(s1)
    s1.delete()
    s2 = make()
    try:
        rng = np.random.default_rng(3)
        n, m = p["n"], p["m"]
        dw = 0.1 + 9.9 * rng.random(m)
        s2.direct_solve(dw, 0.5, rng.standard_normal(n), refactor=True, carry_forward=True)
        dw[:3] *= 2.0
        s2.direct_solve(dw, 0.5, rng.standard_normal(n), refactor=False)
        r2, t2, st2 = run(s2)
        # and after a solve, hook calls again and a second solve: the same as the first solve's repetition on a fresh workspace
        s2.direct_solve(dw, 0.25, rng.standard_normal(n), refactor=True)
        r3 = s2.solve()
    finally:
        s2.delete()
    s4 = make()
    r4a = s4.solve(); r4b = s4.solve()
    s4.delete()
    for a, b in ((r1, r2), (r4b, r3)):
        assert a["info"]["iterations"] == b["info"]["iterations"] and a["info"]["status_val"] == b["info"]["status_val"]
        assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64))
        assert np.array_equal(a["y"].view(np.uint64), b["y"].view(np.uint64))
    assert [tr["tau"] for tr in t1] == [tr["tau"] for tr in t2]
    assert st1["factor_count"] == st2["factor_count"] and st2["chain_fallbacks"] == 0


# ---- large orders: solves only (placed last: k_mid_factor was measured up to n = 12288 only) ---------------------------------------------
def _dense_large(n, seed=3):
    rng = np.random.default_rng(seed)
    Qf = sp.diags(1.0 + rng.random(n)).tocsr()
    m = 64
    A = sp.random(m - 1, n, density=2.0 / n, random_state=rng, format="csr")
    A = sp.vstack([sp.csr_matrix(rng.standard_normal((1, n))), A]).tocsr()
    return Qf, A, 1.0, np.concatenate([[1.0], 0.1 + 9.9 * rng.random(m - 1)])


@pytest.mark.parametrize("n,route", [(12289, "mid"), (12289, "multi_la1"), (20000, "mid"), (40000, "mid")])
def test_dense_large_orders_solves(n, route, gpu_required, monkeypatch):
    env, carry, onelaunch = ROUTES[route]
    Qf, A, sigma, dw = _dense_large(n)
    ws = _workspace(monkeypatch, Qf, A, dict(env, QPDO_DENSE_LOWRANK="0", QPDO_DENSE_MAX_N="40000"))
    try:
        s0 = ws.stats()
        bs = rhs_set(Qf, A, sigma, dw, n)
        xs = [ws.direct_solve(dw, sigma, bs[0], refactor=True, carry_forward=True)]
        xs += [ws.direct_solve(dw, sigma, b, refactor=False) for b in bs[1:]]
        d = _stats_delta(s0, ws.stats())
        assert d == {"factor_count": 1, "onelaunch_factors": 1 if onelaunch else 0, "chain_fallbacks": 0, "lowrank_solves": 0,
                     "lowrank_rejects": 0}, d
    finally:
        ws.delete()
    eta = max(backward_error(Qf, A, sigma, dw, x, b) for x, b in zip(xs, bs)) / (n * U64)
    _note("dense large n (solves)", eta)
    assert eta <= 4.0, eta


def test_band_large_order_solves(gpu_required, monkeypatch):
    n = 200000
    p = problems.banded_random_qp(5, n, 3)
    Qf, A = _full_Q(p), sp.csr_matrix(p["A"])
    dw = 0.1 + 9.9 * np.random.default_rng(1).random(p["m"])
    ws = _band_workspace(monkeypatch, p)
    try:
        bs = rhs_set(Qf, A, 1.0, dw, n)
        xs = [ws.direct_solve(dw, 1.0, bs[0], refactor=True)] + [ws.direct_solve(dw, 1.0, b, refactor=False) for b in bs[1:]]
    finally:
        ws.delete()
    eta = max(backward_error(Qf, A, 1.0, dw, x, b) for x, b in zip(xs, bs)) / (n * U64)
    _note("band large n (solves)", eta)
    assert eta <= 4.0, eta


def test_zz_report():
    """prints the largest measured ratios per group (the figures quoted in the module docstring)"""
    print("\ndirect solver ratios: " + json.dumps(REPORT, sort_keys=True))
    out = os.environ.get("QPDO_DIRECT_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
