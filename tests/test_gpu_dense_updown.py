"""The in-place up/downdate of the kept dense LDL' factor (QPDO_DENSE_UPDOWN; qpdo_amd/csrc/dev/updown.inc) as a linear-algebra object:
through qpdo_amd_direct_solve(refactor = False) with changed weights, qpdo_amd_download_factor and the counters, against K assembled in
extended precision (tests/helpers.py), scaling = 0.  The bounds are the project's bounds for a FRESH factorization
(tests/test_gpu_direct_solvers.py): D > 0 and finite, transposed copies = L' and LinvT = Linv' bit for bit, normwise factor ratio <= 1,
backward error of a solve <= 4 n u, the same bits from the same sequence; tests/test_dense_updown_cpu.py shows on the CPU that the
recurrence itself meets them on the well-conditioned family and that they notice a wrong update.  Linv L_kk = I per diagonal block is
held to INV_C 64 u max(1, max |Linv| |L_kk|): the componentwise residual bound of a triangular inverse formed by substitution (Higham,
Accuracy and Stability of Numerical Algorithms, 14.1: gamma_64 |Linv| |L_kk|), INV_C = 8 for the blocked 16 x 16 scheme's extra products.
On the solver-like family (weights 1e9 entering and leaving) the recurrence itself loses up to four digits, so there only the returned
x is held to 4 n u -- the residual check of every solve with an up/downdated factor, and the refactorization behind it, are what the
caller gets -- and the share of rejects is printed, not capped.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import scipy.sparse as sp

from helpers import U64, backward_error, ldl_normwise_ratio, ldl_numpy, newton_matrix
from qpdo_amd import problems, solver
from test_gpu_direct_solvers import ENV_KEYS, check_factor_storage, matrix, rhs_set

pytestmark = pytest.mark.gpu

CAP = 5
INV_C = 8.0
KEYS = ENV_KEYS + ("QPDO_DENSE_UPDOWN", "QPDO_LAUNCH_AHEAD")
COUNTERS = ("factor_count", "updown_solves", "updown_rows", "updown_rejects", "lowrank_solves", "chain_fallbacks")


def _workspace(monkeypatch, Qf, A, updown=str(CAP)):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QPDO_LINSOLVE", "dense")
    monkeypatch.setenv("QPDO_DENSE_LOWRANK", "0")
    if updown is not None:
        monkeypatch.setenv("QPDO_DENSE_UPDOWN", updown)
    n, m = Qf.shape[0], A.shape[0]
    return solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)


def _delta(a, b):
    return {k: b[k] - a[k] for k in COUNTERS}


def _new_weights(rng, dw, k, zero_one):
    rows = rng.choice(len(dw), k, replace=False)
    dw1 = dw.copy()
    dw1[rows] = dw[rows] * np.where(rng.random(k) < 0.5, 0.2 + 0.6 * rng.random(k), 1.5 + 3.0 * rng.random(k))
    dw1[rows] = np.where(dw[rows] == 0.0, 1.0 + rng.random(k), dw1[rows])          # (a weight an earlier call set to 0 comes back: every chosen row changes)
    if zero_one:
        dw1[rows[0]] = 0.0
    return dw1


def _diag_inverse_residual(ws, Kd, n):
    g = ws.factor_geometry()
    nb = g["nb"]
    Li = ws.download_factor("Linv").reshape(nb, 64, 64).transpose(0, 2, 1)          # [k][r][c]
    worst = 0.0
    for k in range(nb):
        Lkk = np.tril(Kd[64 * k:64 * k + 64, 64 * k:64 * k + 64], -1) + np.eye(64)
        res = np.abs(Li[k] @ Lkk - np.eye(64)).max()
        scale = max(1.0, float((np.abs(Li[k]) @ np.abs(Lkk)).max()))
        worst = max(worst, res / (64 * U64 * scale))
    return worst


def run_well_sequence(monkeypatch, n):
    """one refactored solve, then three calls that change 1, 3 and CAP weights (refactor = False); returns every bit that came back"""
    Qf, A, sigma, dw = matrix("well", n)
    A = sp.csr_matrix(A)
    m = A.shape[0]
    rng = np.random.default_rng(100 + n)
    bits = []
    ws = _workspace(monkeypatch, Qf, A)
    try:
        ws.direct_solve(dw, sigma, rhs_set(Qf, A, sigma, dw, n)[0], refactor=True)
        for call, k in enumerate((1, 3, CAP)):
            k = min(k, m)
            dw = _new_weights(rng, dw, k, zero_one=(call == 1))
            s0 = ws.stats()
            bs = rhs_set(Qf, A, sigma, dw, n)
            xs = [ws.direct_solve(dw, sigma, b, refactor=False) for b in bs]
            d = _delta(s0, ws.stats())
            print("n = %d, %d changed rows: %s" % (n, k, d))
            # the first solve applies the k rows, the other two find nothing changed; all three are checked solves, none factors
            assert d == {"factor_count": 0, "updown_solves": 3, "updown_rows": k, "updown_rejects": 0, "lowrank_solves": 0, "chain_fallbacks": 0}, d
            L, D, Kd = check_factor_storage(ws, n)
            inv = _diag_inverse_residual(ws, Kd, n)
            K = newton_matrix(Qf, A, sigma, dw)
            ratio = ldl_normwise_ratio(K, L, D)
            eta = max(backward_error(Qf, A, sigma, dw, x, b, K=K) for x, b in zip(xs, bs)) / (n * U64)
            print("   normwise factor ratio %.3g, eta / (n u) %.3g, |Linv L_kk - I| / (64 u scale) %.3g" % (ratio, eta, inv))
            assert inv <= INV_C, inv
            assert ratio <= 1.0, ratio
            assert eta <= 4.0, eta
            bits += [x.view(np.uint64).copy() for x in xs]
            bits += [np.tril(Kd, -1).view(np.uint64).copy(), ws.download_factor("Dg").view(np.uint64), ws.download_factor("Linv").view(np.uint64)]
    finally:
        ws.delete()
    return bits


@pytest.mark.parametrize("n", [1, 64, 65, 207, 369, 1008, 2088])
def test_updown_keeps_the_factor_inside_the_bounds_of_a_fresh_one(n, gpu_required, monkeypatch):
    first = run_well_sequence(monkeypatch, n)
    again = run_well_sequence(monkeypatch, n)
    assert len(first) == len(again) and all(np.array_equal(a, b) for a, b in zip(first, again))


def test_more_changed_rows_than_the_cap_refactor(gpu_required, monkeypatch):
    n = 369
    Qf, A, sigma, dw = matrix("well", n)
    ws = _workspace(monkeypatch, Qf, A)
    try:
        b = rhs_set(Qf, A, sigma, dw, n)[0]
        ws.direct_solve(dw, sigma, b, refactor=True)
        dw1 = _new_weights(np.random.default_rng(1), dw, CAP + 1, False)
        s0 = ws.stats()
        x = ws.direct_solve(dw1, sigma, b, refactor=False)
        d = _delta(s0, ws.stats())
        assert d == {"factor_count": 1, "updown_solves": 0, "updown_rows": 0, "updown_rejects": 0, "lowrank_solves": 0, "chain_fallbacks": 0}, d
    finally:
        ws.delete()
    assert backward_error(Qf, A, sigma, dw1, x, b) / (n * U64) <= 4.0


@pytest.mark.parametrize("setting,changed,expect_rows,expect_factors", [
    ("1", 1, 1, 0), ("1", 2, 0, 1),                    # "1": the default cap, one row
    ("1000", 64, 64, 0), ("1000", 65, 0, 1),           # clamped at 64 rows
    ("0", 2, 0, 0), (None, 2, 0, 0)])                  # off: the kept factor is reused as it is (the caller's business), the counters stay 0
def test_the_switch_values(setting, changed, expect_rows, expect_factors, gpu_required, monkeypatch):
    n = 369
    Qf, A, sigma, dw = matrix("well", n)
    ws = _workspace(monkeypatch, Qf, A, updown=setting)
    try:
        b = rhs_set(Qf, A, sigma, dw, n)[0]
        ws.direct_solve(dw, sigma, b, refactor=True)
        dw1 = _new_weights(np.random.default_rng(4), dw, changed, False)
        s0 = ws.stats()
        x = ws.direct_solve(dw1, sigma, b, refactor=False)
        d = _delta(s0, ws.stats())
        print(setting, changed, d)
        on = expect_rows > 0
        assert d == {"factor_count": expect_factors, "updown_solves": 1 if on else 0, "updown_rows": expect_rows, "updown_rejects": 0,
                     "lowrank_solves": 0, "chain_fallbacks": 0}, d
    finally:
        ws.delete()
    if setting not in ("0", None):
        assert backward_error(Qf, A, sigma, dw1, x, b) / (n * U64) <= 4.0


def test_another_sigma_and_the_refactor_flag_refactor(gpu_required, monkeypatch):
    n = 369
    Qf, A, sigma, dw = matrix("well", n)
    ws = _workspace(monkeypatch, Qf, A)
    try:
        b = rhs_set(Qf, A, sigma, dw, n)[0]
        ws.direct_solve(dw, sigma, b, refactor=True)
        dw1 = _new_weights(np.random.default_rng(2), dw, 2, False)
        s0 = ws.stats()
        x1 = ws.direct_solve(dw1, 0.5 * sigma, b, refactor=False)
        s1 = ws.stats()
        dw2 = _new_weights(np.random.default_rng(3), dw1, 2, False)
        x2 = ws.direct_solve(dw2, 0.5 * sigma, b, refactor=True)
        s2 = ws.stats()
        for d in (_delta(s0, s1), _delta(s1, s2)):
            assert d == {"factor_count": 1, "updown_solves": 0, "updown_rows": 0, "updown_rejects": 0, "lowrank_solves": 0, "chain_fallbacks": 0}, d
    finally:
        ws.delete()
    assert backward_error(Qf, A, 0.5 * sigma, dw1, x1, b) / (n * U64) <= 4.0
    assert backward_error(Qf, A, 0.5 * sigma, dw2, x2, b) / (n * U64) <= 4.0


@pytest.mark.parametrize("n", [207, 369, 1008])
def test_heavy_rows_entering_and_leaving_return_checked_solutions(n, gpu_required, monkeypatch):
    Qf, A, sigma, dw = matrix("solver", n)
    m = A.shape[0]
    rng = np.random.default_rng(7 + n)
    calls = 12
    ws = _workspace(monkeypatch, Qf, A)
    worst = 0.0
    try:
        ws.direct_solve(dw, sigma, rhs_set(Qf, A, sigma, dw, n)[0], refactor=True)
        s0 = ws.stats()
        for call in range(calls):
            k = 1 + call % 3
            on, off = np.flatnonzero(dw == 1e9), np.flatnonzero(dw == 0.0)
            leave = rng.choice(on, k // 2 + (call % 2), replace=False)
            enter = rng.choice(off, k - len(leave), replace=False) if k > len(leave) else np.zeros(0, int)
            dw = dw.copy()
            dw[leave] = 0.0
            dw[enter] = 1e9
            b = rhs_set(Qf, A, sigma, dw, n, seed=call)[call % 3]
            x = ws.direct_solve(dw, sigma, b, refactor=False)
            assert np.all(np.isfinite(x))
            eta = backward_error(Qf, A, sigma, dw, x, b) / (n * U64)
            worst = max(worst, eta)
            assert eta <= 4.0, (call, eta)
        d = _delta(s0, ws.stats())
    finally:
        ws.delete()
    print("solver-like n = %d: %d calls, %s, reject share %.2f, worst eta / (n u) %.3g" % (n, calls, d, d["updown_rejects"] / calls, worst))
    assert d["updown_solves"] + d["updown_rejects"] == calls, d
    assert d["factor_count"] == d["updown_rejects"] and d["chain_fallbacks"] == 0, d


def test_a_downdate_that_makes_K_indefinite_is_rejected_and_refactored(gpu_required, monkeypatch):
    n = 207
    Qf, A, sigma, dw = matrix("well", n)
    A = sp.csr_matrix(A)
    K = newton_matrix(Qf, A, sigma, dw).astype(np.float64)
    r = int(np.argmax(np.asarray(A.multiply(A).sum(axis=1)).ravel()))
    a = np.asarray(A[r].todense()).ravel()
    dw1 = dw.copy()
    dw1[r] = -2.0 / float(a @ np.linalg.solve(K - dw[r] * np.outer(a, a), a))      # below what was factored by more than the row holds
    K1 = newton_matrix(Qf, A, sigma, dw1)
    assert np.linalg.eigvalsh(K1.astype(np.float64))[0] < 0
    # what a fresh LDL' without pivoting of this indefinite K can promise: 4 n u times its growth |L| |D| |L'| / |K| (Higham, 11.x)
    Lr, Dr = ldl_numpy(K1.astype(np.float64))
    growth = max(1.0, float((np.abs(Lr) * np.abs(Dr)[None, :] @ np.abs(Lr).T).sum(axis=1).max() / np.abs(K1.astype(np.float64)).sum(axis=1).max()))
    ws = _workspace(monkeypatch, Qf, A)
    try:
        bs = rhs_set(Qf, A, sigma, dw1, n)
        ws.direct_solve(dw, sigma, bs[0], refactor=True)
        Kd0, Dg0 = ws.download_factor("Kd"), ws.download_factor("Dg")
        s0 = ws.stats()
        try:
            x = ws.direct_solve(dw1, sigma, bs[0], refactor=False)
        except solver.LostProducer:
            raise
        except RuntimeError as e:              # a clean error is the other allowed outcome
            print("indefinite downdate: refused with", e)
            return
        d = _delta(s0, ws.stats())
        print("indefinite downdate:", d, "growth of the refactored LDL' %.3g" % growth)
        assert d["updown_rejects"] == 1 and d["factor_count"] == 1 and d["updown_solves"] == 0, d
    finally:
        ws.delete()
    assert np.all(np.isfinite(x))
    eta = backward_error(Qf, A, sigma, dw1, x, bs[0], K=K1) / (n * U64)
    print("   eta / (n u) %.3g (bound 4 x growth)" % eta)
    assert eta <= 4.0 * growth, eta
    assert np.all(np.isfinite(Kd0[:n, :n])) and np.all(Dg0[:n] > 0)


WHOLE = {"n200": (41, 200, 300, 0.1, 20), "n500": (42, 500, 1000, 0.05, 40), "n1000": (43, 1000, 1500, 0.02, 60)}


@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_solves_agree_with_the_route_off(name, gpu_required, monkeypatch):
    p = problems.random_qp(*WHOLE[name])

    def run(updown):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("QPDO_LINSOLVE", "dense")
        if updown:
            monkeypatch.setenv("QPDO_DENSE_UPDOWN", updown)
        s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p.get("Qstype", -1), verbose=0)
        try:
            r = s.solve()
            return r, s.stats()
        finally:
            s.delete()

    r0, st0 = run(None)
    r1, st1 = run(str(CAP))
    eps = float(solver.default_settings().eps_abs)
    print(name, "off:", r0["info"]["status_val"], r0["info"]["iterations"], {k: st0[k] for k in COUNTERS + ("ahead_steps",)})
    print(name, "on: ", r1["info"]["status_val"], r1["info"]["iterations"], {k: st1[k] for k in COUNTERS + ("ahead_steps",)})
    assert st0["updown_solves"] == st0["updown_rows"] == st0["updown_rejects"] == 0
    assert st0["ahead_steps"] > 0 and st1["ahead_steps"] == 0           # the launch-ahead route: as before when off, not taken when on
    assert r1["info"]["status_val"] == r0["info"]["status_val"]
    for key in ("x", "y"):
        dv = float(np.abs(r1[key] - r0[key]).max())
        print("   |d%s|inf = %.3g" % (key, dv))
        assert dv <= 10 * eps * max(1.0, float(np.abs(r0[key]).max())), (key, dv)
    assert st1["updown_rows"] > 0 and st1["factor_count"] < st0["factor_count"], (st0, st1)
