"""Chain QPs with a few dense coupling rows (QPDO_BAND_COUPLING; dev/band.inc, dev/host_band.inc): the Newton matrix is band plus low rank,
K = B + U W U', and is solved by the band LDL' of B, one multi-right-hand-side band solve for Z = B^-1 U and the k x k system S = W^-1 +
U'Z, inside the residual-checked refinement of the dense low-rank path.  (a) single linear solves at the smallest shapes against K in
extended precision (tests/helpers.py), with the factor of B, every column of Z, the counters and the reuse rules; (b) the selection rules;
(c) whole solves against the oracle; (d) the test hook leaves no trace.  tests/test_band_coupled_cpu.py shows on the CPU that a float64
emulation of this solve is accepted by the device's residual rule on every Newton pass of the oracle's runs on the instances of (c): a
reject on the device is a finding, not a number to relax."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_coupled_ref as ref
from helpers import ITERATE_RTOL, U64, assert_same_trace, backward_error, close_vec, ldl_elementwise_ratio, newton_matrix
from oracle import binding as ob
from qpdo_amd import problems, solver
from test_gpu_direct_solvers import ENV_KEYS, _full_Q, rhs_set

pytestmark = pytest.mark.gpu

SEED = ref.ORACLE_SEED


def _env(monkeypatch, linsolve="band", coupling="64"):
    for k in ENV_KEYS + ("QPDO_BAND_COUPLING",):
        monkeypatch.delenv(k, raising=False)
    if linsolve:
        monkeypatch.setenv("QPDO_LINSOLVE", linsolve)
    if coupling:
        monkeypatch.setenv("QPDO_BAND_COUPLING", coupling)


def _linear_workspace(p):
    return solver.QPDO().setup(p["Q"], np.zeros(p["n"]), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)


def _counters(ws):
    st = ws.stats()
    return {k: st[k] for k in ("factor_count", "coupled_solves", "coupled_sweeps", "coupled_rejects", "band_fallbacks")}


# ---- (a) linear solves ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 64])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
@pytest.mark.parametrize("b", [3, 64, 127])
def test_coupled_factor_and_solves(b, extra, r, gpu_required, monkeypatch):
    n = max(129, 4 * (b + 1)) + extra           # a span above 127 needs n >= 129; the band solver n >= 4 (b + 1); np is padded to 4
    base = problems.banded_random_qp(300 + b, n, b)
    p = ref.append_rows(base, ref.coupling_rows(300 + b, n, r), -np.ones(r), np.ones(r))
    m0, m = base["m"], p["m"]
    Qf, A = _full_Q(p), sp.csr_matrix(p["A"])
    rows, b_core = ref.classify(Qf, A)
    assert list(rows) == list(range(m0, m)) and b_core == b
    rng = np.random.default_rng(1000 * b + 10 * extra + r)
    dw = 0.1 + 9.9 * rng.random(m)
    if r > 1:
        dw[rows[rng.choice(r, max(1, r // 4), replace=False)]] = 0.0          # at least one coupling row without weight
    dcore = dw.copy()
    dcore[rows] = 0.0
    act = rows[dw[rows] != 0.0]
    sigma = 1.0
    bs = rhs_set(Qf, A, sigma, dw, n)
    _env(monkeypatch)
    ws = _linear_workspace(p)
    try:
        st = ws.stats()
        assert st["linsolve"] == 3 and st["coupled_rows"] == r
        c0 = _counters(ws)
        xs = [ws.direct_solve(dw, sigma, bb, refactor=True) for bb in bs]
        geo = ws.download_factor("coupled_geometry")
        assert geo == dict(r=r, k=len(act), b_core=b, np=(n + 3) // 4 * 4), geo
        assert np.array_equal(ws.download_factor("coupled_rows"), rows)
        g = ws.factor_geometry()
        assert g["b"] == b and g["np"] == geo["np"], g
        Kb, Z = ws.download_factor("Kb"), ws.download_factor("Z")
        assert Z.shape == (geo["np"], len(act))
        x_again = ws.direct_solve(dw, sigma, bs[0], refactor=True)
        assert np.array_equal(x_again.view(np.uint64), xs[0].view(np.uint64))
        assert np.array_equal(ws.download_factor("Kb").view(np.uint64), Kb.view(np.uint64))
        assert np.array_equal(ws.download_factor("Z").view(np.uint64), Z.view(np.uint64))
        c1 = _counters(ws)
        assert c1["factor_count"] - c0["factor_count"] == 4 and c1["coupled_solves"] - c0["coupled_solves"] == 4, (c0, c1)
        assert c1["coupled_rejects"] == 0 and c1["band_fallbacks"] == 0, c1
        # only coupling weights move -- one changes, one without weight gets one (r > 1), one loses its own (k > 1): S alone is rebuilt
        dw2 = dw.copy()
        dw2[act[0]] *= 3.0
        if len(act) < r:
            dw2[[i for i in rows if dw[i] == 0.0][0]] = 2.5
        if len(act) > 1:
            dw2[act[-1]] = 0.0
        x2 = ws.direct_solve(dw2, sigma, bs[0], refactor=False)
        x2_again = ws.direct_solve(dw2, sigma, bs[0], refactor=False)
        c2 = _counters(ws)
        assert c2["factor_count"] == c1["factor_count"] and c2["coupled_solves"] - c1["coupled_solves"] == 2 and c2["coupled_rejects"] == 0, (c1, c2)
        assert np.array_equal(x2.view(np.uint64), x2_again.view(np.uint64))
        assert np.array_equal(ws.download_factor("Kb").view(np.uint64), Kb.view(np.uint64))
        # a core weight moves: B is factored again without being asked to
        dw3 = dw2.copy()
        dw3[0] *= 2.0
        x3 = ws.direct_solve(dw3, sigma, bs[0], refactor=False)
        c3 = _counters(ws)
        assert c3["factor_count"] == c2["factor_count"] + 1 and c3["coupled_rejects"] == 0, (c2, c3)
        # no coupling row weighted: the plain band solve, no residual check
        x0 = ws.direct_solve(dcore, sigma, bs[0], refactor=True)
        c4 = _counters(ws)
        assert c4["coupled_solves"] == c3["coupled_solves"] and c4["coupled_sweeps"] == c3["coupled_sweeps"], (c3, c4)
        assert ws.download_factor("coupled_geometry")["k"] == 0
    finally:
        ws.delete()
    # ... bit for bit the uncoupled band workspace of the core rows alone
    _env(monkeypatch, coupling=None)
    wu = _linear_workspace(base)
    try:
        assert wu.stats()["linsolve"] == 3 and wu.stats()["coupled_rows"] == 0
        xu = wu.direct_solve(dcore[:m0], sigma, bs[0], refactor=True)
    finally:
        wu.delete()
    assert np.array_equal(x0.view(np.uint64), xu.view(np.uint64))
    # Kb is the factor of B
    D = Kb[:n, 0]
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    L = np.eye(n)
    for t in range(1, b + 1):
        j = np.arange(n - t)
        L[j + t, j] = Kb[j, t]
    B = newton_matrix(Qf, A, sigma, dcore)
    elem = ldl_elementwise_ratio(B, L, D)
    assert elem <= 1.0, elem
    # every column of Z solves B z = u
    for j, row in enumerate(act):
        u = A[row].toarray().ravel()
        eta = backward_error(Qf, A, sigma, dcore, Z[:n, j], u, K=B) / (n * U64)
        assert eta <= 4.0, (j, eta)
    # every solve against the full K
    K = newton_matrix(Qf, A, sigma, dw)
    eta = max(backward_error(Qf, A, sigma, dw, x, bb, K=K) for x, bb in zip(xs, bs)) / (n * U64)
    eta2 = backward_error(Qf, A, sigma, dw2, x2, bs[0]) / (n * U64)
    eta3 = backward_error(Qf, A, sigma, dw3, x3, bs[0]) / (n * U64)
    print("b = %d, n = %d, r = %d, k = %d: eta / (n u) %.3g, %.3g, %.3g, elementwise %.3g" % (b, n, r, len(act), eta, eta2, eta3, elem))
    assert eta <= 4.0 and eta2 <= 4.0 and eta3 <= 4.0, (eta, eta2, eta3)


# ---- (b) selection ----------------------------------------------------------------------------------------------------------------------
def _setup_error(p):
    with pytest.raises(RuntimeError) as e:
        solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0).delete()
    return str(e.value)


def test_without_the_variable_nothing_changes(gpu_required, monkeypatch):
    for key in [(600, 5, 1), (2100, 3, 2)]:
        p = ref.coupled_banded_qp(SEED, *key)
        _env(monkeypatch, linsolve=None, coupling=None)
        st = solver.solve_problem(p, verbose=0, max_iter=5)["stats"]
        assert st["linsolve"] == 1 and st["coupled_rows"] == 0 and st["coupled_solves"] == 0, st
        _env(monkeypatch, coupling=None)
        assert "not banded" in _setup_error(p)
        _env(monkeypatch, coupling="0")
        assert "not banded" in _setup_error(p)


def test_more_coupling_rows_than_accepted_fail_at_setup_when_asked_for(gpu_required, monkeypatch):
    base = problems.banded_random_qp(SEED, 700, 17)
    p = ref.append_rows(base, ref.coupling_rows(SEED, 700, 65), -np.ones(65), np.ones(65))
    _env(monkeypatch, coupling="64")
    msg = _setup_error(p)
    assert "65" in msg and "64" in msg, msg
    p3 = ref.coupled_banded_qp(SEED, 600, 5, 3)
    _env(monkeypatch, coupling="2")
    msg = _setup_error(p3)
    assert "3 rows" in msg and "accepts 2" in msg, msg
    # not asked for: the usual selection, as if the variable were unset
    _env(monkeypatch, linsolve=None, coupling="2")
    st = solver.solve_problem(p3, verbose=0, max_iter=5)["stats"]
    assert st["linsolve"] == 1 and st["coupled_rows"] == 0, st


# ---- (c) whole solves against the oracle ------------------------------------------------------------------------------------------------
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


def _assert_coupled(st, r):
    assert st["linsolve"] == 3 and st["coupled_rows"] == r, st
    assert st["coupled_solves"] > 0 and st["coupled_rejects"] == 0 and st["band_fallbacks"] == 0, st
    assert st["coupled_sweeps"] <= 2 * st["coupled_solves"], st          # (at most one refinement sweep per solve: the CPU emulation's finding)


@pytest.mark.parametrize("key", list(ref.ORACLE_RESULTS))
def test_whole_solves_match_the_oracle(key, gpu_required, monkeypatch):
    n, bw, r = key
    p = ref.coupled_banded_qp(SEED, *key)
    # (2100, 3, 2): the band solver is selected automatically from n = 2048 up; the smaller ones on request
    _env(monkeypatch, linsolve=None if n >= 2048 else "band")
    res = solver.solve_problem(p, verbose=0)
    ro, tro = oracle_run(p)
    assert (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"]) == ref.ORACLE_RESULTS[key]
    st = res["stats"]
    print("%s: %s" % (key, {k: st[k] for k in ("newton_passes", "factor_count", "coupled_solves", "coupled_sweeps", "coupled_rejects", "band_fallbacks")}))
    _assert_coupled(st, r)
    assert st["factor_count"] <= st["newton_passes"] and st["lin_iters"] == 0, st
    check(res, ro, tro, p)


def test_update_sequence_and_new_matrix_values(gpu_required, monkeypatch):
    p = ref.coupled_banded_qp(SEED, 600, 5, 3)
    _env(monkeypatch)
    o = ob.OracleSolver(p, ob.default_settings())
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    try:
        ro, rg = o.solve(), s.solve()
        rg["trace"] = s.trace(); check(rg, ro, o.trace(), p)
        _assert_coupled(s.stats(), 3)
        # update_q, update_bounds, warm_start, solve
        q2 = p["q"] * 1.1 + 0.05
        l2, u2 = p["l"].copy(), p["u"].copy()
        l2[:p["n"]] -= 0.05; u2[:p["n"]] += 0.02
        cl, cu = l2[-3:], u2[-3:]                                   # the coupling rows' finite bounds (views)
        cl[np.abs(cl) < 1e19] *= 1.2; cu[np.abs(cu) < 1e19] *= 1.2
        for w in (o, s):
            w.update_q(q2); w.update_bounds(l2, u2); w.warm_start(ro["x"], ro["y"])
        p2 = dict(p, q=q2, l=l2, u=u2)
        ro2, rg2 = o.solve(), s.solve()
        rg2["trace"] = s.trace(); check(rg2, ro2, o.trace(), p2)
        _assert_coupled(s.stats(), 3)
        # new values of Q and A in the same pattern: the coupling rows are the pattern's and stay
        rng = np.random.default_rng(5)
        A3 = p["A"].copy(); A3.data = A3.data * (1.0 + 0.2 * rng.random(A3.nnz))
        Q3 = p["Q"].copy(); Q3.setdiag(Q3.diagonal() * 1.3)
        s.update_matrices(Q=Q3, A=A3)
        p3 = dict(p2, Q=Q3, A=A3)
        o3 = ob.OracleSolver(p3, ob.default_settings())
        ro3 = o3.solve(); tr3 = o3.trace(); o3.close()
        rg3 = s.solve()
        rg3["trace"] = s.trace(); check(rg3, ro3, tr3, p3)
        _assert_coupled(s.stats(), 3)
        assert np.array_equal(s.download_factor("coupled_rows"), np.arange(p["m"] - 3, p["m"]))
    finally:
        s.delete(); o.close()


# ---- (d) no trace -----------------------------------------------------------------------------------------------------------------------
def test_hook_calls_leave_no_trace_on_the_next_solve(gpu_required, monkeypatch):
    p = ref.coupled_banded_qp(SEED, 600, 5, 3)
    _env(monkeypatch)

    def make():
        return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)

    s1 = make()
    r1 = s1.solve(); t1 = s1.trace(); st1 = s1.stats()
    s1.delete()
    s2 = make()
    try:
        rng = np.random.default_rng(3)
        n, m = p["n"], p["m"]
        dw = 0.1 + 9.9 * rng.random(m)
        s2.direct_solve(dw, 0.5, rng.standard_normal(n), refactor=True)
        dw[-2:] *= 2.0
        s2.direct_solve(dw, 0.5, rng.standard_normal(n), refactor=False)
        r2 = s2.solve(); t2 = s2.trace(); st2 = s2.stats()
        s2.direct_solve(dw, 0.25, rng.standard_normal(n), refactor=True)
        r3 = s2.solve()
    finally:
        s2.delete()
    s4 = make()
    s4.solve(); r4b = s4.solve()
    s4.delete()
    for a, b in ((r1, r2), (r4b, r3)):
        assert a["info"]["iterations"] == b["info"]["iterations"] and a["info"]["status_val"] == b["info"]["status_val"]
        assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64))
        assert np.array_equal(a["y"].view(np.uint64), b["y"].view(np.uint64))
    assert [tr["tau"] for tr in t1] == [tr["tau"] for tr in t2]
    for k in ("factor_count", "coupled_solves", "coupled_sweeps", "coupled_rejects", "band_fallbacks"):
        assert st1[k] == st2[k], (k, st1[k], st2[k])
