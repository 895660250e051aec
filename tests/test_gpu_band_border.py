"""Chain QPs with a few coupling VARIABLES (QPDO_BAND_BORDER; dev/band.inc, dev/host_band.inc, qpdo_amd/csrc/band_border.c): the Newton
matrix is a bordered band, K = [B C; C' D], and is solved by block elimination -- the band LDL' of the core B, one multi-right-hand-side
band solve for Z = B^-1 C, the c x c system S = D - C'Z in LDS.  (a) single linear solves at the smallest shapes against K in extended
precision (tests/helpers.py), with the geometry, the factor of B bit for bit that of the plain band workspace on the core-only problem,
every column of Z and the counters; (b) the selection rules; (c) whole solves against the oracle, an update sequence; (d) the test hook
leaves no trace; (e) the sensitivity calls.  tests/test_band_border_cpu.py checks the instances of (c) on the CPU -- status 1, a border
that is off its bound on four of the five -- and shows that a float64 emulation of this elimination stays below 4 n u on every Newton
pass of the oracle's runs.  The bound 4 n u is the project's for its direct solvers (tests/test_gpu_direct_solvers.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_border_ref as ref
import fleet_adjoint_ref as aref
import fleet_sensitivity_ref as sref
from helpers import U64, backward_error, newton_matrix
from oracle import binding as ob
from qpdo_amd import problems, solver
from test_gpu_band_coupled import _setup_error, check, oracle_run
from test_gpu_direct_solvers import ENV_KEYS, _full_Q, rhs_set
from test_gpu_workspace_adjoint import W, check_rhs, raw_adjoint  # noqa: F401
from test_gpu_workspace_tangent import EPS, pick, raw_tangent
from test_gpu_workspace_tangent import check_rhs as check_tangent_rhs

pytestmark = pytest.mark.gpu

SEED = ref.ORACLE_SEED
COUNTERS = ("factor_count", "band_fallbacks", "lin_iters", "coupled_rows", "coupled_solves")


def _env(monkeypatch, linsolve="band", border="64", **more):
    for k in ENV_KEYS + ("QPDO_BAND_COUPLING", "QPDO_BAND_BORDER", "QPDO_BAND_ORDER", "QPDO_AMD_RHS_GROUP"):
        monkeypatch.delenv(k, raising=False)
    if linsolve:
        monkeypatch.setenv("QPDO_LINSOLVE", linsolve)
    if border is not None:
        monkeypatch.setenv("QPDO_BAND_BORDER", border)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def _linear_workspace(p):
    return solver.QPDO().setup(p["Q"], np.zeros(p["n"]), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)


def _workspace(p, **kw):
    return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- (a) linear solves ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 64])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
@pytest.mark.parametrize("b", [3, 64, 127])
def test_border_factor_and_solves(b, extra, c, gpu_required, monkeypatch):
    nc = max(132, 4 * (b + 1)) + extra          # a row 128 columns ahead of the border needs n_core >= 128; the band solver n_core >= 4 (b + 1); np is padded to 4
    p = problems.bordered_banded_qp(300 + b, nc, b, c)
    n, m = p["n"], p["m"]
    assert ref.detect(p["Q"], p["A"]) == (nc, c, b)
    core = ref.core_problem(p, nc)
    Qf, A = _full_Q(p), sp.csr_matrix(p["A"])
    Qc, Ac = _full_Q(core), sp.csr_matrix(core["A"])
    rng = np.random.default_rng(1000 * b + 10 * extra + c)
    dw = 0.1 + 9.9 * rng.random(m)
    dw[rng.choice(m, m // 5, replace=False)] = 0.0
    if c > 1:                                   # every row that touches the last border variable without weight: its column of C comes from Q alone
        dw[sp.csc_matrix(p["A"])[:, n - 1].nonzero()[0]] = 0.0
        assert abs(sp.csr_matrix(Qf)[n - 1, :nc]).sum() > 0
    sigma = 1.0
    bs = rhs_set(Qf, A, sigma, dw, n)
    _env(monkeypatch)
    ws = _linear_workspace(p)
    try:
        st, info = ws.stats(), ws.band_border()
        assert st["linsolve"] == 3 and st["coupled_rows"] == 0, st
        assert (info["max_border"], info["border"], info["n_core"], info["b_core"], info["over"], info["reason"]) == (64, c, nc, b, 0, 0), info
        f0, s0 = st["factor_count"], info["border_solves"]
        xs = [ws.direct_solve(dw, sigma, bb, refactor=True) for bb in bs]
        geo = ws.download_factor("border_geometry")
        assert geo == dict(n_core=nc, c=c, b_core=b, np=(nc + 3) // 4 * 4), geo
        g = ws.factor_geometry()
        assert g["b"] == b and g["np"] == geo["np"], g
        Kb, Cd, Z = ws.download_factor("Kb"), ws.download_factor("border_C"), ws.download_factor("border_Z")
        assert Cd.shape == Z.shape == (geo["np"], c)
        x_again = ws.direct_solve(dw, sigma, bs[0], refactor=True)
        assert np.array_equal(_bits(x_again), _bits(xs[0]))
        for name, arr in (("Kb", Kb), ("border_C", Cd), ("border_Z", Z)):
            assert np.array_equal(_bits(ws.download_factor(name)), _bits(arr)), name
        st1, info1 = ws.stats(), ws.band_border()
        assert st1["factor_count"] - f0 == len(bs) + 1 and info1["border_solves"] - s0 == len(bs) + 1, (st1, info1)
        assert st1["band_fallbacks"] == 0 and ws.rhs_group() == 1, st1
    finally:
        ws.delete()
    # Kb is, bit for bit, the factor of the plain band workspace on the core-only problem: the same rows without the border columns
    _env(monkeypatch, border=None)
    wu = _linear_workspace(core)
    try:
        assert wu.stats()["linsolve"] == 3
        wu.direct_solve(dw, sigma, bs[0][:nc], refactor=True)
        assert wu.factor_geometry() == g
        Ku = wu.download_factor("Kb")
    finally:
        wu.delete()
    assert np.array_equal(_bits(Kb), _bits(Ku))
    D = Kb[:nc, 0]
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    # C is the border block of K; every column of Z solves B z = C_j
    K = newton_matrix(Qf, A, sigma, dw)
    B = newton_matrix(Qc, Ac, sigma, dw)
    assert np.array_equal(K[:nc, :nc], B)
    Cref = K[:nc, nc:].astype(np.float64)
    assert np.abs(Cd[:nc] - Cref).max() <= 4.0 * n * U64 * float(np.abs(K).max()) and not Cd[nc:].any()
    eta_z = max(backward_error(Qc, Ac, sigma, dw, Z[:nc, j], Cref[:, j], K=B) for j in range(c)) / (nc * U64)
    assert eta_z <= 4.0, eta_z
    # every solve against the full K
    eta = max(backward_error(Qf, A, sigma, dw, x, bb, K=K) for x, bb in zip(xs, bs)) / (n * U64)
    print("b = %d, n_core = %d, c = %d: eta / (n u) %.3g, columns of Z %.3g" % (b, nc, c, eta, eta_z))
    assert eta <= 4.0, eta


# ---- (b) selection ----------------------------------------------------------------------------------------------------------------------
def _short_solve(p):
    s = _workspace(p, max_iter=5)
    try:
        r = s.solve()
        return r, s.stats(), s.band_border(), s.band_order_info()
    finally:
        s.delete()


def test_without_the_variable_nothing_changes(gpu_required, monkeypatch):
    for key in [(600, 5, 1), (2100, 3, 2)]:
        p = ref.bordered_qp(key)
        runs = []
        for border in (None, "0"):
            _env(monkeypatch, linsolve=None, border=border)
            r, st, info, _ = _short_solve(p)
            assert st["linsolve"] == 1 and info["border"] == 0 and info["max_border"] == 0 and info["border_solves"] == 0, (st, info)
            runs.append((r, st))
            _env(monkeypatch, border=border)
            msg = _setup_error(p)
            assert "not banded" in msg and "BORDER" not in msg, msg
        (ra, sa), (rb, sb) = runs
        assert np.array_equal(_bits(ra["x"]), _bits(rb["x"])) and np.array_equal(_bits(ra["y"]), _bits(rb["y"]))
        assert {k: sa[k] for k in COUNTERS} == {k: sb[k] for k in COUNTERS}


def test_a_plainly_banded_problem_is_the_plain_band_workspace(gpu_required, monkeypatch):
    p = problems.banded_random_qp(SEED, 600, 5)
    _env(monkeypatch, border=None)
    ra, sa, _, _ = _short_solve(p)
    _env(monkeypatch)
    rb, sb, info, _ = _short_solve(p)
    assert sa["linsolve"] == sb["linsolve"] == 3
    assert (info["border"], info["n_core"], info["b_core"], info["over"], info["reason"], info["border_solves"]) == (0, 600, 5, 0, 0, 0), info
    assert np.array_equal(_bits(ra["x"]), _bits(rb["x"])) and np.array_equal(_bits(ra["y"]), _bits(rb["y"]))
    assert {k: sa[k] for k in COUNTERS} == {k: sb[k] for k in COUNTERS}


def test_more_border_variables_than_accepted(gpu_required, monkeypatch):
    p65 = problems.bordered_banded_qp(SEED, 700, 17, 65)
    _env(monkeypatch)
    msg = _setup_error(p65)
    assert "not banded" in msg and "65" in msg and "64" in msg, msg
    p3 = ref.bordered_qp((600, 5, 3))
    _env(monkeypatch, border="2")
    msg = _setup_error(p3)
    assert "3 trailing border variables" in msg and "accepts 2" in msg, msg
    # not asked for: the usual selection, as if the variable were unset; the count is kept
    _env(monkeypatch, linsolve=None, border="2")
    _, st, info, _ = _short_solve(p3)
    assert st["linsolve"] == 1 and (info["border"], info["over"], info["reason"]) == (0, 3, 1), (st, info)
    # a core too short for the automatic rule (n_core < 2048): the same
    _env(monkeypatch, linsolve=None)
    _, st, info, _ = _short_solve(p3)
    assert st["linsolve"] == 1 and (info["border"], info["over"], info["reason"], info["n_core"]) == (0, 3, 6, 600), (st, info)


def test_ignored_with_a_reason_and_the_order_it_displaces(gpu_required, monkeypatch):
    p = ref.bordered_qp((600, 5, 3))
    # the coupling-row mode keeps precedence
    _env(monkeypatch, linsolve=None, QPDO_BAND_COUPLING="64")
    _, st, info, _ = _short_solve(p)
    assert st["linsolve"] == 1 and (info["border"], info["reason"]) == (0, 3) and "COUPLING" in info["reason_text"], (st, info)
    for ls, want in (("dense", 1), ("pcg", 0)):
        _env(monkeypatch, linsolve=ls)
        _, st, info, _ = _short_solve(p)
        assert st["linsolve"] == want and (info["border"], info["reason"]) == (0, 5), (st, info)
    # a configured band order is ignored on a workspace that adopts a border
    _env(monkeypatch, QPDO_BAND_ORDER="rcm")
    _, st, info, order = _short_solve(p)
    assert st["linsolve"] == 3 and info["border"] == 3 and info["border_solves"] > 0, (st, info)
    assert order["adopted"] == 0 and order["reason"] == 6, order


# ---- (c) whole solves against the oracle ------------------------------------------------------------------------------------------------
def _assert_border(s, c):
    st, info = s.stats(), s.band_border()
    assert st["linsolve"] == 3 and info["border"] == c and info["reason"] == 0, (st, info)
    assert info["border_solves"] > 0 and st["band_fallbacks"] == 0 and st["lin_iters"] == 0, (st, info)
    return st, info


@pytest.mark.parametrize("key", list(ref.ORACLE_RESULTS))
def test_whole_solves_match_the_oracle(key, gpu_required, monkeypatch):
    n_core, bw, c = key
    p = ref.bordered_qp(key)
    # (2100, 3, 2): the band solver is selected automatically from n_core = 2048 up; the smaller ones on request
    _env(monkeypatch, linsolve=None if n_core >= 2048 else "band")
    ro, tro = oracle_run(p)
    assert (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"]) == ref.ORACLE_RESULTS[key]
    s = _workspace(p)
    try:
        res = s.solve()
        res["trace"] = s.trace()
        st, info = _assert_border(s, c)
        geo = s.download_factor("border_geometry")
    finally:
        s.delete()
    print("%s: %s, border_solves %d" % (key, {k: st[k] for k in ("newton_passes", "factor_count", "band_fallbacks")}, info["border_solves"]))
    assert geo == dict(n_core=n_core, c=c, b_core=max(3, bw), np=(n_core + 3) // 4 * 4), geo
    assert st["factor_count"] <= st["newton_passes"], st
    check(res, ro, tro, p)


def test_update_sequence_and_new_matrix_values(gpu_required, monkeypatch):
    p = ref.bordered_qp((600, 5, 3))
    _env(monkeypatch)
    o = ob.OracleSolver(p, ob.default_settings())
    s = _workspace(p)
    try:
        ro, rg = o.solve(), s.solve()
        rg["trace"] = s.trace(); check(rg, ro, o.trace(), p)
        _assert_border(s, 3)
        geo = s.download_factor("border_geometry")
        # update_q, update_bounds, warm_start, solve
        q2 = p["q"] * 1.1 + 0.05
        q2[-3:] = p["q"][-3:] * 1.5
        l2, u2 = p["l"].copy(), p["u"].copy()
        l2[:600] -= 0.05; u2[:600] += 0.02
        for w in (o, s):
            w.update_q(q2); w.update_bounds(l2, u2); w.warm_start(ro["x"], ro["y"])
        p2 = dict(p, q=q2, l=l2, u=u2)
        ro2, rg2 = o.solve(), s.solve()
        rg2["trace"] = s.trace(); check(rg2, ro2, o.trace(), p2)
        _assert_border(s, 3)
        # new values of Q and A in the same pattern: the border is the pattern's and stays
        rng = np.random.default_rng(5)
        A3 = p["A"].copy(); A3.data = A3.data * (1.0 + 0.2 * rng.random(A3.nnz))
        Q3 = p["Q"].copy(); Q3.setdiag(Q3.diagonal() * 1.3)
        s.update_matrices(Q=Q3, A=A3)
        p3 = dict(p2, Q=Q3, A=A3)
        ro3, tr3 = oracle_run(p3)
        rg3 = s.solve()
        rg3["trace"] = s.trace(); check(rg3, ro3, tr3, p3)
        _assert_border(s, 3)
        assert s.download_factor("border_geometry") == geo == dict(n_core=600, c=3, b_core=5, np=600)
    finally:
        s.delete(); o.close()


# ---- (d) no trace -----------------------------------------------------------------------------------------------------------------------
def test_hook_calls_leave_no_trace_on_the_next_solve(gpu_required, monkeypatch):
    p = ref.bordered_qp((600, 5, 3))
    _env(monkeypatch)
    s1 = _workspace(p)
    r1 = s1.solve(); t1 = s1.trace(); st1 = s1.stats(); i1 = s1.band_border()
    s1.delete()
    s2 = _workspace(p)
    try:
        rng = np.random.default_rng(3)
        n, m = p["n"], p["m"]
        dw = 0.1 + 9.9 * rng.random(m)
        s2.direct_solve(dw, 0.5, rng.standard_normal(n), refactor=True)
        dw[-2:] *= 2.0
        s2.direct_solve(dw, 0.5, rng.standard_normal(n), refactor=True)
        r2 = s2.solve(); t2 = s2.trace(); st2 = s2.stats(); i2 = s2.band_border()
        s2.direct_solve(dw, 0.25, rng.standard_normal(n), refactor=True)
        r3 = s2.solve()
    finally:
        s2.delete()
    s4 = _workspace(p)
    s4.solve(); r4b = s4.solve()
    s4.delete()
    for a, b in ((r1, r2), (r4b, r3)):
        assert a["info"]["iterations"] == b["info"]["iterations"] and a["info"]["status_val"] == b["info"]["status_val"]
        assert np.array_equal(_bits(a["x"]), _bits(b["x"])) and np.array_equal(_bits(a["y"]), _bits(b["y"]))
    assert [tr["tau"] for tr in t1] == [tr["tau"] for tr in t2]
    for k in COUNTERS:
        assert st1[k] == st2[k], (k, st1[k], st2[k])
    assert i1 == i2, (i1, i2)


# ---- (e) sensitivities ------------------------------------------------------------------------------------------------------------------
def test_adjoint_and_tangent_on_a_bordered_workspace(W, gpu_required, monkeypatch):
    """one adjoint call (gx, gy) and one tangent call (tq) on (600, 5, 3), the right-hand sides one after the other (rhs_group 1): both code
    0 under the acceptance helpers of tests/test_gpu_workspace_adjoint.py / _tangent.py, and the duality <g, d> = <v, r> within the bound of
    tests/test_gpu_workspace_tangent.py test_duality: the two systems' longdouble residuals times the other solution's 1-norm, plus
    (n + k + 2) eps (|g|.|d| + |v|.|r|)."""
    p = ref.bordered_qp((600, 5, 3))
    n, m = p["n"], p["m"]
    _env(monkeypatch)
    qp = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=10, verbose=0, max_iter=1000)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        _assert_border(qp, 3)
        assert qp.rhs_group() == 1
        c0 = {k: qp.stats()[k] for k in COUNTERS}, qp.band_border()
        rng = np.random.default_rng(41)
        gx, gy, tq = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(n)
        rc, msg, a = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        check_rhs(W, p, sol, a, 0, gx, gy, True, "bordered (600, 5, 3) adjoint")
        rc, msg, d = raw_tangent(qp, dict(tq=tq))
        assert rc == 0, msg
        check_tangent_rhs(p, sol, d, 0, dict(tq=tq), "bordered (600, 5, 3) tangent")
        flags = a["active"]
        assert np.array_equal(flags, d["active"]) and a["status"][0, 0] == 0 and d["status"][0, 0] == 0
        assert ({k: qp.stats()[k] for k in COUNTERS}, qp.band_border()) == c0
        Mk, S = aref.kkt(aref.full_Q(p["Q"], p["Qstype"]), aref.dense(p["A"]), flags)
        k, LD = len(S), aref.LD
        v = np.concatenate([-a["dq"][0].astype(LD), (a["dl"][0] + a["du"][0]).astype(LD)[S]])
        dd = np.concatenate([d["dx"][0].astype(LD), d["dy"][0].astype(LD)[S]])
        g = np.concatenate([gx.astype(LD), gy.astype(LD)[S]])
        rh = sref.tangent_rhs(p["Q"], p["Qstype"], p["A"], flags, sol["x"], sol["y"], **pick(dict(tq=tq), 0))
        rr = np.concatenate([rh["rx"], rh["ry"]])
        e_a, e_t = np.abs(Mk @ v - g).max(), np.abs(Mk @ dd - rr).max()
        lhs, vr, mag = sref.duality_sides(g, dd, v, rr)
        bound = np.abs(v).sum() * e_t + np.abs(dd).sum() * e_a + (n + k + 2) * EPS * mag
        print("duality: |<g,d> - <v,r>| %.3e <= %.3e; magnitude %.3e" % (float(abs(lhs - vr)), float(bound), float(mag)))
        assert abs(lhs - vr) <= bound, (float(abs(lhs - vr)), float(bound))
        assert bound <= 1e-6 * mag, ("the check would be vacuous", float(bound), float(mag))
    finally:
        qp.delete()
