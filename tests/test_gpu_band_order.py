"""The band direct solver under a variable order (qpdo_amd_band_order_config, include/qpdo_amd_ext.h; kernels: the _perm instances of
dev/band.inc and dev/band_wide.inc).

1. The kernels, with an order the test knows: a chain QP p is relabelled even/odd (ps) and the solver is GIVEN the inverse relabelling, so
   its order is the original chain: factor arrays and solves carry the bits of p's natural-order workspace; the factor of P K P' meets the
   derived bounds of test_gpu_direct_solvers.py (|P K P' - L D L'| <= 4 n u |L||D||L'| elementwise, backward error <= 4 n u).
2. Selection: what QPDO_BAND_ORDER=rcm changes, and what ignores it.
3. qpdo_amd_adjoint / qpdo_amd_tangent on an ordered workspace, by the acceptance rules of their own test modules; groups of 8.
4. solve -> sensitivities -> update_matrices -> solve leaves no trace.
All bit comparisons run with scaling = 0."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_wide_ref as bw
from helpers import U64, backward_error, ldl_elementwise_ratio, newton_matrix
from qpdo_amd import problems, solver
from test_gpu_workspace_adjoint import W, bits, raw_adjoint, same_bits  # noqa: F401
from test_gpu_workspace_adjoint import check_rhs as adjoint_check_rhs
from test_gpu_workspace_tangent import check_rhs as tangent_check_rhs
from test_gpu_workspace_tangent import perturbation, pick, raw_tangent

pytestmark = pytest.mark.gpu

ENV_KEYS = ("QPDO_LINSOLVE", "QPDO_DENSE_MID", "QPDO_DENSE_LOOKAHEAD", "QPDO_DENSE_SOLVE", "QPDO_DENSE_LOWRANK", "QPDO_DENSE_UPDOWN", "QPDO_HYBRID",
            "QPDO_DENSE_MAX_N", "QPDO_SMALL_FUSED", "QPDO_PCG_MAXIT", "QPDO_PCG_DENSE_FALLBACK", "QPDO_PCG_SCHUR", "QPDO_BAND_COUPLING", "QPDO_BAND_ORDER",
            "QPDO_AMD_RHS_GROUP")


@pytest.fixture
def env(gpu_required, monkeypatch):
    """a clean environment, and the process-wide order configuration back at its default afterwards"""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    solver.band_order_config("env")
    yield monkeypatch
    solver.band_order_config("env")


def even_odd(n):
    return np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])


def relabelled(p):
    """(ps, shuffle, inv): variable k of ps is variable shuffle[k] of p; GIVEN = inv puts the solver back on p's chain"""
    shuffle = even_odd(p["n"])
    return problems.permute_variables(p, shuffle), shuffle, np.argsort(shuffle)


def linear_workspace(p):
    return solver.QPDO().setup(p["Q"], np.zeros(p["n"]), p["A"], -np.ones(p["m"]), np.ones(p["m"]), Qstype=-1, scaling=0, verbose=0)


def full_Q(p):
    Ql = sp.csr_matrix(p["Q"])
    return (Ql + sp.tril(Ql, -1).T).tocsr()


def factor_arrays(ws, wide):
    return [ws.download_factor(k) for k in (("Wb", "Wd") if wide else ("Kb", "Lt"))]


# ---- 1. the kernels, with an order the test knows -----------------------------------------------------------------------------------------
CASES = [(b, 4 * (b + 1) + extra) for b in (3, 64, 127) for extra in (0, 3)] + [(128, 4 * 129 + 1)]


@pytest.mark.parametrize("b,n", CASES)
def test_given_order_carries_the_natural_bits(b, n, env):
    wide = b > 127
    p = problems.banded_random_qp(300 + b, n, b)
    ps, shuffle, inv = relabelled(p)
    dw = 0.1 + 9.9 * np.random.default_rng(b + n).random(p["m"])
    sigma = 1.0
    Qf, A = full_Q(p), sp.csr_matrix(p["A"])
    bs = bw.rhs_set(Qf, A, sigma, dw, n)                                   # in p's order
    env.setenv("QPDO_LINSOLVE", "band")
    ws = linear_workspace(p)                                               # nothing configured: the natural-order workspace of p
    try:
        assert ws.stats()["linsolve"] == 3 and ws.band_order_info()["adopted"] == 0 and ws.band_order_info()["newold"] is None
        xs_p = [ws.direct_solve(dw, sigma, r, refactor=True) for r in bs]
        g_p, F_p = ws.factor_geometry(), factor_arrays(ws, wide)
        assert solver.band_order(p["Q"], p["A"], -1)[1]["b_natural"] == g_p["b"]      # the host's b_natural is what the device's detection finds
        with pytest.raises(RuntimeError):
            ws.download_factor("perm")
    finally:
        ws.delete()
    solver.band_order_config("given", inv)
    ws = linear_workspace(ps)
    try:
        info = ws.band_order_info()
        assert ws.stats()["linsolve"] == 3
        assert info["mode"] == solver.BAND_ORDER_GIVEN and info["adopted"] == 1 and info["reason"] == 0 and info["b_ordered"] == b and info["b_natural"] > b, info
        assert np.array_equal(info["newold"], inv) and np.array_equal(ws.download_factor("perm"), inv)
        xs_s = [ws.direct_solve(dw, sigma, r[shuffle], refactor=True) for r in bs]
        g = ws.factor_geometry()
        assert g == g_p and g["b"] == b and g["np"] == ((n + 63) // 64 * 64 if wide else (n + 3) // 4 * 4), (g, g_p)
        F = factor_arrays(ws, wide)
        # the same call twice: the same bits
        assert same_bits(ws.direct_solve(dw, sigma, bs[0][shuffle], refactor=True), xs_s[0])
        for a, c in zip(factor_arrays(ws, wide), F):
            assert same_bits(a, c)
        # a kept factor, the solve on its own
        assert same_bits(ws.direct_solve(dw, sigma, bs[1][shuffle], refactor=False), xs_s[1])
    finally:
        ws.delete()
    # the factor and the solves are p's, bit for bit (the solution un-shuffled)
    for a, c, name in zip(F, F_p, ("Wb", "Wd") if wide else ("Kb", "Lt")):
        assert same_bits(a, c), name
    for x_s, x_p in zip(xs_s, xs_p):
        assert same_bits(x_s, x_p[shuffle])
    # ... and it is a factor of P K P', K the Newton matrix of ps, by the bounds of test_gpu_direct_solvers.py
    if wide:
        L, D = bw.unpack(F[0], F[1], n, b)
    else:
        Kb, D = F[0], F[0][:n, 0]
        L = np.eye(n)
        for t in range(1, b + 1):
            j = np.arange(n - t)
            L[j + t, j] = Kb[j, t]
    assert np.all(np.isfinite(D)) and np.all(D > 0)
    Qs, As = full_Q(ps), sp.csr_matrix(ps["A"])
    K = newton_matrix(Qs, As, sigma, dw)
    PKP = K[np.ix_(inv, inv)]
    elem = ldl_elementwise_ratio(PKP, L, D)
    eta = max(backward_error(Qs, As, sigma, dw, x, r[shuffle], K=K) for x, r in zip(xs_s, bs)) / (n * U64)
    print("ordered band b=%d n=%d: elementwise %.3g, eta / (n u) %.3g" % (b, n, elem, eta))
    assert elem <= 1.0, elem
    assert eta <= 4.0, eta


@pytest.mark.parametrize("b,n", [(3, 19), (128, 517)])
def test_identity_order_is_the_unconfigured_workspace(b, n, env):
    """GIVEN = identity is adopted -- the permuted kernels run -- and delivers the bits of the workspace with nothing configured"""
    wide = b > 127
    p = problems.banded_random_qp(300 + b, n, b)
    dw = 0.1 + 9.9 * np.random.default_rng(n).random(p["m"])
    rhs = np.random.default_rng(n + 1).standard_normal(n)
    env.setenv("QPDO_LINSOLVE", "band")
    out = []
    for given in (False, True):
        solver.band_order_config("given", np.arange(n)) if given else solver.band_order_config("env")
        ws = linear_workspace(p)
        try:
            assert ws.band_order_info()["adopted"] == int(given) and ws.stats()["linsolve"] == 3
            x = ws.direct_solve(dw, 1.0, rhs, refactor=True)
            out.append([x] + factor_arrays(ws, wide) + [ws.factor_geometry()])
        finally:
            ws.delete()
    assert out[0][3] == out[1][3]
    for a, c in zip(out[0][:3], out[1][:3]):
        assert same_bits(a, c)


# ---- 2. selection ---------------------------------------------------------------------------------------------------------------------------
def test_rcm_brings_a_relabelled_chain_back_to_the_band_solver(env):
    p = problems.banded_qp(1, 2048)
    ps = problems.permute_variables(p, even_odd(2048))
    # unset: the relabelled chain is not seen as banded and takes the dense factor -- the behaviour without this feature
    ws = solver.QPDO().setup(ps["Q"], ps["q"], ps["A"], ps["l"], ps["u"], Qstype=-1, verbose=0)
    try:
        assert ws.stats()["linsolve"] == 1
        info = ws.band_order_info()
        assert info["mode"] == solver.BAND_ORDER_NATURAL and info["adopted"] == 0 and info["reason"] == 0
    finally:
        ws.delete()
    env.setenv("QPDO_BAND_ORDER", "rcm")
    r = solver.solve_problem(ps, verbose=0)
    assert r["stats"]["linsolve"] == 3 and r["info"]["status_val"] == 1, (r["stats"]["linsolve"], r["info"])
    rp, rd = problems.kkt_residuals(ps, r["x"], r["y"])
    assert rp <= 1e-6 and rd <= 1e-6 and abs(rp - r["info"]["res_prim_norm"]) <= 1e-9 and abs(rd - r["info"]["res_dual_norm"]) <= 1e-9, (rp, rd)
    ws = solver.QPDO().setup(ps["Q"], ps["q"], ps["A"], ps["l"], ps["u"], Qstype=-1, verbose=0)
    try:
        info = ws.band_order_info()
        assert info["mode"] == solver.BAND_ORDER_RCM and info["adopted"] == 1 and info["b_natural"] == 1024 and info["b_ordered"] <= 3 and info["order_seconds"] > 0, info
        host_newold, host_info = solver.band_order(ps["Q"], ps["A"], -1)
        assert np.array_equal(info["newold"], host_newold) and host_info["b_ordered"] == info["b_ordered"]
    finally:
        ws.delete()
    # an order that is already optimal is not adopted: the natural-order workspace
    ws = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0)
    try:
        info = ws.band_order_info()
        assert ws.stats()["linsolve"] == 3 and info["adopted"] == 0 and info["reason"] == 1 and info["b_ordered"] == info["b_natural"] == 1, info
    finally:
        ws.delete()


def test_band_on_request_under_rcm(env):
    env.setenv("QPDO_LINSOLVE", "band")
    # a relabelled b = 130 chain: not banded in the caller's order (n < 4 (b + 1)), the tiled route under the order
    p = problems.banded_random_qp(7, 1100, 130)
    ps = problems.permute_variables(p, even_odd(1100))
    with pytest.raises(RuntimeError):
        linear_workspace(ps)
    env.setenv("QPDO_BAND_ORDER", "rcm")
    ws = linear_workspace(ps)
    try:
        info = ws.band_order_info()
        assert ws.stats()["linsolve"] == 3 and info["adopted"] == 1 and 127 < info["b_ordered"] < 275, info
        dw = 0.1 + 9.9 * np.random.default_rng(1).random(ps["m"])
        rhs = np.random.default_rng(2).standard_normal(1100)
        x = ws.direct_solve(dw, 1.0, rhs, refactor=True)
        g = ws.factor_geometry()
        assert g["b"] == info["b_ordered"] and g["np"] == 1152 and ws.download_factor("Wd").shape == (1152,)
        Qs, As = full_Q(ps), sp.csr_matrix(ps["A"])
        assert backward_error(Qs, As, 1.0, dw, x, rhs) <= 4.0 * 1100 * U64
    finally:
        ws.delete()
    # no order brings this one under 1023: refused, and the message names the ordered bandwidth
    pr = problems.random_qp(3, 2500, 3000, 0.01)
    _, host_info = solver.band_order(pr["Q"], pr["A"], pr["Qstype"])
    assert host_info["b_ordered"] > 1023 and host_info["early_out"] == 0
    with pytest.raises(RuntimeError) as e:
        solver.solve_problem(pr, verbose=0)
    assert "1023" in str(e.value) and ("%d under the configured band order" % host_info["b_ordered"]) in str(e.value), str(e.value)


def test_workspaces_that_ignore_the_order(env):
    p = problems.banded_random_qp(7, 64, 3)
    env.setenv("QPDO_BAND_ORDER", "rcm")
    for var, val, reason in (("QPDO_BAND_COUPLING", "4", 3), ("QPDO_LINSOLVE", "dense", 5), ("QPDO_LINSOLVE", "pcg", 5), (None, None, 4)):
        env.setenv("QPDO_LINSOLVE", "band")
        if var:
            env.setenv(var, val)
        else:
            env.delenv("QPDO_LINSOLVE")                                   # defaults at n = 64: the fused small-problem route
        ws = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=0, verbose=0)
        try:
            info = ws.band_order_info()
            assert info["mode"] == solver.BAND_ORDER_RCM and info["adopted"] == 0 and info["reason"] == reason and info["newold"] is None, (var, val, info)
            assert info["reason_text"] == solver.BAND_ORDER_REASONS[reason]
            if var == "QPDO_BAND_COUPLING":
                assert ws.stats()["linsolve"] == 3
        finally:
            ws.delete()
        if var:
            env.delenv(var)
    # a GIVEN order of another length fails the setup
    solver.band_order_config("given", np.arange(63))
    with pytest.raises(RuntimeError) as e:
        solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=0, verbose=0)
    assert "63 entries" in str(e.value) and "64 variables" in str(e.value), str(e.value)
    solver.band_order_config("env")
    env.setenv("QPDO_BAND_ORDER", "amd")
    with pytest.raises(RuntimeError) as e:
        solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=0, verbose=0)
    assert "QPDO_BAND_ORDER=amd" in str(e.value), str(e.value)


# ---- 3. sensitivities -------------------------------------------------------------------------------------------------------------------------
def ordered_workspace(env, ps, inv):
    env.setenv("QPDO_LINSOLVE", "band")
    solver.band_order_config("given", inv)
    return solver.QPDO().setup(ps["Q"], ps["q"], ps["A"], ps["l"], ps["u"], Qstype=ps["Qstype"], c=0.0, scaling=0, verbose=0, max_iter=1000)


def test_adjoint_and_tangent_on_an_ordered_workspace(W, env):
    b, n = 64, 4 * 65 + 3
    ps, shuffle, inv = relabelled(problems.banded_random_qp(300 + b, n, b))
    qp = ordered_workspace(env, ps, inv)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1 and qp.stats()["linsolve"] == 3 and qp.band_order_info()["adopted"] == 1 and qp.rhs_group() == 8
        rng = np.random.default_rng(64)
        for R in (3, 11):
            gx = rng.standard_normal((R, n))
            rc, msg, o0 = raw_adjoint(qp, gx[0])
            assert rc == 0, msg
            gy = rng.standard_normal((R, ps["m"]))
            gy[:, o0["active"] == 0] = np.nan
            rc, msg, many = raw_adjoint(qp, gx, gy, matrices=True)
            assert rc == 0, msg
            t = perturbation(ps, rng, R)
            rc, msg, tmany = raw_tangent(qp, t)
            assert rc == 0, msg
            for r in range(R):
                rc, msg, one = raw_adjoint(qp, gx[r], gy[r], matrices=True)
                assert rc == 0, msg
                for k in ("dq", "dl", "du", "dQ_values", "dA_values", "residual"):
                    assert same_bits(many[k][r], one[k][0]), ("adjoint", R, r, k)
                assert many["status"][r].tolist() == one["status"][0].tolist()
                rc, msg, tone = raw_tangent(qp, pick(t, r))
                assert rc == 0, msg
                for k in ("dx", "dy", "residual"):
                    assert same_bits(tmany[k][r], tone[k][0]), ("tangent", R, r, k)
                assert tmany["status"][r].tolist() == tone["status"][0].tolist()
                if R == 3:                                                 # the acceptance rules of the two calls' own tests
                    assert adjoint_check_rhs(W, ps, sol, many, r, gx[r], gy[r], True, "ordered band adjoint rhs %d" % r) == 0
                    assert tangent_check_rhs(ps, sol, tmany, r, t, "ordered band tangent rhs %d" % r)[0] == 0
        assert qp.rhs_group() == 8
    finally:
        qp.delete()


# ---- 4. no trace ------------------------------------------------------------------------------------------------------------------------------
def sequence(qp, p, rng):
    """solve -> adjoint, tangent -> update_matrices -> solve; everything it delivers, and factor_count after each stage"""
    out, counts = [], []
    s1 = qp.solve()
    counts.append(qp.stats()["factor_count"])
    a = qp.adjoint(rng.standard_normal((3, p["n"])), None, matrices=True)
    t = qp.tangent(tq=rng.standard_normal((3, p["n"])))
    counts.append(qp.stats()["factor_count"])
    qp.update_matrices(Q=p["Q"] * 1.25, A=p["A"] * 0.5)
    s2 = qp.solve()
    counts.append(qp.stats()["factor_count"])
    assert s1["info"]["status_val"] == 1 and s2["info"]["status_val"] == 1
    out += [s1["x"], s1["y"], a["dq"], a["dl"], a["du"], a["dQ_values"], a["dA_values"], t["dx"], t["dy"], s2["x"], s2["y"]]
    return out, counts, [s1["info"]["iterations"], s2["info"]["iterations"]]


def test_sequence_leaves_no_trace(env):
    b, n = 64, 4 * 65 + 3
    p = problems.banded_random_qp(300 + b, n, b)
    ps, shuffle, inv = relabelled(p)
    runs = []
    for _ in range(2):                                                     # the same sequence on two fresh ordered workspaces, twice over on each
        qp = ordered_workspace(env, ps, inv)
        try:
            assert qp.band_order_info()["adopted"] == 1
            first = sequence(qp, ps, np.random.default_rng(5))
            qp.update_matrices(Q=ps["Q"], A=ps["A"])
            second = sequence(qp, ps, np.random.default_rng(5))
            assert qp.band_order_info()["adopted"] == 1 and np.array_equal(qp.download_factor("perm"), inv)      # the pattern is fixed: the order stays
        finally:
            qp.delete()
        for a, c in zip(first[0], second[0]):
            assert same_bits(a, c)
        assert first[2] == second[2] and np.array_equal(np.diff(first[1]), np.diff(second[1]))
        runs.append(first)
    for a, c in zip(runs[0][0], runs[1][0]):
        assert same_bits(a, c)
    assert runs[0][1] == runs[1][1]
    # factor_count moves as on a natural band workspace: p with the identity GIVEN (the permuted kernels) against p with nothing configured
    # (the natural ones) -- the same arithmetic, so the same bits and the same counts at every stage
    both = []
    for given in (True, False):
        solver.band_order_config("given", np.arange(n)) if given else solver.band_order_config("env")
        env.setenv("QPDO_LINSOLVE", "band")
        qp = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, c=0.0, scaling=0, verbose=0, max_iter=1000)
        try:
            assert qp.band_order_info()["adopted"] == int(given)
            both.append(sequence(qp, p, np.random.default_rng(5)))
        finally:
            qp.delete()
    assert both[0][1] == both[1][1] and both[0][2] == both[1][2], (both[0][1], both[1][1])
    for a, c in zip(both[0][0], both[1][0]):
        assert same_bits(a, c)
    # the relabelled workspace's solves take the same passes' factorizations where the iterates agree to rounding: report, do not pin
    print("factor_count: ordered relabelled %s, natural %s" % (runs[0][1], both[1][1]))
