"""The workspace adjoint / tangent and their groups of right-hand sides (include/qpdo_amd_ext.h) on the two band kinds the calls
used to refuse, on the MI355X, in this process:
  * the WIDE band (half-bandwidth 128 .. 1023, dev/band_wide.inc), in the natural order and under an adopted variable order
    (QPDO_BAND_ORDER=rcm): the single solves run k_bw_solve[_perm], the groups k_bw_solve_group[_perm];
  * the band WITH COUPLING ROWS (QPDO_BAND_COUPLING): K = B + U W_c U' is solved by ONE Woodbury application per sweep (host_band.inc
    band_coupled_apply; the groups: k_band_solve_group, k_bc_t_group, k_bc_apply_group).  tests/test_workspace_band_sens_cpu.py
    emulate_sweeps() is the float64 emulation of that scheme: it pins these instances (accepted within 20 sweeps, positive pivots of S, the
    duplicated coupling row ends as code 1 and never as code 3) without a device.
The helpers, the acceptance rules and the tolerances are those of tests/test_gpu_workspace_adjoint.py, tests/test_gpu_workspace_tangent.py
and tests/test_gpu_workspace_group.py, imported from there; nothing here sets a tolerance of its own.  Group checks are BITWISE."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_coupled_ref as bref
import fleet_adjoint_ref as ref
import test_gpu_workspace_adjoint as TA
import test_gpu_workspace_group as TG
import test_gpu_workspace_tangent as TT
import test_workspace_band_sens_cpu as EM
from qpdo_amd import problems, solver
from test_gpu_workspace_adjoint import W, bits, check_rhs, raw_adjoint, same_bits, snapshot  # noqa: F401
from test_gpu_workspace_group import A_KEYS, rounds_of, same_outputs, slab_is_single
from test_gpu_workspace_tangent import O_KEYS, perturbation, pick, raw_tangent

pytestmark = pytest.mark.gpu

WIDE = {
    "b128": lambda: problems.banded_random_qp(428, 516, 128),                    # w = 2, np = 576 != n
    "b129": lambda: problems.banded_random_qp(429, 521, 129, win=130),           # w = 3
    "b260": lambda: problems.banded_random_qp(611, 1100, 260, win=64),           # w = 5: each wave's second trip in bw_sweep
}
_cache = {}


def wide(name):
    if name not in _cache:
        _cache[name] = WIDE[name]()
    return _cache[name]


def hidden(p, seed=5):
    """p with its variables in a fixed random order: a band only QPDO_BAND_ORDER=rcm finds again"""
    key = ("hidden", id(p), seed)
    if key not in _cache:
        _cache[key] = problems.permute_variables(p, np.random.default_rng(seed).permutation(p["n"]))
    return _cache[key]


def coupled(name):
    """(problem, number of coupling rows); name: a key of EM.COUPLED_KEYS, "free" or "dup" """
    if name == "free":
        return EM.free_rows_instance(), 2
    if name == "dup":
        return EM.dup_instance(), 4
    return EM.coupled_instance(name), name[2]


def workspace(monkeypatch, p, scaling, env=None, **kw):
    monkeypatch.delenv("QPDO_BAND_ORDER", raising=False)
    return TG.workspace(monkeypatch, p, "band", scaling, env=env, **kw)


COUPLING = {"QPDO_BAND_COUPLING": "64"}
COUNTERS = ("factor_count", "coupled_rows", "coupled_solves", "coupled_sweeps", "coupled_rejects", "band_fallbacks")


def counters(qp):
    st = qp.stats()
    return {k: st[k] for k in COUNTERS}


def assert_wide(qp, what):
    assert qp.stats()["linsolve"] == 3 and qp.factor_geometry()["b"] > 127, (what, qp.stats()["linsolve"], qp.factor_geometry())


def adjoint_and_tangent(W, qp, p, sol, scaling, what):
    """per instance: the adjoint with gy = None and with a gy that is NaN off S (matrices=True), the tangent with all five arrays and NaN on
    the ignored entries, tangent(tq) against adjoint(gx = tq) exactly.  Returns the delivered flags."""
    rng = np.random.default_rng(100 + scaling)
    gx = rng.standard_normal(p["n"])
    rc, msg, o = raw_adjoint(qp, gx, None, matrices=True)
    assert rc == 0, msg
    check_rhs(W, p, sol, o, 0, gx, None, True, what + " gy=None")
    flags = o["active"].copy()
    gy = rng.standard_normal(p["m"])
    gy[flags == 0] = np.nan
    rc, msg, o2 = raw_adjoint(qp, gx, gy, matrices=True)
    assert rc == 0, msg
    assert np.array_equal(o2["active"], flags)
    check_rhs(W, p, sol, o2, 0, gx, gy, True, what + " gy")
    # the tangent: every entry the call ignores holds NaN
    t = perturbation(p, rng, 1)
    A = sp.csc_matrix(p["A"]); A.sort_indices()
    clean = {k: v.copy() for k, v in t.items()}
    for k in ("tl", "tu", "tA_values"):
        clean[k][:, (flags != -1) if k == "tl" else (flags != 1) if k == "tu" else (flags[A.indices] == 0)] = 0.0
    t["tl"][:, flags != -1] = np.nan
    t["tu"][:, flags != 1] = np.nan
    t["tA_values"][:, flags[A.indices] == 0] = np.nan
    rc, msg, ot = raw_tangent(qp, t)
    assert rc == 0, msg
    assert np.array_equal(ot["active"], flags)
    TT.check_rhs(p, sol, ot, 0, clean, what + " tangent, all five")
    # one driver
    tq = rng.standard_normal((2, p["n"]))
    rc, msg, a = raw_adjoint(qp, tq, None)
    assert rc == 0 and (a["status"][:, 0] == 0).all(), (msg, a["status"].tolist())
    rc, msg, d = raw_tangent(qp, dict(tq=tq))
    assert rc == 0, msg
    assert np.array_equal(d["dx"], a["dq"]) and np.array_equal(d["dy"], -(a["dl"] + a["du"])), what
    assert np.array_equal(d["status"], a["status"]) and same_bits(d["residual"], a["residual"]) and (a["status"][:, 1] >= 1).all()
    return flags, o, o2


# ---- 1. the wide band -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scaling", [("b128", 10), ("b128", 0), ("b129", 10), ("b129", 0), ("b260", 10)])
def test_wide_band(W, monkeypatch, name, scaling):
    p = wide(name)
    qp = workspace(monkeypatch, p, scaling)
    try:
        sol = qp.solve()
        what = "wide %s[%d]" % (name, scaling)
        assert sol["info"]["status_val"] == 1, (what, sol["info"])
        assert_wide(qp, what)
        assert qp.rhs_group() == 8
        c0 = counters(qp)
        adjoint_and_tangent(W, qp, p, sol, scaling, what)
        assert counters(qp) == c0, what
    finally:
        qp.delete()


def test_wide_band_under_an_adopted_order(W, monkeypatch):
    p = hidden(wide("b129"))
    qp = workspace(monkeypatch, p, 10, env={"QPDO_BAND_ORDER": "rcm"})
    try:
        sol = qp.solve()
        info = qp.band_order_info()
        assert sol["info"]["status_val"] == 1 and info["adopted"] and info["b_ordered"] > 127, (sol["info"], info)
        assert_wide(qp, "wide b129 rcm")
        assert qp.rhs_group() == 8
        adjoint_and_tangent(W, qp, p, sol, 10, "wide b129 rcm")
    finally:
        qp.delete()


# ---- 2. coupling rows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("key", EM.COUPLED_KEYS)
def test_coupled(W, monkeypatch, key, scaling):
    p, r = coupled(key)
    m = p["m"]
    qp = workspace(monkeypatch, p, scaling, env=COUPLING)
    try:
        sol = qp.solve()
        what = "coupled %s[%d]" % (key, scaling)
        assert sol["info"]["status_val"] == 1 and qp.stats()["linsolve"] == 3, (what, sol["info"], qp.stats()["linsolve"])
        assert qp.stats()["coupled_rows"] == r and qp.rhs_group() == 8, (what, qp.stats()["coupled_rows"], qp.rhs_group())
        c0 = counters(qp)
        flags, o, o2 = adjoint_and_tangent(W, qp, p, sol, scaling, what)
        assert counters(qp) == c0, (what, c0, counters(qp))
        # a coupling row is active where the CPU classification says so: the Woodbury application ran, and dAx on those rows passed check_matrices
        l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
        cpu = ref.classify(sol["x"], sol["y"], ref.dense(p["A"]), l, u)
        assert (cpu[m - r:] != 0).any() and (flags[m - r:] != 0).any(), (what, cpu[m - r:], flags[m - r:])
        A = sp.csc_matrix(p["A"]); A.sort_indices()
        on_coupling = (A.indices >= m - r) & (flags[A.indices] != 0)
        assert on_coupling.any() and np.abs(o2["dA_values"][0][on_coupling]).max() > 0, what
        print("%s: sweeps gy=None %d, gy %d" % (what, o["status"][0, 1], o2["status"][0, 1]))
    finally:
        qp.delete()


@pytest.mark.parametrize("scaling", [10, 0])
def test_coupled_without_a_flagged_coupling_row(W, monkeypatch, scaling):
    """two coupling rows with no finite bound: never flagged, the adjoint's k is 0 and the plain band solve on B is the whole solve"""
    p, r = coupled("free")
    qp = workspace(monkeypatch, p, scaling, env=COUPLING)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1 and qp.stats()["linsolve"] == 3 and qp.stats()["coupled_rows"] == 2
        c0 = counters(qp)
        flags, o, o2 = adjoint_and_tangent(W, qp, p, sol, scaling, "coupled, free rows[%d]" % scaling)
        assert not flags[-2:].any() and counters(qp) == c0
        assert qp.download_factor("coupled_geometry")["k"] == 0
    finally:
        qp.delete()


# ---- 3. groups, both kinds ------------------------------------------------------------------------------------------------------------------------
GROUP_CASES = {"wide b128": ("b128", None, None), "wide b129 rcm": ("b129", None, "rcm"), "coupled (600, 5, 3)": (None, (600, 5, 3), None),
               "coupled (520, 12, 8)": (None, (520, 12, 8), None)}


def group_case(case):
    wname, ckey, order = GROUP_CASES[case]
    if wname:
        p = wide(wname)
        return (hidden(p) if order else p), ({"QPDO_BAND_ORDER": order} if order else {})
    return coupled(ckey)[0], dict(COUPLING)


@pytest.mark.parametrize("case", list(GROUP_CASES))
def test_groups_against_singles(monkeypatch, case):
    """R = 2, 8 and 11 right-hand sides of both calls: every slab carries the bits of the nrhs = 1 call with that slab, the same call twice
    gives the same bits, the counters say that ceil(R / 8) groups ran with one read-back per sweep each.  On the coupled instances the
    right-hand sides with an even number have gy = 0 and the others a random gy: the sweep counts differ inside a group (the emulation: 3
    against 4 - 6)."""
    p, env = group_case(case)
    n, m = p["n"], p["m"]
    is_coupled = "QPDO_BAND_COUPLING" in env
    qp = workspace(monkeypatch, p, 10, env=env)
    try:
        assert qp.solve()["info"]["status_val"] == 1
        assert qp.rhs_group() == 8 and qp.group_stats()["group"] == 8 and qp.group_stats()["scratch_bytes"] == 0
        rng = np.random.default_rng(77)
        RMAX = 11
        gx, gy = rng.standard_normal((RMAX, n)), rng.standard_normal((RMAX, m))
        if is_coupled:
            gy[0::2] = 0.0
        t = perturbation(p, rng, RMAX)
        a_one, t_one = [], []
        for r in range(RMAX):
            rc, msg, o = raw_adjoint(qp, gx[r], gy[r])
            assert rc == 0 and o["status"][0, 0] == 0, (msg, o["status"].tolist())
            a_one.append(o)
            rc, msg, o = raw_tangent(qp, pick(t, r))
            assert rc == 0 and o["status"][0, 0] == 0, (msg, o["status"].tolist())
            t_one.append(o)
        assert qp.group_stats()["scratch_bytes"] == 0, "single calls allocate nothing of the group's"
        for R in (2, 8, 11):
            for kind in ("adjoint", "tangent"):
                def call():
                    if kind == "adjoint":
                        return raw_adjoint(qp, gx[:R], gy[:R])
                    return raw_tangent(qp, {k: v[:R] for k, v in t.items()})
                s0 = qp.group_stats()
                rc, msg, many = call()
                assert rc == 0, msg
                s1 = qp.group_stats()
                assert s1["groups_run"] - s0["groups_run"] == (R + 7) // 8, (case, kind, R, s0, s1)
                assert s1["rounds_total"] - s0["rounds_total"] == rounds_of(many["status"], 8), (case, kind, R, s0, s1, many["status"].tolist())
                assert s1["scratch_bytes"] > 0 and s1["group"] == 8
                rc, msg, again = call()
                assert rc == 0, msg
                keys = A_KEYS if kind == "adjoint" else O_KEYS
                same_outputs(many, again, keys, (case, kind, R, "the same call twice"))
                for r in range(R):
                    slab_is_single(many, r, (a_one if kind == "adjoint" else t_one)[r], keys, (case, kind, R))
                if kind == "adjoint" and R == 8:
                    sw = many["status"][:, 1]
                    print("%s: sweeps of the R = 8 adjoint group %s" % (case, sw.tolist()))
                    if is_coupled:
                        assert len(set(sw.tolist())) > 1 and sw[0::2].max() < sw[1::2].max(), (case, "sweep counts inside a group", sw.tolist())
        sb = qp.group_stats()["scratch_bytes"]
        assert sb >= 8 * 5 * (n + m) * 8 and sb == s1["scratch_bytes"], "allocated once"
    finally:
        qp.delete()


@pytest.mark.parametrize("case", ["wide b128", "coupled (600, 5, 3)"])
def test_the_switch(monkeypatch, case):
    """QPDO_AMD_RHS_GROUP=1 and =3 workspaces carry the default workspace's bits"""
    p, env = group_case(case)
    D = workspace(monkeypatch, p, 10, env=env)
    S = workspace(monkeypatch, p, 10, env=dict(env, QPDO_AMD_RHS_GROUP="1"))
    T3 = workspace(monkeypatch, p, 10, env=dict(env, QPDO_AMD_RHS_GROUP="3"))
    try:
        for q in (D, S, T3):
            assert q.solve()["info"]["status_val"] == 1
        assert (D.rhs_group(), S.rhs_group(), T3.rhs_group()) == (8, 1, 3)
        rng = np.random.default_rng(5)
        R = 8
        gx, gy = rng.standard_normal((R, p["n"])), rng.standard_normal((R, p["m"]))
        t = perturbation(p, rng, R)
        for kind, keys in (("adjoint", A_KEYS), ("tangent", O_KEYS)):
            outs = []
            for q, G in ((D, 8), (S, 1), (T3, 3)):
                s0 = q.group_stats()
                rc, msg, o = raw_adjoint(q, gx, gy, matrices=True) if kind == "adjoint" else raw_tangent(q, t)
                assert rc == 0 and (o["status"][:, 0] == 0).all(), (msg, o["status"].tolist())
                s1 = q.group_stats()
                assert s1["groups_run"] - s0["groups_run"] == (R + G - 1) // G, (kind, G, s0, s1)
                assert s1["rounds_total"] - s0["rounds_total"] == rounds_of(o["status"], G), (kind, G, s0, s1, o["status"].tolist())
                outs.append(o)
            same_outputs(outs[0], outs[1], keys, (case, kind, "default against QPDO_AMD_RHS_GROUP=1"))
            same_outputs(outs[0], outs[2], keys, (case, kind, "default against QPDO_AMD_RHS_GROUP=3"))
        assert S.group_stats()["scratch_bytes"] == 0 and T3.group_stats()["scratch_bytes"] > 0
    finally:
        D.delete(); S.delete(); T3.delete()


# ---- 4. code 1 on a coupled workspace -----------------------------------------------------------------------------------------------------------
def test_not_accepted_on_a_coupled_workspace(W, monkeypatch):
    """the equality coupling row stored twice (the recipe of the adjoint's test_not_accepted): gy = (+1, -1) on the two copies is code 1 at
    20 sweeps with NaN slices, gy = None code 0; one R = 3 call gives 0, 1, 0 with slabs 0 and 2 bitwise the single calls.  The pivots of
    S stay positive (2.7e-8 the smallest, tests/test_workspace_band_sens_cpu.py): code 3 never appears."""
    p, r = coupled("dup")
    m = p["m"]
    qp = workspace(monkeypatch, p, 10, env=COUPLING)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1 and qp.stats()["coupled_rows"] == r, (sol["info"], qp.stats()["coupled_rows"])
        gx = np.random.default_rng(3).standard_normal(p["n"])
        gy = np.zeros(m)
        gy[m - 2], gy[m - 1] = 1.0, -1.0
        rc, msg, bad = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0, msg
        assert bad["status"][0, :2].tolist() == [1, 20] and bad["active"][m - 2] != 0 and bad["active"][m - 1] != 0, bad["status"].tolist()
        check_rhs(W, p, sol, bad, 0, gx, gy, True, "inconsistent gy", accept=(1,))
        rc, msg, ok = raw_adjoint(qp, gx, None, matrices=True)
        assert rc == 0, msg
        check_rhs(W, p, sol, ok, 0, gx, None, True, "gy=None")
        assert np.array_equal(ok["active"], bad["active"])
        gx3 = np.stack([gx, gx, 2.0 * gx])
        gy3 = np.stack([np.zeros(m), gy, np.zeros(m)])
        rc, msg, mix = raw_adjoint(qp, gx3, gy3, matrices=True)
        assert rc == 0 and mix["status"][:, 0].tolist() == [0, 1, 0] and mix["status"][1, 1] == 20, (msg, mix["status"].tolist())
        for k in range(3):
            check_rhs(W, p, sol, mix, k, gx3[k], gy3[k], True, "mixed call, right-hand side %d" % k, accept=((1,) if k == 1 else (0,)))
        for k in (0, 2):
            rc, msg, one = raw_adjoint(qp, gx3[k], gy3[k], matrices=True)
            assert rc == 0, msg
            slab_is_single(mix, k, one, A_KEYS, "beside a code 1")
        assert qp.stats()["coupled_rejects"] == 0
    finally:
        qp.delete()


# ---- 5. no trace ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["wide b128", "coupled (600, 5, 3)"])
def test_no_bit_moves(monkeypatch, case):
    """two workspaces on one problem, calls of both kinds with nrhs = 1 and nrhs = 11 on X only: the counters of QPDOAmdStats stay, and every
    later solve of X carries Y's bits -- x, y, info, every trace record, every QPDOAmdStats member but the timings"""
    p, env = group_case(case)
    is_coupled = "QPDO_BAND_COUPLING" in env
    X, Y = workspace(monkeypatch, p, 10, env=env), workspace(monkeypatch, p, 10, env=env)
    try:
        rng = np.random.default_rng(5)
        R = 11
        gx, gy = rng.standard_normal((R, p["n"])), rng.standard_normal((R, p["m"]))
        t = perturbation(p, rng, R)

        def calls_on_X():
            for args in ((gx[0], gy[0]), (gx, gy)):
                rc, msg, o = raw_adjoint(X, *args, matrices=True)
                assert rc == 0 and (o["status"][:, 0] == 0).all(), (msg, o["status"].tolist())
            for tt in (pick(t, 0), t):
                rc, msg, o = raw_tangent(X, tt)
                assert rc == 0 and (o["status"][:, 0] == 0).all(), (msg, o["status"].tolist())

        a, b = X.solve(), Y.solve()
        assert a["info"]["status_val"] == 1 and snapshot(X, a) == snapshot(Y, b)
        calls_on_X()
        assert snapshot(X, a)["stats"] == snapshot(Y, b)["stats"], "QPDOAmdStats after the calls"
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "the solve after the calls"
        calls_on_X()
        for S in (X, Y):
            S.update_q(1.5 * p["q"] + 0.1)
            S.warm_start(a["x"], a["y"])
        a, b = X.solve(), Y.solve()
        assert a["info"]["status_val"] == 1 and snapshot(X, a) == snapshot(Y, b), "update_q, warm_start, solve"
        if is_coupled:
            calls_on_X()
            A2 = sp.csc_matrix(p["A"]).copy(); A2.sort_indices()
            A2.data = A2.data * (1.0 + 0.01 * np.cos(np.arange(A2.nnz)))
            for S in (X, Y):
                S.update_matrices(A=A2)
            a, b = X.solve(), Y.solve()
            assert snapshot(X, a) == snapshot(Y, b), "update_matrices, solve"
            rc, msg, o = raw_adjoint(X, gx[:2], gy[:2])
            assert rc == 0 and (o["status"][:, 0] != 3).all(), (msg, o["status"].tolist())
            a, b = X.solve(), Y.solve()
            assert snapshot(X, a) == snapshot(Y, b), "the solve after a call on the new matrices"
        assert Y.group_stats()["groups_run"] == 0 and Y.group_stats()["scratch_bytes"] == 0 and Y.adjoint_stats()["calls"] == 0
    finally:
        X.delete(); Y.delete()


# ---- 6. the layer ---------------------------------------------------------------------------------------------------------------------------------
def test_workspace_qp_layer_on_a_coupled_workspace(W, monkeypatch):
    """WorkspaceQP forward / backward on coupled (600, 5, 3): backward equals the direct call bit for bit and passes check_rhs; one
    finite-difference spot check of dL/dq_j, with the bound of test_gpu_workspace_adjoint.py test_workspace_qp_layer (derived there): the two
    solves' KKT residuals weighted with the REFERENCE's adjoint solution, over 2 h, plus the adjoint's own error bound."""
    import torch
    from qpdo_amd.torch_layer import WorkspaceQP
    p, r = coupled((600, 5, 3))
    qp = workspace(monkeypatch, p, 0, env=COUPLING, eps_abs=1e-9, max_iter=10000)
    try:
        Qp = sp.csc_matrix(p["Q"]); Qp.sort_indices()
        Ap = sp.csc_matrix(p["A"]); Ap.sort_indices()
        rng = np.random.default_rng(21)
        w, z = rng.standard_normal(p["n"]), rng.standard_normal(p["m"])
        wt, zt = torch.from_numpy(w), torch.from_numpy(z)
        vals = [p["q"], p["l"], p["u"], Qp.data, Ap.data]
        leaves = [torch.from_numpy(np.array(v, np.float64)).requires_grad_(True) for v in vals]
        layer = WorkspaceQP(qp)
        x, y = layer(*leaves)
        assert layer.status == 1 and qp.stats()["linsolve"] == 3 and qp.stats()["coupled_rows"] == r
        ((wt * x).sum() + (zt * torch.nan_to_num(y)).sum()).backward()
        direct = qp.adjoint(w, z, matrices=True)
        assert direct["status"][0] == 0 and layer.adjoint_status.tolist() == direct["status"].tolist()
        for v, k in zip(leaves, ("dq", "dl", "du", "dQ_values", "dA_values")):
            assert same_bits(v.grad.numpy(), direct[k]), k
        sol = dict(x=x.detach().numpy(), y=y.detach().numpy())
        o = {k: (None if v is None else v[None]) for k, v in direct.items() if k != "active"}
        o["active"] = direct["active"]
        check_rhs(W, p, sol, o, 0, w, z, True, "WorkspaceQP backward, coupled")
        flags = direct["active"]
        assert (flags[p["m"] - r:] != 0).any()
        dqw = qp.adjoint(w, None)
        assert dqw["status"][0] == 0 and np.array_equal(dqw["active"], flags)
        # (h: with the active set fixed the solution map is linear in q, so the step carries no truncation term, and the solves' share of
        # the bound falls as 1 / h.  Measured on the CPU oracle at eps_abs 1e-9, j = 3: h = 1e-4 gives a bound of 6 % of |dq_j| -- the
        # vacuity check below would refuse it --, h = 1e-2 leaves the active set as it is, difference 9.2e-11, bound 1.6e-4, |dq_j| 0.26.)
        h, j = 1e-2, 3
        Ad = ref.dense(p["A"])
        rvx, rvy, M, S = ref.adjoint(ref.full_Q(p["Q"], p["Qstype"]), Ad, flags, w.astype(ref.LD), None)
        minv = float(np.abs(np.linalg.inv(M.astype(np.float64))).sum(axis=1).max())
        anorm = float(np.abs(Ad.astype(np.float64)).sum(axis=0).max())
        v1x, v1y = float(np.abs(rvx).sum()), float(np.abs(rvy).sum())
        L, dL = [], 0.0
        for sgn in (1.0, -1.0):
            qj = p["q"].copy(); qj[j] += sgn * h
            plain = WorkspaceQP(qp)
            xs, ys = plain(torch.from_numpy(qj))
            assert plain.status == 1
            assert np.array_equal(ref.classify(xs.numpy(), ys.numpy(), Ad, p["l"], p["u"]), flags), "the step h moved the active set"
            info = qp.info()
            dL += v1x * (info["res_dual_norm"] + anorm * info["res_prim_norm"]) + v1y * info["res_prim_norm"]
            L.append(float(w @ xs.numpy()))
        fd = (L[0] - L[1]) / (2 * h)
        bound = dL / (2 * h) + 2.0 * minv * TA.TOL * np.abs(w).max()
        diff = abs(fd - dqw["dq"][j])
        print("finite differences of dL/dq[%d]: adjoint %.12e, central difference %.12e, |difference| %.3e, bound %.3e" % (j, dqw["dq"][j], fd, diff, bound))
        assert bound <= 1e-2 * abs(float(rvx[j])), ("the check would be vacuous", bound, float(rvx[j]))
        assert diff <= bound, (fd, dqw["dq"][j], bound)
    finally:
        qp.delete()


# ---- 7. refusals that remain ----------------------------------------------------------------------------------------------------------------------
def test_pcg_is_still_refused(monkeypatch):
    p = TA.problem("n40")
    monkeypatch.delenv("QPDO_BAND_ORDER", raising=False)
    qp = TG.workspace(monkeypatch, p, "pcg", 10)
    try:
        assert qp.solve()["info"]["status_val"] == 1 and qp.stats()["linsolve"] == 0 and qp.rhs_group() == 0
        for part in ("the workspace's solver is PCG", "QPDO_LINSOLVE=dense"):
            rc, msg, o = raw_adjoint(qp, np.ones(p["n"]))
            assert rc != 0 and part in msg and TA.untouched(o), (part, rc, msg)
            rc, msg, o = raw_tangent(qp, dict(tq=np.ones(p["n"])))
            assert rc != 0 and part in msg and TT.untouched(o), (part, rc, msg)
    finally:
        qp.delete()
