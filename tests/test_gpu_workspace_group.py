"""Groups of right-hand sides in the workspace adjoint and tangent (include/qpdo_amd_ext.h "GROUPS of right-hand sides") on the
MI355X, in this process, on the problems, workspaces and acceptance rules of tests/test_gpu_workspace_adjoint.py and
tests/test_gpu_workspace_tangent.py (imported from there).  Everything here is BITWISE: the multi-vector product against the single
product, a call with R right-hand sides against the R single calls (which run the G = 1 code path), the default workspace against one set
up with QPDO_AMD_RHS_GROUP=1, solver.QPDO.jacobian against the single tangent / adjoint calls; plus the counters of QPDOAmdGroupStats, which
say that the groups were in fact taken."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_workspace_adjoint as TA
import test_gpu_workspace_tangent as TT
from qpdo_amd import solver
from test_gpu_workspace_adjoint import ENV_KEYS, W, bits, problem, raw_adjoint, same_bits, snapshot  # noqa: F401
from test_gpu_workspace_tangent import O_KEYS, perturbation, pick, raw_tangent

pytestmark = pytest.mark.gpu

A_KEYS = ("dq", "dl", "du", "dQ_values", "dA_values", "residual")
FILL = -4321.5


def workspace(monkeypatch, p, linsolve, scaling, env=None, **kw):
    for k in ENV_KEYS + ("QPDO_AMD_RHS_GROUP", "QPDO_SPMV"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env or {}, **({"QPDO_LINSOLVE": linsolve} if linsolve else {})).items():
        monkeypatch.setenv(k, v)
    return solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=p["Qstype"], c=p.get("c", 0.0), scaling=scaling, verbose=0,
                               max_iter=kw.pop("max_iter", 1000), **kw)


def no_rows_problem():
    rng = np.random.default_rng(2)
    n = 40
    B = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.2)
    Q = sp.csc_matrix(np.tril(B @ B.T + n * np.eye(n))); Q.sort_indices()
    return dict(n=n, m=0, Q=Q, Qstype=-1, A=sp.csc_matrix((0, n)), q=rng.standard_normal(n), l=np.zeros(0), u=np.zeros(0), c=0.0)


def rounds_of(status, G):
    """read-backs of the sweep loop for these right-hand sides in groups of G: per group 1 + the largest sweep count"""
    sw = status[:, 1].tolist()
    return sum(1 + max(sw[i:i + G]) for i in range(0, len(sw), G))


def same_outputs(a, b, keys, what):
    for k in keys:
        if a[k] is not None:
            assert same_bits(a[k], b[k]), (what, k)
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["active"], b["active"]), (what, a["status"].tolist(), b["status"].tolist())


def slab_is_single(many, r, one, keys, what):
    for k in keys:
        if many[k] is not None:
            assert same_bits(many[k][r], one[k][0]), (what, r, k)
    assert many["status"][r].tolist() == one["status"][0].tolist() and np.array_equal(many["active"], one["active"]), (what, r, many["status"][r].tolist(), one["status"][0].tolist())


# ---- 1. the product alone -------------------------------------------------------------------------------------------------------------------------
def rows_problem(m, n, lengths, seed):
    """Q = I, loose bounds, row i of A with lengths[i] entries in random columns"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i, k in enumerate(lengths):
        c = np.sort(rng.choice(n, size=k, replace=False))
        rows += [i] * k; cols += c.tolist(); vals += rng.standard_normal(k).tolist()
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n)); A.sort_indices()
    Q = sp.identity(n, format="csc")
    return dict(n=n, m=m, Q=Q, Qstype=-1, A=A, q=rng.standard_normal(n), l=np.full(m, -1e3), u=np.full(m, 1e3), c=0.0)


@pytest.mark.parametrize("shape", ["a", "b"])
def test_the_product_alone(monkeypatch, shape):
    """qpdo_amd_spmv_group against qpdo_amd_spmv, bitwise, for A, A' and Q.  (a) m = 41, n = 48, row i of A with i entries: the average of 20
    gives 16 lanes per row, and the lengths cover the empty row, under 16, 16, 17, 32, 33 and the loop-plus-tail rows.  (b) m = 20, n = 150,
    rows of 130 .. 149 entries: 64 lanes per row, rows longer than 128.  The vectors outside the mask hold NaN: they are never gathered,
    and their slabs of y keep the fill."""
    p = rows_problem(41, 48, list(range(41)), 7) if shape == "a" else rows_problem(20, 150, list(range(130, 150)), 8)
    qp = workspace(monkeypatch, p, "dense", 0)
    try:
        rng = np.random.default_rng(11)
        for which in (0, 1, 2):
            ncols = p["n"] if which != 1 else p["m"]
            for nvec in (1, 3, 8):
                v = rng.standard_normal((nvec, ncols))
                single = np.stack([qp.spmv(which, v[g]) for g in range(nvec)])
                masks = {(1 << nvec) - 1, 1 << (nvec - 1)} | ({0b101} if nvec >= 3 else set())
                for mask in sorted(masks):
                    vv = v.copy()
                    vv[[g for g in range(nvec) if not (mask >> g) & 1]] = np.nan
                    y = qp.spmv_group(which, vv, mask, fill=FILL)
                    for g in range(nvec):
                        if (mask >> g) & 1:
                            assert same_bits(y[g], single[g]), (shape, which, nvec, bin(mask), g)
                        else:
                            assert (y[g] == FILL).all(), (shape, which, nvec, bin(mask), g, "a slab outside the mask was written")
            assert np.abs(single).max() > 0
    finally:
        qp.delete()


# ---- 2. groups against singles --------------------------------------------------------------------------------------------------------------------
CASES = {"n130[10]": ("n130", "dense", 10), "n130[0]": ("n130", "dense", 0), "n40": ("n40", "dense", 10), "band72": ("band72", "band", 10),
         "no rows": (None, "dense", 10)}


@pytest.mark.parametrize("case", list(CASES))
def test_groups_against_singles(monkeypatch, case):
    """R = 2, 8 and 11 right-hand sides (one partial group, one full group, a full and a partial one) of both calls: every slab carries the
    bits of the nrhs = 1 call with that slab -- outputs, status, res, active --, the same call twice gives the same bits, and the counters
    say that ceil(R / 8) groups ran with one read-back per sweep each"""
    name, linsolve, scaling = CASES[case]
    p = problem(name) if name else no_rows_problem()
    n, m = p["n"], p["m"]
    matrices = name == "n130"
    qp = workspace(monkeypatch, p, linsolve, scaling)
    try:
        assert qp.solve()["info"]["status_val"] == 1
        assert qp.rhs_group() == 8 and qp.group_stats()["group"] == 8 and qp.group_stats()["scratch_bytes"] == 0
        rng = np.random.default_rng(77)
        RMAX = 11
        gx, gy = rng.standard_normal((RMAX, n)), rng.standard_normal((RMAX, m))
        t = perturbation(p, rng, RMAX)
        if m == 0:
            t = dict(tq=t["tq"], tQ_values=t["tQ_values"])
        a_one, t_one = [], []
        for r in range(RMAX):
            rc, msg, o = raw_adjoint(qp, gx[r], gy[r], matrices=matrices)
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
                        return raw_adjoint(qp, gx[:R], gy[:R], matrices=matrices)
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
        assert qp.adjoint_stats()["scratch_bytes"] + qp.tangent_stats()["scratch_bytes"] > 0
        sb = qp.group_stats()["scratch_bytes"]
        assert sb >= 8 * 5 * (n + m) * 8 and sb == s1["scratch_bytes"], "G copies of the 5 n + 5 m work vectors, allocated once"
    finally:
        qp.delete()


# ---- 3. mixed sweep counts in one group --------------------------------------------------------------------------------------------------------
def test_mixed_sweep_counts_in_one_group(W, monkeypatch):
    """R = 8 on n130 with max_sweeps = 4: right-hand side 1 is all zero (accepted at sweep 0 with zeros), right-hand side 5 carries a NaN in
    an entry that is used (code 1, NaN slices, sweeps = max_sweeps); the other six are bitwise their single calls with code 0"""
    p = problem("n130")
    n, m = p["n"], p["m"]
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        assert qp.solve()["info"]["status_val"] == 1
        rng = np.random.default_rng(31)
        gx, gy = rng.standard_normal((8, n)), rng.standard_normal((8, m))
        gx[1] = 0.0; gy[1] = 0.0
        gx[5, 3] = np.nan
        rc, msg, many = raw_adjoint(qp, gx, gy, matrices=True, max_sweeps=4)
        assert rc == 0, msg
        print("adjoint status", many["status"].tolist())
        assert many["status"][:, 0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0], many["status"].tolist()
        assert many["status"][1, 1] == 0 and many["status"][5, 1] == 4
        assert not many["dq"][1].any() and not many["dl"][1].any() and not many["du"][1].any()
        assert all(np.isnan(many[k][5]).all() for k in A_KEYS)
        for r in range(8):
            rc, msg, one = raw_adjoint(qp, gx[r], gy[r], matrices=True, max_sweeps=4)
            assert rc == 0, msg
            if r == 5:
                assert one["status"][0].tolist() == many["status"][5].tolist()
            else:
                slab_is_single(many, r, one, A_KEYS, "adjoint, mixed group")
        t = perturbation(p, rng, 8)
        for k in t:
            t[k][1] = 0.0
        t["tq"][5, 3] = np.nan
        rc, msg, many = raw_tangent(qp, t, max_sweeps=4)
        assert rc == 0, msg
        print("tangent status", many["status"].tolist())
        assert many["status"][:, 0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and many["status"][1, 1] == 0 and many["status"][5, 1] == 4, many["status"].tolist()
        assert not many["dx"][1].any() and not many["dy"][1].any() and all(np.isnan(many[k][5]).all() for k in O_KEYS)
        for r in range(8):
            rc, msg, one = raw_tangent(qp, pick(t, r), max_sweeps=4)
            assert rc == 0, msg
            if r != 5:
                slab_is_single(many, r, one, O_KEYS, "tangent, mixed group")
    finally:
        qp.delete()


def test_not_accepted_in_a_group(W, monkeypatch):
    """the duplicated-rows problem of the adjoint's test_not_accepted: R = 4 with one gy outside the range and three inside -- codes (1, 0, 0,
    0) in the order given, the accepted ones bitwise their single calls: a right-hand side that runs to max_sweeps touches no other"""
    p = W.dup_item()
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        gx = np.random.default_rng(3).standard_normal(p["n"])
        bad = np.zeros(p["m"])
        bad[0], bad[1] = 1.0, -1.0
        gx4 = np.stack([gx, gx, 2.0 * gx, -0.5 * gx])
        gy4 = np.stack([bad, np.zeros(p["m"]), np.zeros(p["m"]), np.zeros(p["m"])])
        s0 = qp.group_stats()
        rc, msg, mix = raw_adjoint(qp, gx4, gy4, matrices=True)
        assert rc == 0 and mix["status"][:, 0].tolist() == [1, 0, 0, 0] and mix["status"][0, 1] == 20, (msg, mix["status"].tolist())
        s1 = qp.group_stats()
        assert s1["groups_run"] - s0["groups_run"] == 1 and s1["rounds_total"] - s0["rounds_total"] == 21
        for r in range(4):
            TA.check_rhs(W, p, sol, mix, r, gx4[r], gy4[r], True, "group with a code 1, right-hand side %d" % r, accept=((1,) if r == 0 else (0,)))
            rc, msg, one = raw_adjoint(qp, gx4[r], gy4[r], matrices=True)
            assert rc == 0, msg
            if r:
                slab_is_single(mix, r, one, A_KEYS, "beside a code 1")
            else:
                assert one["status"][0].tolist() == mix["status"][0].tolist()
    finally:
        qp.delete()


# ---- 4. the switch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_the_switch(monkeypatch, name, linsolve):
    """QPDO_AMD_RHS_GROUP=1 at setup: the right-hand sides follow one another (one "group" and 1 + sweeps read-backs each), and every
    output carries the default workspace's bits; =3: groups of three"""
    p = problem(name)
    D = workspace(monkeypatch, p, linsolve, 10)
    S = workspace(monkeypatch, p, linsolve, 10, env={"QPDO_AMD_RHS_GROUP": "1"})
    T3 = workspace(monkeypatch, p, linsolve, 10, env={"QPDO_AMD_RHS_GROUP": "3"})
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
            same_outputs(outs[0], outs[1], keys, (name, kind, "default against QPDO_AMD_RHS_GROUP=1"))
            same_outputs(outs[0], outs[2], keys, (name, kind, "default against QPDO_AMD_RHS_GROUP=3"))
        assert S.group_stats()["scratch_bytes"] == 0 and T3.group_stats()["scratch_bytes"] > 0
    finally:
        D.delete(); S.delete(); T3.delete()


# ---- 5. no trace --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,linsolve", [("n130", "dense"), ("band72", "band")])
def test_no_bit_moves(monkeypatch, name, linsolve):
    """two workspaces on one problem, R = 11 calls of both kinds on X only: every later solve of X carries Y's bits"""
    p = problem(name)
    X, Y = workspace(monkeypatch, p, linsolve, 10), workspace(monkeypatch, p, linsolve, 10)
    try:
        rng = np.random.default_rng(5)
        R = 11
        gx, gy = rng.standard_normal((R, p["n"])), rng.standard_normal((R, p["m"]))
        t = perturbation(p, rng, R)
        a, b = X.solve(), Y.solve()
        assert a["info"]["status_val"] == 1 and snapshot(X, a) == snapshot(Y, b)
        rc, msg, o = raw_adjoint(X, gx, gy, matrices=True)
        assert rc == 0 and (o["status"][:, 0] != 3).all(), (msg, o["status"].tolist())
        rc, msg, o = raw_tangent(X, t)
        assert rc == 0 and (o["status"][:, 0] != 3).all(), (msg, o["status"].tolist())
        assert snapshot(X, a)["stats"] == snapshot(Y, b)["stats"], "QPDOAmdStats after the group calls"
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "the solve after the group calls"
        rc, msg, o = raw_tangent(X, t)
        assert rc == 0, msg
        rc, msg, o = raw_adjoint(X, gx, gy)
        assert rc == 0, msg
        for S in (X, Y):
            S.update_q(1.5 * p["q"] + 0.1)
            S.warm_start(a["x"], a["y"])
        a, b = X.solve(), Y.solve()
        assert snapshot(X, a) == snapshot(Y, b), "update_q, warm_start, solve"
        assert X.group_stats()["groups_run"] == 8 and Y.group_stats()["groups_run"] == 0 and Y.group_stats()["scratch_bytes"] == 0
    finally:
        X.delete(); Y.delete()


# ---- 6. the group size per workspace kind ---------------------------------------------------------------------------------------------------
def test_rhs_group_per_workspace_kind(monkeypatch):
    p = problem("n130")
    qp = workspace(monkeypatch, p, "pcg", 10)
    try:
        assert qp.rhs_group() == 0 and qp.group_stats()["group"] == 0
    finally:
        qp.delete()
    qp = workspace(monkeypatch, p, "dense", 10, env={"QPDO_DENSE_SOLVE": "steps"})
    try:
        assert qp.solve()["info"]["status_val"] == 1
        assert qp.rhs_group() == 1
        rng = np.random.default_rng(9)
        gx, gy = rng.standard_normal((3, p["n"])), rng.standard_normal((3, p["m"]))
        t = perturbation(p, rng, 3)
        s0 = qp.group_stats()
        rc, msg, many = raw_adjoint(qp, gx, gy, matrices=True)
        assert rc == 0 and (many["status"][:, 0] == 0).all(), (msg, many["status"].tolist())
        rc, msg, tmany = raw_tangent(qp, t)
        assert rc == 0 and (tmany["status"][:, 0] == 0).all(), (msg, tmany["status"].tolist())
        s1 = qp.group_stats()
        assert s1["groups_run"] - s0["groups_run"] == 6 and s1["scratch_bytes"] == 0
        for r in range(3):
            rc, msg, one = raw_adjoint(qp, gx[r], gy[r], matrices=True)
            assert rc == 0, msg
            slab_is_single(many, r, one, A_KEYS, "stepwise solves, adjoint")
            rc, msg, one = raw_tangent(qp, pick(t, r))
            assert rc == 0, msg
            slab_is_single(tmany, r, one, O_KEYS, "stepwise solves, tangent")
    finally:
        qp.delete()


# ---- 7. jacobian ----------------------------------------------------------------------------------------------------------------------------------
def test_jacobian(W, monkeypatch):
    """n40, both modes with wrt = (q, l, u) and outputs = (x, y): every column of the tangent mode is the single tangent call of that unit
    perturbation and every row of the adjoint mode the single adjoint call of that unit gradient, bitwise; the columns of dx_dl / dx_du of
    rows that are not -1 / +1 are exact zeros; three sampled columns and rows pass the two calls' own acceptance rules"""
    p = problem("n40")
    n, m = p["n"], p["m"]
    qp = workspace(monkeypatch, p, "dense", 10)
    try:
        sol = qp.solve()
        assert sol["info"]["status_val"] == 1
        s0 = qp.group_stats()
        Jt = qp.jacobian(wrt=("q", "l", "u"), outputs=("x", "y"), mode="tangent")
        s1 = qp.group_stats()
        assert Jt["mode"] == "tangent" and Jt["status"].shape == (n + 2 * m, 3) and (Jt["status"][:, 0] == 0).all()
        assert s1["groups_run"] - s0["groups_run"] == (n + 2 * m + 7) // 8
        flags = Jt["active"]
        assert (flags == 1).any() and (flags == -1).any() and (flags == 0).any()
        for k, sz in (("q", n), ("l", m), ("u", m)):
            assert Jt["dx_d" + k].shape == (n, sz) and Jt["dy_d" + k].shape == (m, sz)
        sampled = {("q", 3), ("l", int(np.flatnonzero(flags == -1)[0])), ("u", int(np.flatnonzero(flags == 1)[0]))}
        for k, sz in (("q", n), ("l", m), ("u", m)):
            for j in range(sz):
                e = np.zeros(sz); e[j] = 1.0
                tt = {"t" + k: e}
                rc, msg, one = raw_tangent(qp, tt)
                assert rc == 0 and one["status"][0, 0] == 0, msg
                assert same_bits(Jt["dx_d" + k][:, j], one["dx"][0]) and same_bits(Jt["dy_d" + k][:, j], one["dy"][0]), (k, j)
                if (k, j) in sampled:
                    TT.check_rhs(p, sol, one, 0, tt, "jacobian column d/d%s[%d]" % (k, j))
        assert not Jt["dx_dl"][:, flags != -1].any() and not Jt["dx_du"][:, flags != 1].any()
        assert not Jt["dy_dl"][:, flags != -1].any() and not Jt["dy_du"][:, flags != 1].any()
        assert np.abs(Jt["dx_dl"][:, flags == -1]).max() > 0 and np.abs(Jt["dx_du"][:, flags == 1]).max() > 0

        Ja = qp.jacobian(wrt=("q", "l", "u"), outputs=("x", "y"), mode="adjoint")
        assert Ja["mode"] == "adjoint" and Ja["status"].shape == (n + m, 3) and (Ja["status"][:, 0] == 0).all() and np.array_equal(Ja["active"], flags)
        rows = {("x", 5), ("y", int(np.flatnonzero(flags == -1)[0])), ("y", int(np.flatnonzero(flags == 1)[0]))}
        for o_, sz in (("x", n), ("y", m)):
            for i in range(sz):
                gx, gy = np.zeros(n), (np.zeros(m) if o_ == "y" else None)
                (gx if o_ == "x" else gy)[i] = 1.0
                rc, msg, one = raw_adjoint(qp, gx, gy)
                assert rc == 0 and one["status"][0, 0] == 0, msg
                for k in ("q", "l", "u"):
                    assert same_bits(Ja["d%s_d%s" % (o_, k)][i], one["d" + k][0]), (o_, i, k)
                if (o_, i) in rows:
                    TA.check_rhs(W, p, sol, one, 0, gx, gy, False, "jacobian row d%s[%d]/d" % (o_, i))
        assert not Ja["dx_dl"][:, flags != -1].any() and not Ja["dx_du"][:, flags != 1].any()
        # auto: the mode with fewer right-hand sides, adjoint on a tie
        assert qp.jacobian(wrt=("q", "l", "u"), outputs=("x",))["mode"] == "adjoint"          # n < n + 2 m
        assert qp.jacobian(wrt=("q",), outputs=("x", "y"))["mode"] == "tangent"               # n < n + m
        Jq = qp.jacobian(wrt=("q",), outputs=("x",))
        assert Jq["mode"] == "adjoint" and set(Jq) == {"mode", "dx_dq", "active", "status"} and same_bits(Jq["dx_dq"], Ja["dx_dq"])
    finally:
        qp.delete()
