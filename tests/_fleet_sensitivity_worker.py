"""Child process of tests/test_gpu_fleet_sensitivity.py: the scenarios of the fleet's many-right-hand-side calls
(qpdo_amd_fleet_adjoint_multi_dev, qpdo_amd_fleet_tangent_dev; solver.Fleet.adjoint_many_device / tangent_device; FleetQP.tangent / vjp_many),
each run once, their outcomes written as JSON.  A process of its own because torch comes FIRST here (tests/_fleet_device_worker.py).  The
fleets are those of tests/_fleet_adjoint_worker.py.

Adjoint slabs are compared with the single call BIT FOR BIT.  The tangent is checked against tests/fleet_sensitivity_ref.py (numpy,
longdouble) with the DEVICE's flags: with d = (dx, dy_S) read back and r the longdouble right-hand side, the residual must be at most
    tol max(||rx||, ||ry_S||) + (n + k + 2) eps || |M| |d| ||_inf + (L + 2) eps ||T||_inf
(second term: the kernel's fp64 residual evaluation; third: its fp64 right-hand side, L the longest row of the formation and T the sum of
the absolute values of its terms per component), and where M's float64 condition number is below 1 / eps also
||d - d_ref|| <= 2 ||M^-1||_inf (that bound): the rule of _fleet_adjoint_worker.check_item.
usage: _fleet_sensitivity_worker.py OUT.json"""
import functools
import json
import os
import sys
import traceback

import numpy as np
import torch  # noqa: F401  (before qpdo_amd loads its library: one HIP runtime in the process)
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fleet_adjoint_ref as ref  # noqa: E402
import fleet_sensitivity_ref as sref  # noqa: E402
from qpdo_amd import problems, solver  # noqa: E402
from qpdo_amd.torch_layer import FleetQP  # noqa: E402
from _fleet_adjoint_worker import EPS, LAYOUT, SENTINEL, ST, TOL, dup_item, eq_item, fleet, gpu, host  # noqa: E402
from _fleet_device_worker import bit_equal, bits, compare_host, pack  # noqa: E402
from test_gpu_fleet_matrices import new_A, new_Q  # noqa: E402

NOTES = {}
ADJ_KEYS = ("dq", "dl", "du", "dQ_values", "dA_values")


def nrhs_values(G):
    """1, 2, G, G + 1, 2G + 3 (1, 2, 5 where G = 1)"""
    return sorted({1, 2, G, G + 1, 2 * G + 3})


def sizes(F, matrices=True):
    no, mo = F.packed_layout()
    qo, ao = F.packed_matrix_layout() if matrices else ([0], [0])
    return int(no[-1]), int(mo[-1]), int(qo[-1]), int(ao[-1])


def full(shape, dtype=torch.float64, value=SENTINEL):
    return torch.full(shape, value, dtype=dtype).cuda()


def adj_sentinel(F, R, matrices):
    """outputs pre-filled with a sentinel (an entry the kernel never wrote is seen); R None: the single call's shapes"""
    N, M, NQ, NA = sizes(F, matrices)
    sh = (lambda *s: s) if R is None else (lambda *s: (R,) + s)
    d = dict(dq=full(sh(N)), dl=full(sh(M)), du=full(sh(M)), active=full((M,), torch.int32, 77), status=full(sh(F.count, 3), torch.int64, -77),
             residual=full(sh(F.count)))
    if matrices:
        d.update(dQ_values=full(sh(NQ)), dA_values=full(sh(NA)))
    return d


def tan_sentinel(F, R):
    N, M, _, _ = sizes(F, False)
    sh = (lambda *s: s) if R is None else (lambda *s: (R,) + s)
    return dict(dx=full(sh(N)), dy=full(sh(M)), active=full((M,), torch.int32, 77), status=full(sh(F.count, 3), torch.int64, -77), residual=full(sh(F.count)))


def same_bits(a, b, what):
    """two arrays equal as bit patterns (integers compared as such)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        assert bit_equal(a, b), (what, "bits differ", int((bits(a) != bits(b)).sum()))
    else:
        assert np.array_equal(a, b), (what, "values differ")


def compare_slabs(F, many, singles, matrices, what):
    """every output slab r of adjoint_many_device against adjoint_device with slab r, sentinels included"""
    mo = F.packed_layout()[1]
    keys = ("dq", "dl", "du") + (("dQ_values", "dA_values") if matrices else ()) + ("status", "residual")
    for r, one in enumerate(singles):
        for k in keys:
            assert not (many[k][r] == (SENTINEL if many[k].dtype.kind == "f" else -77)).any(), (what, r, k, "an unwritten entry")
            same_bits(many[k][r], one[k], "%s rhs %d %s" % (what, r, k))
    # the flags are the solve's: an item's slice equals the single call's wherever that call delivered its flags (code 0), is zeros for codes 2, 3
    codes = np.array([one["status"][:, 0] for one in singles])
    for i in range(F.count):
        sl = slice(int(mo[i]), int(mo[i + 1]))
        got = many["active"][sl]
        assert not (got == 77).any(), (what, i, "flags unwritten")
        ok = np.flatnonzero(codes[:, i] == 0)
        if len(ok):
            assert np.array_equal(got, singles[ok[0]]["active"][sl]), (what, i, "flags")
        elif (codes[:, i] >= 2).all():
            assert not got.any(), (what, i, "flags of an item that is not solved")


# ---- 1. adjoint slabs carry the single call's bits ----------------------------------------------------------------------------------------
def adjoint_bits(name, scaling):
    probs = list(fleet(name))
    F = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=scaling, **ST)
    try:
        assert F.factor_layout() == LAYOUT[name]
        G = F.rhs_group()
        assert 1 <= G <= 8
        N, M, NQ, NA = sizes(F)
        sol = host(F.solve_device())
        assert (sol["status"][:, 0] == 1).sum() >= len(probs) - 2
        Rmax = 2 * G + 3
        rng = np.random.default_rng(500 + scaling)
        gx = rng.standard_normal((Rmax, N))
        flags = host(F.adjoint_device(gpu(gx[0])))["active"]
        gy = rng.standard_normal((Rmax, M))
        gy[:, flags == 0] = np.nan                           # (entries of inactive rows are ignored: NaN must reach nothing)
        calls = 0
        for with_gy in (False, True):
            for matrices in (False, True):
                singles = [host(F.adjoint_device(gpu(gx[r]), gpu(gy[r]) if with_gy else None, matrices=matrices, out=adj_sentinel(F, None, matrices), tol=TOL))
                           for r in range(Rmax)]
                for R in nrhs_values(G):
                    many = host(F.adjoint_many_device(gpu(gx[:R]), gpu(gy[:R]) if with_gy else None, matrices=matrices, out=adj_sentinel(F, R, matrices), tol=TOL))
                    compare_slabs(F, many, singles[:R], matrices, "%s[%d] gy=%s matrices=%s R=%d" % (name, scaling, with_gy, matrices, R))
                    calls += 1
                if not with_gy:
                    assert all((o["status"][sol["status"][:, 0] == 1, 0] == 0).all() for o in singles), "gy=None: every solved item is accepted"
        st = F.sensitivity_stats()
        assert st["calls"] == calls and st["rhs_total"] == 4 * sum(nrhs_values(G)) and F.adjoint_stats()["resident_extra_bytes"] == 0, st
        # the slots of the right-hand sides carried at once: allocated once, G x (7 n-vectors + 5 m-vectors); none where they follow one another
        assert st["scratch_bytes"] == (8 * G * (7 * N + 5 * M) if G > 1 else 0) and G == (8 if name == "P" else 1), (G, st)
        NOTES["rhs_group %s[%d]" % (name, scaling)] = G
        NOTES["scratch_bytes %s[%d]" % (name, scaling)] = st["scratch_bytes"]
    finally:
        F.close()


# ---- 2. a refused right-hand side stays alone ----------------------------------------------------------------------------------------------
def refused_alone():
    probs = [problems.random_qp(23, 40, 60, 0.2, 10), dup_item(), eq_item()]
    F = solver.Fleet(probs, adjoint=True, scaling=10, **ST)
    try:
        no, mo = F.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        sol = host(F.solve_device())
        assert sol["status"][:, 0].tolist() == [1, 1, 1]
        R = 2 * F.rhs_group() + 3
        rng = np.random.default_rng(3)
        gx = rng.standard_normal((R, N))
        gy = np.zeros((R, M))
        gy[1::2, int(mo[1])], gy[1::2, int(mo[1]) + 1] = 1.0, -1.0      # odd r: the two identical (equality) rows of item 1 disagree
        singles = [host(F.adjoint_device(gpu(gx[r]), gpu(gy[r]), out=adj_sentinel(F, None, False), tol=TOL)) for r in range(R)]
        many = host(F.adjoint_many_device(gpu(gx), gpu(gy), out=adj_sentinel(F, R, False), tol=TOL))
        compare_slabs(F, many, singles, False, "refused_alone")
        n0, n1, m0, m1 = int(no[1]), int(no[2]), int(mo[1]), int(mo[2])
        for r in range(R):
            assert many["status"][r, :, 0].tolist() == [0, r % 2, 0], (r, many["status"][r].tolist())
            sl = [many["dq"][r, n0:n1], many["dl"][r, m0:m1], many["du"][r, m0:m1]]
            if r % 2:
                assert all(np.isnan(s).all() for s in sl) and np.isnan(many["residual"][r, 1]) and many["status"][r, 1, 1] == 20, r
            else:
                assert not any(np.isnan(s).any() for s in sl) and many["residual"][r, 1] <= TOL, r
        assert many["active"][m0:m1].any(), "the item's flags are delivered whatever its right-hand sides' codes"
    finally:
        F.close()


# ---- 3. / 4. the tangent against the longdouble reference; duality --------------------------------------------------------------------------
def perturbation(F, probs, rng, R):
    """tq, tl, tu, tQ, tA of R right-hand sides in the packed layouts; tQ symmetric as a matrix (needed where an item's Q is stored in full)"""
    N, M, NQ, NA = sizes(F)
    qo, _ = F.packed_matrix_layout()
    tQ = np.zeros((R, NQ))
    for i, p in enumerate(probs):
        Q = sp.csc_matrix(p["Q"]); Q.sort_indices()
        rows, cols = Q.indices, np.repeat(np.arange(p["n"]), np.diff(Q.indptr))
        for r in range(R):
            B = rng.standard_normal((p["n"], p["n"]))
            tQ[r, int(qo[i]):int(qo[i + 1])] = (B + B.T)[rows, cols]
    return dict(tq=rng.standard_normal((R, N)), tl=rng.standard_normal((R, M)), tu=rng.standard_normal((R, M)), tQ_values=tQ, tA_values=rng.standard_normal((R, NA)))


def item_slices(F, i):
    (no, mo), (qo, ao) = F.packed_layout(), F.packed_matrix_layout()
    return tuple(slice(int(o[i]), int(o[i + 1])) for o in (no, mo, qo, ao))


def tangent_rhs_of(F, p, i, r, sol, flags, t):
    sn, sm, sq, sa = item_slices(F, i)
    pick = lambda k, s: None if t.get(k) is None else t[k][r][s]
    return sref.tangent_rhs(p["Q"], p["Qstype"], p["A"], flags[sm], sol["x"][sn], sol["y"][sm], pick("tq", sn), pick("tl", sm), pick("tu", sm),
                            pick("tQ_values", sq), pick("tA_values", sa))


def check_tangent(F, probs, sol, o, t, R, what, expect_all_accepted):
    """every per-item check of one tangent call with R right-hand sides; returns the number of error-bound checks that ran"""
    flags = o["active"]
    ran = 0
    for i, p in enumerate(probs):
        sn, sm, _, _ = item_slices(F, i)
        n, m = p["n"], p["m"]
        Qf, A = ref.full_Q(p["Q"], p["Qstype"]), (ref.dense(p["A"]) if m else np.zeros((0, n)))
        for r in range(R):
            code, sweeps, k = o["status"][r, i].tolist()
            w = "%s item %d rhs %d" % (what, i, r)
            dx, dy = o["dx"][r][sn], o["dy"][r][sm]
            if sol["status"][i][0] != 1:
                assert code == 2, (w, code)
            else:
                assert code in ((0,) if expect_all_accepted else (0, 1)), (w, code, sweeps)
            if code != 0:
                assert np.isnan(dx).all() and np.isnan(dy).all() and np.isnan(o["residual"][r, i]), (w, "NaN slices")
                continue
            assert np.isfinite(dx).all() and np.isfinite(dy).all() and (dx != SENTINEL).all() and (dy != SENTINEL).all(), (w, "NaN or an unwritten entry")
            f = flags[sm]
            assert k == int((f != 0).sum()) and o["residual"][r, i] <= TOL and 0 <= sweeps <= 20, w
            assert not bits(dy)[f == 0].any(), (w, "dy off S is a bitwise +0.0")
            rh = tangent_rhs_of(F, p, i, r, sol, flags, t)
            M, S = ref.kkt(Qf, A, f)
            d = np.concatenate([dx.astype(ref.LD), dy.astype(ref.LD)[S]])
            rhs = np.concatenate([rh["rx"], rh["ry"]])
            gn = float(np.abs(rhs).max()) if len(rhs) else 0.0
            res = float(np.abs(M @ d - rhs).max())
            bound = TOL * gn + (n + k + 2) * EPS * float((np.abs(M) @ np.abs(d)).max()) + (rh["L"] + 2) * EPS * float(rh["T"].max())
            assert res <= bound, (w, "residual", res, bound)
            M64 = M.astype(np.float64)
            cond = np.linalg.cond(M64) if M64.size else 1.0
            if np.isfinite(cond) and cond < 1.0 / EPS:
                minv = float(np.abs(np.linalg.inv(M64)).sum(axis=1).max())
                dref, _ = ref.solve_ref(M, rhs)
                err = float(np.abs(d - dref).max())
                assert err <= 2.0 * minv * bound, (w, "error", err, 2.0 * minv * bound)
                ran += 1
    return ran


def tangent_fleet(name, scaling):
    probs = list(fleet(name))
    F = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=scaling, **ST)
    try:
        assert F.factor_layout() == LAYOUT[name]
        G = F.rhs_group()
        sol = host(F.solve_device())
        solved = int((sol["status"][:, 0] == 1).sum())
        rng = np.random.default_rng(700 + scaling)
        R = 2 * G + 3
        t = perturbation(F, probs, rng, R)
        # q alone (one vector, no leading R): ry = 0 is consistent whatever the active rows -- every solved item is accepted
        o1 = host(F.tangent_device(tq=gpu(t["tq"][0]), out=tan_sentinel(F, None), tol=TOL))
        o1 = {k: (v if k == "active" else v[None]) for k, v in o1.items()}
        ran = check_tangent(F, probs, sol, o1, dict(tq=t["tq"][:1]), 1, "%s[%d] tq" % (name, scaling), True)
        # q and Q (ry still 0: every solved item accepted, the item whose Q is stored in full among them)
        tqQ = dict(tq=t["tq"][:2], tQ_values=t["tQ_values"][:2])
        o2 = host(F.tangent_device(**{k: gpu(v) for k, v in tqQ.items()}, out=tan_sentinel(F, 2), tol=TOL))
        ran += check_tangent(F, probs, sol, o2, tqQ, 2, "%s[%d] tq, tQ" % (name, scaling), True)
        # all five, every value of nrhs (dependent active rows may make ry inconsistent: code 1)
        for Rr in nrhs_values(G):
            o = host(F.tangent_device(**{k: gpu(v[:Rr]) for k, v in t.items()}, out=tan_sentinel(F, Rr), tol=TOL))
            if Rr == R:
                ran += check_tangent(F, probs, sol, o, t, R, "%s[%d] all" % (name, scaling), False)
                oR = o
            else:
                keep = o
                for k in ("dx", "dy", "status", "residual"):
                    assert not (keep[k] == (SENTINEL if keep[k].dtype.kind == "f" else -77)).any(), (k, Rr, "an unwritten entry")
        for k in ("dx", "dy", "status", "residual"):        # a right-hand side's result does not depend on how many travel with it
            same_bits(keep[k], oR[k][:keep[k].shape[0]], "nrhs %d against %d, %s" % (keep[k].shape[0], R, k))
        codes = oR["status"][:, :, 0]
        assert ((codes == 0).sum(axis=1) >= solved - 1).all(), codes.tolist()
        # NaN planted on rows that do not use them changes no bit
        flags = oR["active"]
        (_, mo), (_, ao) = F.packed_layout(), F.packed_matrix_layout()
        tn = {k: v.copy() for k, v in t.items()}
        tn["tl"][:, flags != -1] = np.nan
        tn["tu"][:, flags != 1] = np.nan
        for i, p in enumerate(probs):
            A = sp.csc_matrix(p["A"]); A.sort_indices()
            unused = flags[int(mo[i]):int(mo[i + 1])][A.indices] == 0
            tn["tA_values"][:, int(ao[i]) + np.flatnonzero(unused)] = np.nan
        on = host(F.tangent_device(**{k: gpu(v) for k, v in tn.items()}, out=tan_sentinel(F, R), tol=TOL))
        for k in ("dx", "dy", "active", "status", "residual"):
            same_bits(on[k], oR[k], "NaN on unused rows, " + k)
        # NaN on a row that IS used is never accepted
        used = np.flatnonzero(flags == 1)
        if len(used):
            tb = {k: v.copy() for k, v in t.items()}
            tb["tu"][0, used[0]] = np.nan
            ob = host(F.tangent_device(**{k: gpu(v) for k, v in tb.items()}, tol=TOL))
            item = int(np.searchsorted(mo, used[0], side="right") - 1)
            assert ob["status"][0, item, 0] == 1 and np.isnan(ob["dx"][0][item_slices(F, item)[0]]).all(), ob["status"][0].tolist()
        # a zero right-hand side is accepted at sweep 0 with zeros
        oz = host(F.tangent_device(tq=gpu(np.zeros_like(t["tq"][0])), out=tan_sentinel(F, None), tol=TOL))
        ok = sol["status"][:, 0] == 1
        assert (oz["status"][ok, 0] == 0).all() and (oz["status"][ok, 1] == 0).all(), oz["status"].tolist()
        assert ran >= 1, "the error-bound branch ran for no accepted item of fleet %s" % name
        NOTES["error-bound checks %s[%d]" % (name, scaling)] = ran
        NOTES["tangent codes %s[%d]" % (name, scaling)] = codes.reshape(-1).tolist()
    finally:
        F.close()


def duality(name):
    probs = list(fleet(name))
    F = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)
    try:
        G = F.rhs_group()
        sol = host(F.solve_device())
        rng = np.random.default_rng(900)
        R = 2 * G + 3
        N, M, _, _ = sizes(F)
        t = perturbation(F, probs, rng, R)
        gx, gy = rng.standard_normal((R, N)), rng.standard_normal((R, M))
        a = host(F.adjoint_many_device(gpu(gx), gpu(gy), matrices=True, tol=TOL))
        d = host(F.tangent_device(**{k: gpu(v) for k, v in t.items()}, tol=TOL))
        flags = a["active"]
        pairs, worst = 0, 0.0
        for i, p in enumerate(probs):
            sn, sm, _, _ = item_slices(F, i)
            n, m = p["n"], p["m"]
            Qf, A = ref.full_Q(p["Q"], p["Qstype"]), (ref.dense(p["A"]) if m else np.zeros((0, n)))
            for r in range(R):
                if a["status"][r, i, 0] != 0 or d["status"][r, i, 0] != 0:
                    continue
                Mk, S = ref.kkt(Qf, A, flags[sm])
                k = len(S)
                v = np.concatenate([-a["dq"][r][sn].astype(ref.LD), (a["dl"][r][sm] + a["du"][r][sm]).astype(ref.LD)[S]])
                dd = np.concatenate([d["dx"][r][sn].astype(ref.LD), d["dy"][r][sm].astype(ref.LD)[S]])
                g = np.concatenate([gx[r][sn].astype(ref.LD), gy[r][sm].astype(ref.LD)[S]])
                rh = tangent_rhs_of(F, p, i, r, sol, flags, t)
                rr = np.concatenate([rh["rx"], rh["ry"]])
                e_a, e_t = np.abs(Mk @ v - g).max(), np.abs(Mk @ dd - rr).max()
                lhs, rhs_, mag = sref.duality_sides(g, dd, v, rr)
                bound = np.abs(v).sum() * e_t + np.abs(dd).sum() * e_a + (n + k + 2) * EPS * mag
                assert abs(lhs - rhs_) <= bound, ("duality", name, i, r, float(abs(lhs - rhs_)), float(bound))
                worst = max(worst, float(abs(lhs - rhs_) / max(float(mag), 1e-300)))
                pairs += 1
        assert pairs >= R, ("accepted pairs", pairs)
        NOTES["duality pairs %s" % name] = pairs
        NOTES["duality worst relative gap %s" % name] = "%.3e" % worst
    finally:
        F.close()


# ---- 5. no bit of any solve moves -----------------------------------------------------------------------------------------------------------
def no_bit_moves(name):
    probs = list(fleet(name))
    X = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)       # a tangent and a multi-adjoint call after every solve
    Y = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)       # the flag, never asked
    Z = solver.Fleet(probs, matrix_updates=True, scaling=10, **ST)                      # no flag
    try:
        assert X.factor_layout() == Y.factor_layout() == Z.factor_layout() == LAYOUT[name]
        R = X.rhs_group() + 1
        N, M, _, _ = sizes(X)
        rng = np.random.default_rng(5)
        gx, gy = gpu(rng.standard_normal((R, N))), gpu(rng.standard_normal((R, M)))
        t = {k: gpu(v) for k, v in perturbation(X, probs, rng, R).items()}

        def solve(what):
            outs = [host(F.solve_device()) for F in (X, Y, Z)]
            for k in outs[0]:
                assert bit_equal(outs[0][k], outs[1][k]) and bit_equal(outs[0][k], outs[2][k]), (what, k)
            a = host(X.adjoint_many_device(gx, gy, matrices=True))
            d = host(X.tangent_device(**t))
            solved = outs[0]["status"][:, 0] == 1
            assert ((a["status"][:, :, 0] == 2) == ~solved).all() and ((d["status"][:, :, 0] == 2) == ~solved).all(), (what, a["status"].tolist(), d["status"].tolist())
            compare_host(X.fetch_last(), Y.fetch_last(), "fetch_last after the sensitivity calls, " + what)
            again = host(X._dev_out)
            for k in outs[0]:
                assert bit_equal(outs[0][k], again[k]), (what, k, "the solve's outputs after the sensitivity calls")

        solve("cold")
        q, l, u = [1.5 * p["q"] + 0.1 for p in probs], [p["l"] - 0.1 for p in probs], [p["u"] + 0.05 for p in probs]
        for F in (X, Y, Z):
            F.update_device(pack(q), pack(l), pack(u)); F.warm_start_last_device()
        solve("update, warm_start_last")
        Qn, An = [new_Q(p, 300 + 10 * i) for i, p in enumerate(probs)], [new_A(p, 301 + 10 * i) for i, p in enumerate(probs)]
        qv, av, mask = X.pack_matrix_values(Q=Qn, A=An)
        for F in (X, Y, Z):
            F.update_matrices_device(gpu(qv), gpu(av), mask=gpu(mask))
        solve("update_matrices")
        sx = X.sensitivity_stats()
        assert (sx["calls"], sx["rhs_total"]) == (6, 6 * R) and Y.sensitivity_stats()["calls"] == 0, sx
        assert X.adjoint_stats() == Y.adjoint_stats() == dict(adjoint_calls=0, resident_extra_bytes=0)
        a, b = X.stats(), Y.stats()
        assert (a["solve_launches"], a["solves"]) == (b["solve_launches"], b["solves"]) == (3, 3)
        assert X.matrix_stats()["resident_extra_bytes"] == Z.matrix_stats()["resident_extra_bytes"]
    finally:
        X.close(); Y.close(); Z.close()


# ---- 6. refusals launch nothing -------------------------------------------------------------------------------------------------------------
def refusals_launch_nothing():
    import ctypes as C
    probs = [problems.random_qp(23, 40, 60, 0.2, 10), eq_item()]
    F = solver.Fleet(probs, adjoint=True, scaling=10, **ST)
    H = solver.Fleet(probs, matrix_updates=True, scaling=10, **ST)
    try:
        no, mo = F.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        gx, tq = gpu(np.ones((2, N))), gpu(np.ones(N))

        def counters(K):
            dev = K.sync()
            return (dev, K.stats(), K.adjoint_stats(), K.sensitivity_stats(), K.matrix_stats() if K is H else None)

        def refused(K, call, msg):
            before = counters(K)
            try:
                call()
            except (RuntimeError, ValueError) as e:
                assert msg in str(e), (msg, str(e))
            else:
                raise AssertionError("not refused: " + msg)
            assert counters(K) == before, msg

        refused(F, lambda: F.adjoint_many_device(gx), "was not a solve")                                # before any solve
        refused(F, lambda: F.tangent_device(tq=tq), "was not a solve")
        F.solve_device()
        assert host(F.adjoint_many_device(gx))["status"][:, :, 0].tolist() == [[0, 0], [0, 0]]
        assert host(F.tangent_device(tq=tq))["status"][:, 0].tolist() == [0, 0]
        assert F.sensitivity_stats() == dict(calls=2, rhs_total=3, scratch_bytes=F.sensitivity_stats()["scratch_bytes"])
        F.update_device(q=pack([p["q"] for p in probs]))
        refused(F, lambda: F.adjoint_many_device(gx), "was not a solve")                                # after an update
        refused(F, lambda: F.tangent_device(tq=tq), "was not a solve")
        F.warm_start_last_device(); F.solve_device()
        H.solve_device()
        refused(H, lambda: H.adjoint_many_device(gx), "without QPDO_AMD_FLEET_ADJOINT")                 # a fleet without the flag
        refused(H, lambda: H.tangent_device(tq=tq), "without QPDO_AMD_FLEET_ADJOINT")
        refused(F, lambda: F.adjoint_many_device(gx, matrices=True), "QPDO_AMD_FLEET_MATRIX_UPDATES")   # matrices without the matrix flag
        refused(F, lambda: F.tangent_device(), "no tangent passed")
        refused(F, lambda: F.tangent_device(tq=gpu(np.ones((2, N))), tl=gpu(np.ones((3, M)))), "do not agree on R")
        L = solver.lib()
        out = F.adjoint_many_device(gx)
        tout = F.tangent_device(tq=tq)
        torch.cuda.synchronize()
        a = [out[k].data_ptr() for k in ("dq", "dl", "du")]
        tail = [None, None, out["active"].data_ptr(), out["status"].data_ptr(), out["residual"].data_ptr()]
        d = [tout[k].data_ptr() for k in ("dx", "dy")]
        ttail = [tout["active"].data_ptr(), tout["status"].data_ptr(), tout["residual"].data_ptr()]
        before = F.sensitivity_stats()["calls"]

        def raw(gxp, n_len, m_len, nrhs=2, tol=1e-9, sweeps=20, dqp=a[0]):
            rc = L.qpdo_amd_fleet_adjoint_multi_dev(F._h, nrhs, gxp, None, dqp, a[1], a[2], *tail, tol, sweeps, n_len, m_len, 0, 0, None)
            if rc:
                raise RuntimeError((L.qpdo_amd_last_error() or b"").decode())

        def rawt(tqp, n_len, m_len, nrhs=1, tol=1e-9, sweeps=20, dxp=d[0], dyp=d[1], tAp=None, a_len=0):
            rc = L.qpdo_amd_fleet_tangent_dev(F._h, nrhs, tqp, None, None, None, tAp, dxp, dyp, *ttail, tol, sweeps, n_len, m_len, 0, a_len, None)
            if rc:
                raise RuntimeError((L.qpdo_amd_last_error() or b"").decode())

        g = gx.data_ptr()
        hostbuf = np.ones(2 * N)
        refused(F, lambda: raw(g, N, M, nrhs=0), "nrhs is 0, it must be at least 1")
        refused(F, lambda: raw(g, N, M, nrhs=-3), "nrhs is -3, it must be at least 1")
        refused(F, lambda: raw(g, N, M, nrhs=2 ** 31), "nrhs is %d, the kernel counts at most %d" % (2 ** 31, 2 ** 31 - 1))
        refused(F, lambda: raw(g, N + 1, M), "n_len is %d, the fleet's packed n-vectors have %d" % (N + 1, N))
        refused(F, lambda: raw(g, N, M - 1), "m_len is %d, the fleet's packed m-vectors have %d" % (M - 1, M))
        refused(F, lambda: raw(hostbuf.ctypes.data, N, M), "gx is not device memory")
        refused(F, lambda: raw(g, N, M, dqp=hostbuf.ctypes.data), "dq is not device memory")
        refused(F, lambda: raw(None, N, M), "gx is NULL")
        refused(F, lambda: raw(g, N, M, tol=0.0), "tol is")
        refused(F, lambda: raw(g, N, M, sweeps=0), "max_sweeps is 0")
        t1 = tq.data_ptr()
        refused(F, lambda: rawt(t1, N, M, nrhs=0), "nrhs is 0, it must be at least 1")
        refused(F, lambda: rawt(t1, N + 2, M), "n_len is %d, the fleet's packed n-vectors have %d" % (N + 2, N))
        refused(F, lambda: rawt(None, N, M), "no tangent passed")
        refused(F, lambda: rawt(t1, N, M, dxp=None), "dx is NULL")
        refused(F, lambda: rawt(t1, N, M, dyp=None), "dy is NULL")
        refused(F, lambda: rawt(hostbuf.ctypes.data, N, M), "tq is not device memory")
        refused(F, lambda: rawt(t1, N, M, tol=float("nan")), "tol is")
        refused(F, lambda: rawt(t1, N, M, tAp=t1, a_len=N), "tAx was passed, but")
        raw(g, N, M); rawt(t1, N, M)                                                                    # ... and with nothing wrong they launch
        assert F.sensitivity_stats()["calls"] == before + 2 and F.adjoint_stats()["adjoint_calls"] == 0
        assert C.sizeof(solver.FleetSensitivityStats) == 24 and C.sizeof(solver.FleetAdjointStats) == 16
        assert L.qpdo_amd_fleet_rhs_group(None) == -1 and 1 <= F.rhs_group() <= 8
    finally:
        F.close(); H.close()


# ---- 7. a side stream -------------------------------------------------------------------------------------------------------------------------
def streams():
    probs = list(fleet("B"))
    F = solver.Fleet(probs, adjoint=True, scaling=10, **ST)
    try:
        N, M, _, _ = sizes(F, False)
        R = F.rhs_group() + 1
        rng = np.random.default_rng(8)
        gx, tq = gpu(rng.standard_normal((R, N))), gpu(rng.standard_normal((R, N)))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        F.solve_device()                                    # on the current stream ...
        with torch.cuda.stream(side):                       # ... the sensitivities on another one: ordered by the fleet's event alone
            a = F.adjoint_many_device(gx, out=adj_sentinel(F, R, False))
            d = F.tangent_device(tq=tq, out=tan_sentinel(F, R))
        a, d = host(a), host(d)
        a2, d2 = host(F.adjoint_many_device(gx, out=adj_sentinel(F, R, False))), host(F.tangent_device(tq=tq, out=tan_sentinel(F, R)))
        assert (a["status"][:, :, 0] == 0).all() and (d["status"][:, :, 0] == 0).all()
        for k in ("dq", "dl", "du", "active", "status", "residual"):
            same_bits(a[k], a2[k], k)
        for k in ("dx", "dy", "active", "status", "residual"):
            same_bits(d[k], d2[k], k)
        assert F.sensitivity_stats()["calls"] == 4
    finally:
        F.close()


# ---- 8. the layer ---------------------------------------------------------------------------------------------------------------------------
def fleet_qp_layer():
    probs = list(fleet("P"))
    F = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)
    try:
        N, M, NQ, NA = sizes(F)
        (no, mo) = F.packed_layout()
        R = F.rhs_group() + 1
        rng = np.random.default_rng(21)
        gx, gy = gpu(rng.standard_normal((R, N))), gpu(rng.standard_normal((R, M)))
        t = {k: gpu(v) for k, v in perturbation(F, probs, rng, R).items()}
        layer = FleetQP(F, on_failure="nan")
        try:
            layer.tangent(tq=t["tq"])
        except RuntimeError as e:
            assert "no forward yet" in str(e), str(e)
        else:
            raise AssertionError("a tangent before any forward was not refused")
        layer(gpu(np.concatenate([p["q"] for p in probs])))
        got_t, got_v = layer.tangent(**t), layer.vjp_many(gx, gy, matrices=True)
        dt, dv = F.tangent_device(**t), F.adjoint_many_device(gx, gy, matrices=True)
        got_t, got_v, dt, dv = host(got_t), host(got_v), host(dt), host(dv)
        for k in ("dx", "dy", "active", "status", "residual"):
            same_bits(got_t[k], dt[k], "tangent " + k)
        for k in ADJ_KEYS + ("active", "status", "residual"):
            same_bits(got_v[k], dv[k], "vjp_many " + k)
        assert got_v["status"][:, :2, 0].tolist() == [[2, 2]] * R and np.isnan(got_v["dq"][:, :int(no[2])]).all() and np.isnan(got_t["dx"][:, :int(no[2])]).all()
        assert same_or_none(layer.vjp_status, dv["status"]) and same_or_none(layer.tangent_status, dt["status"])
        # "zero": the slices of the right-hand sides that were not delivered are zeros, the others keep their bits
        lz = FleetQP(F, on_failure="zero")
        lz()
        zt, zv = host(lz.tangent(**t)), host(lz.vjp_many(gx, gy, matrices=True))
        dt, dv = host(F.tangent_device(**t)), host(F.adjoint_many_device(gx, gy, matrices=True))
        qo, ao = F.packed_matrix_layout()
        for z, dd, keys in ((zt, dt, (("dx", no), ("dy", mo))), (zv, dv, tuple(zip(ADJ_KEYS, (no, mo, mo, qo, ao))))):
            for k, off in keys:
                assert not np.isnan(z[k]).any(), k
                for r in range(R):
                    for i in range(F.count):
                        s = slice(int(off[i]), int(off[i + 1]))
                        if dd["status"][r, i, 0]:
                            assert not bits(z[k][r, s]).any() and np.isnan(dd[k][r, s]).all(), (k, r, i)
                        else:
                            assert bit_equal(z[k][r, s], dd[k][r, s]), (k, r, i)
        # sensitivities that belong to an earlier forward
        layer()
        lz()                                                # (the same fleet: it has moved on)
        for call, nm in ((lambda: layer.tangent(**t), "tangent"), (lambda: layer.vjp_many(gx, gy), "vjp_many")):
            try:
                call()
            except RuntimeError as e:
                assert "solved again since this forward" in str(e), str(e)
            else:
                raise AssertionError("a stale %s was not refused" % nm)
        lz.tangent(**t); lz.vjp_many(gx)                    # the most recent forward's are served
        torch.cuda.synchronize()
    finally:
        F.close()


def same_or_none(tensor, arr):
    return tensor is not None and np.array_equal(tensor.cpu().numpy(), arr)


SCENARIOS = {"adjoint_bits_%s[%d]" % (nm, sc): functools.partial(adjoint_bits, nm, sc) for nm in ("P", "B", "G") for sc in (10, 0)}
SCENARIOS.update({"tangent_%s[%d]" % (nm, sc): functools.partial(tangent_fleet, nm, sc) for nm in ("P", "B", "G") for sc in (10, 0)})
SCENARIOS.update({"duality[%s]" % nm: functools.partial(duality, nm) for nm in ("P", "B", "G")})
SCENARIOS.update({"no_bit_moves[%s]" % nm: functools.partial(no_bit_moves, nm) for nm in ("P", "B", "G")})
SCENARIOS.update({"refused_alone": refused_alone, "refusals_launch_nothing": refusals_launch_nothing, "streams": streams, "fleet_qp_layer": fleet_qp_layer})


def main():
    only = sys.argv[2:]                                     # (scenario names: a measuring run of a few of them)
    todo = {k: v for k, v in SCENARIOS.items() if not only or k in only}
    out = {}
    for name, run in todo.items():
        try:
            run()
            out[name] = "ok"
        except AssertionError:                      # a failed check: recorded, the other scenarios still run
            out[name] = traceback.format_exc()[-3000:]
        except Exception:                           # anything else may be a device error: nothing more is started on the GPU
            out[name] = traceback.format_exc()[-3000:]
            for rest in todo:
                out.setdefault(rest, "not run: '%s' ended with an error" % name)
        out["notes"] = {k: (v if isinstance(v, (int, float, str)) else list(map(int, v))) for k, v in NOTES.items()}
        with open(sys.argv[1], "w") as f:
            json.dump(out, f)
        if len(out) >= len(todo) + 1:
            break


if __name__ == "__main__":
    main()
