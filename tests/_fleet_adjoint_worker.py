"""Child process of tests/test_gpu_fleet_adjoint.py: the scenarios of the fleet's adjoint call (qpdo_amd_fleet_adjoint_dev,
solver.Fleet.adjoint_device, qpdo_amd.torch_layer.FleetQP), each run once, their outcomes written as JSON.  A process of its own because
torch comes FIRST here (one HIP runtime in the process; tests/_fleet_device_worker.py).

The reference is tests/fleet_adjoint_ref.py (numpy, longdouble).  Everything is checked against the DEVICE's flags: with vx = -dq and
vy = dl + du read back, the longdouble residual of the unscaled adjoint system must be at most
    tol max(||gx||, ||gy_S||) + (n + k + 2) eps || |M| |v| ||_inf
(the second term: the rounding of the kernel's own fp64 residual evaluation, the standard dot-product bound), and where M's float64
condition number is below 1 / eps -- beyond that a float64 inverse says nothing -- also ||v - v_ref|| <= 2 ||M^-1||_inf (that bound).
usage: _fleet_adjoint_worker.py OUT.json
       _fleet_adjoint_worker.py --record PATH     (writes what the scenario parent_bits compares against: tests/golden/fleet_adjoint_parent_bits.json)"""
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
from qpdo_amd import problems, solver  # noqa: E402
from qpdo_amd.torch_layer import FleetQP  # noqa: E402
from _fleet_device_worker import band_problems, bit_equal, bits, compare_host, pack  # noqa: E402
from _fleet_matrices_device_worker import lp_item  # noqa: E402
from test_gpu_fleet_matrices import fleet_problems, new_A, new_Q  # noqa: E402

ST = dict(max_iter=1000, verbose=0)
EPS = float(np.finfo(np.float64).eps)
TOL = 1e-9
SENTINEL = 12345.678
NOTES = {}


def eq_item(seed=7):
    """a strictly convex QP over a box with two equality rows (l_i = u_i): always active, whatever y says"""
    rng = np.random.default_rng(seed)
    n = 8
    B = rng.standard_normal((n, n))
    Q = sp.csc_matrix(np.tril(B @ B.T + n * np.eye(n)))
    A = sp.csc_matrix(np.vstack([rng.standard_normal((2, n)), np.eye(n)]))
    b = np.array([0.3, -0.2])
    return dict(n=n, m=n + 2, Q=Q, Qstype=-1, A=A, q=rng.standard_normal(n), l=np.concatenate([b, -np.ones(n)]), u=np.concatenate([b, np.ones(n)]), c=0.0)


def dup_item(seed=9):
    """eq_item with its first equality row stored twice: two identical active rows -- consistent for gy = 0, not for gy that differs on them"""
    p = eq_item(seed)
    A = sp.csc_matrix(sp.vstack([p["A"][0], p["A"]]))
    return dict(p, m=p["m"] + 1, A=A, l=np.concatenate([p["l"][:1], p["l"]]), u=np.concatenate([p["u"][:1], p["u"]]))


@functools.lru_cache(maxsize=None)
def fleet(name):
    if name == "P":
        return tuple(fleet_problems(False)) + (lp_item(), eq_item())
    if name == "B":
        return tuple(band_problems())
    # G: a dense-pattern item of n = 256, m = 300 -- neither the packed triangle nor a band of at most 128 fits one workgroup's LDS
    return (problems.random_qp(31, 256, 300, 1.0, 20), problems.random_qp(23, 40, 60, 0.2, 10))


LAYOUT = dict(P=solver.K_PACKED, B=solver.K_BAND, G=solver.K_GLOBAL)


def gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def sentinel_out(F, matrices):
    """output tensors pre-filled with a sentinel: an entry the kernel never wrote is seen"""
    no, mo = F.packed_layout()
    N, M = int(no[-1]), int(mo[-1])
    d = dict(dq=torch.full((N,), SENTINEL, dtype=torch.float64).cuda(), dl=torch.full((M,), SENTINEL, dtype=torch.float64).cuda(),
             du=torch.full((M,), SENTINEL, dtype=torch.float64).cuda(), active=torch.full((M,), 77, dtype=torch.int32).cuda(),
             status=torch.full((F.count, 3), -77, dtype=torch.int64).cuda(), residual=torch.full((F.count,), SENTINEL, dtype=torch.float64).cuda())
    if matrices:
        qo, ao = F.packed_matrix_layout()
        d.update(dQ_values=torch.full((int(qo[-1]),), SENTINEL, dtype=torch.float64).cuda(), dA_values=torch.full((int(ao[-1]),), SENTINEL, dtype=torch.float64).cuda())
    return d


def check_item(p, x, y, flags, dq, dl, du, gx, gy, tol, what):
    """the solve check and the placement check of one accepted item; returns (vx, vy) in longdouble"""
    n, m = p["n"], p["m"]
    Qf, A = ref.full_Q(p["Q"], p["Qstype"]), (ref.dense(p["A"]) if m else np.zeros((0, n)))
    M, S = ref.kkt(Qf, A, flags)
    k = len(S)
    vx, vy = -dq.astype(ref.LD), (dl + du).astype(ref.LD)
    v = np.concatenate([vx, vy[S]])
    rhs = np.concatenate([gx.astype(ref.LD), (gy[S] if gy is not None else np.zeros(k)).astype(ref.LD)])
    assert np.isfinite(v.astype(np.float64)).all(), (what, "not finite")
    gn = float(np.abs(rhs).max()) if len(rhs) else 0.0
    r = float(np.abs(M @ v - rhs).max())
    bound = tol * gn + (n + k + 2) * EPS * float((np.abs(M) @ np.abs(v)).max())
    assert r <= bound, (what, "residual", r, bound)
    M64 = M.astype(np.float64)
    cond = np.linalg.cond(M64) if M64.size else 1.0
    if np.isfinite(cond) and cond < 1.0 / EPS:
        minv = float(np.abs(np.linalg.inv(M64)).sum(axis=1).max())
        vref, _ = ref.solve_ref(M, rhs)
        err = float(np.abs(v - vref).max())
        assert err <= 2.0 * minv * bound, (what, "error", err, 2.0 * minv * bound)
    # placement: du lives on +1 rows, dl on -1 rows, everything else is a bitwise +0.0
    assert not bits(du)[flags != 1].any() and not bits(dl)[flags != -1].any(), (what, "placement")
    return vx, vy


def check_matrices(p, x, y, flags, vx, vy, dQ, dA, what):
    g = ref.gradients(p["Q"], p["Qstype"], p["A"], flags, x, y, vx, vy)
    tQ, tA = ref.matrix_terms(p["Q"], p["Qstype"], p["A"], flags, x, y, vx, vy)
    assert len(dQ) == len(g["dQ_values"]) and len(dA) == len(g["dA_values"]), what
    assert (np.abs(dQ.astype(ref.LD) - g["dQ_values"]) <= 4 * EPS * tQ).all(), (what, "dQ")
    assert (np.abs(dA.astype(ref.LD) - g["dA_values"]) <= 4 * EPS * tA).all(), (what, "dA")
    Acsc = sp.csc_matrix(p["A"]); Acsc.sort_indices()
    assert not bits(dA)[flags[Acsc.indices] == 0].any(), (what, "entries of inactive rows are +0.0")


def run_checks(F, probs, sol, out, gx, gy, tol, matrices, what, expect_all_accepted):
    """every per-item check of one adjoint call; returns the device flags and the number of rows skipped for their margin"""
    no, mo = F.packed_layout()
    o = host(out)
    sx, sy, st = sol["x"], sol["y"], sol["status"]
    skipped = rows = 0
    for i, p in enumerate(probs):
        n0, n1, m0, m1 = int(no[i]), int(no[i + 1]), int(mo[i]), int(mo[i + 1])
        code, sweeps, k = o["status"][i].tolist()
        w = "%s item %d" % (what, i)
        sl = [o["dq"][n0:n1], o["dl"][m0:m1], o["du"][m0:m1]]
        if matrices:
            qo, ao = F.packed_matrix_layout()
            sl += [o["dQ_values"][int(qo[i]):int(qo[i + 1])], o["dA_values"][int(ao[i]):int(ao[i + 1])]]
        if st[i][0] != 1:
            assert code == 2, (w, code)
        else:
            assert code in ((0,) if expect_all_accepted else (0, 1)), (w, code, sweeps)
        if code != 0:
            assert all(np.isnan(s).all() for s in sl) and not o["active"][m0:m1].any() and np.isnan(o["residual"][i]), (w, "NaN slices, 0 flags")
            continue
        assert not any(np.isnan(s).any() for s in sl) and all((s != SENTINEL).all() for s in sl), (w, "NaN or an unwritten entry")
        assert o["residual"][i] <= tol and 0 <= sweeps <= 20, (w, o["residual"][i], sweeps)
        x, y, flags = sx[n0:n1], sy[m0:m1], o["active"][m0:m1]
        assert k == int((flags != 0).sum()) and set(np.unique(flags)) <= {-1, 0, 1}, w
        l, u = np.clip(p["l"], -1e20, 1e20), np.clip(p["u"], -1e20, 1e20)
        if p["m"]:
            mg = ref.margins(x, y, p["A"], l, u)
            sure = mg >= 1e-9
            assert (flags[sure] == ref.classify(x, y, ref.dense(p["A"]), l, u)[sure]).all(), (w, "flags")
            skipped += int((~sure).sum()); rows += p["m"]
        gyi = None if gy is None else gy[m0:m1]
        vx, vy = check_item(p, x, y, flags, sl[0], sl[1], sl[2], gx[n0:n1], gyi, tol, w)
        if matrices:
            check_matrices(p, x, y, flags, vx, vy, sl[3], sl[4], w)
    assert skipped <= 0.01 * max(rows, 1), (what, "rows below the margin", skipped, rows)
    return o["active"], skipped


def one_fleet(name, scaling):
    probs = list(fleet(name))
    both = name == "P"
    assert solver.small_factor_layout(probs, solver.KIND_FLEET, scaling=scaling, **ST)[0] == LAYOUT[name]
    F = solver.Fleet(probs, matrix_updates=both, adjoint=True, scaling=scaling, **ST)
    try:
        assert F.factor_layout() == LAYOUT[name]
        no, mo = F.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        sol = host(F.solve_device())
        sts = sol["status"][:, 0].tolist()
        if name == "P":
            assert sts[0] == -3 and sts[1] == -4 and sts[2:] == [1] * (len(probs) - 2), sts
            assert [p["Qstype"] for p in probs[:3]] == [-1, 1, 0] and any(p["m"] == 0 for p in probs) and sp.csc_matrix(probs[-2]["Q"]).nnz == 0
        else:
            assert sts == [1] * len(probs), sts
        rng = np.random.default_rng(100 + scaling)
        gx = rng.standard_normal(N)
        out = F.adjoint_device(gpu(gx), None, matrices=both, out=sentinel_out(F, both), tol=TOL)
        flags, skipped = run_checks(F, probs, sol, out, gx, None, TOL, both, "%s[%d] gy=None" % (name, scaling), True)
        NOTES["skipped_rows %s[%d]" % (name, scaling)] = skipped
        NOTES["sweeps %s[%d]" % (name, scaling)] = host(out)["status"][:, 1].tolist()
        # a random gy with NaN on every inactive row: NaN must not reach an accepted item (dependent active rows may make gy inconsistent: code 1)
        gy = rng.standard_normal(M)
        gy[flags == 0] = np.nan
        out = F.adjoint_device(gpu(gx), gpu(gy), matrices=both, out=sentinel_out(F, both), tol=TOL)
        flags2, _ = run_checks(F, probs, sol, out, gx, gy, TOL, both, "%s[%d] gy" % (name, scaling), False)
        codes = host(out)["status"][:, 0].tolist()
        NOTES["codes with gy %s[%d]" % (name, scaling)] = codes
        assert sum(c == 0 for c in codes) >= sum(s == 1 for s in sts) - 1, codes
        assert F.adjoint_stats()["adjoint_calls"] == 2
    finally:
        F.close()


def not_accepted():
    probs = [problems.random_qp(23, 40, 60, 0.2, 10), dup_item(), eq_item()]
    F = solver.Fleet(probs, adjoint=True, scaling=10, **ST)
    try:
        no, mo = F.packed_layout()
        sol = host(F.solve_device())
        assert sol["status"][:, 0].tolist() == [1, 1, 1]
        rng = np.random.default_rng(3)
        gx = rng.standard_normal(int(no[-1]))
        gy = np.zeros(int(mo[-1]))
        gy[int(mo[1])], gy[int(mo[1]) + 1] = 1.0, -1.0        # the two identical (equality, hence active) rows of item 1
        out = F.adjoint_device(gpu(gx), gpu(gy), out=sentinel_out(F, False), tol=TOL)
        o = host(out)
        assert o["status"][:, 0].tolist() == [0, 1, 0] and o["status"][1, 1] == 20, o["status"].tolist()
        run_checks(F, probs, sol, out, gx, gy, TOL, False, "inconsistent gy", False)
        out = F.adjoint_device(gpu(gx), None, out=sentinel_out(F, False), tol=TOL)
        assert host(out)["status"][:, 0].tolist() == [0, 0, 0]
        run_checks(F, probs, sol, out, gx, None, TOL, False, "gy=None", True)
    finally:
        F.close()


def no_bit_moves(name):
    """P: the work vectors and K live in LDS; B: K in LDS, G: K and the work vectors in the items' GLOBAL scratch, which the adjoint overwrites"""
    probs = list(fleet(name))
    X = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)       # adjoint calls after every solve
    Y = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)       # the flag, never asked
    Z = solver.Fleet(probs, matrix_updates=True, scaling=10, **ST)                      # no flag
    try:
        assert X.factor_layout() == Y.factor_layout() == Z.factor_layout() == LAYOUT[name]
        no, mo = X.packed_layout()
        rng = np.random.default_rng(5)
        gx, gy = gpu(rng.standard_normal(int(no[-1]))), gpu(rng.standard_normal(int(mo[-1])))

        def solve(what):
            outs = [host(F.solve_device()) for F in (X, Y, Z)]
            for k in outs[0]:
                assert bit_equal(outs[0][k], outs[1][k]) and bit_equal(outs[0][k], outs[2][k]), (what, k)
            a1 = host(X.adjoint_device(gx, gy, matrices=True))
            a2 = host(X.adjoint_device(gx, None, matrices=True))
            solved = outs[0]["status"][:, 0] == 1
            # (which of the solved items are ACCEPTED is not this scenario's business: the badly scaled matrices of the last step are not;
            # the codes go to the notes)
            assert ((a1["status"][:, 0] == 2) == ~solved).all() and ((a2["status"][:, 0] == 2) == ~solved).all(), (what, a1["status"].tolist(), a2["status"].tolist())
            NOTES["codes, no_bit_moves[%s] %s" % (name, what)] = a2["status"][:, 0].tolist()
            compare_host(X.fetch_last(), Y.fetch_last(), "fetch_last after the adjoint calls, " + what)
            again = host(X._dev_out)
            for k in outs[0]:
                assert bit_equal(outs[0][k], again[k]), (what, k, "the solve's outputs after the adjoint calls")

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
        assert X.adjoint_stats()["adjoint_calls"] == 6 and Y.adjoint_stats()["adjoint_calls"] == 0
        sx, sy = X.stats(), Y.stats()
        assert (sx["solve_launches"], sx["solves"]) == (sy["solve_launches"], sy["solves"]) == (3, 3)
        assert X.adjoint_stats()["resident_extra_bytes"] == 0 and X.matrix_stats()["resident_extra_bytes"] == Z.matrix_stats()["resident_extra_bytes"]
    finally:
        X.close(); Y.close(); Z.close()


def refusals_launch_nothing():
    import ctypes as C
    probs = [problems.random_qp(23, 40, 60, 0.2, 10), eq_item()]
    F = solver.Fleet(probs, adjoint=True, scaling=10, **ST)
    G = solver.Fleet(probs, matrix_updates=True, scaling=10, **ST)
    try:
        no, mo = F.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        gx = gpu(np.ones(N))

        def counters(H):
            dev = H.sync()                              # (first: it also refreshes last_kernel_seconds of stats())
            return (dev, H.stats(), H.adjoint_stats(), H.matrix_stats() if H is G else None)

        def refused(H, call, msg):
            before = counters(H)
            try:
                call()
            except (RuntimeError, ValueError) as e:
                assert msg in str(e), (msg, str(e))
            else:
                raise AssertionError("not refused: " + msg)
            assert counters(H) == before, msg

        refused(F, lambda: F.adjoint_device(gx), "was not a solve")                                   # before any solve
        F.solve_device()
        ok = host(F.adjoint_device(gx))
        assert ok["status"][:, 0].tolist() == [0, 0] and F.adjoint_stats()["adjoint_calls"] == 1
        F.update_device(q=pack([p["q"] for p in probs]))
        refused(F, lambda: F.adjoint_device(gx), "was not a solve")                                   # after an update
        F.warm_start_last_device(); F.solve_device()
        G.solve_device()
        refused(G, lambda: G.adjoint_device(gx), "without QPDO_AMD_FLEET_ADJOINT")                    # a fleet without the flag
        refused(F, lambda: F.adjoint_device(gx, matrices=True), "QPDO_AMD_FLEET_MATRIX_UPDATES")      # matrices without the matrix flag
        L = solver.lib()
        out = F.adjoint_device(gx)                                                                    # (tensors to borrow addresses from)
        torch.cuda.synchronize()
        a = [out[k].data_ptr() for k in ("dq", "dl", "du")]
        tail = [None, None, out["active"].data_ptr(), out["status"].data_ptr(), out["residual"].data_ptr()]

        def raw(gxp, n_len, m_len, tol=1e-9, sweeps=20, dqp=a[0]):
            rc = L.qpdo_amd_fleet_adjoint_dev(F._h, gxp, None, dqp, a[1], a[2], *tail, tol, sweeps, n_len, m_len, 0, 0, None)
            if rc:
                raise RuntimeError((L.qpdo_amd_last_error() or b"").decode())

        refused(F, lambda: raw(gx.data_ptr(), N + 1, M), "n_len is %d, the fleet's packed n-vectors have %d" % (N + 1, N))
        refused(F, lambda: raw(gx.data_ptr(), N, M - 1), "m_len is %d, the fleet's packed m-vectors have %d" % (M - 1, M))
        hostbuf = np.ones(N)
        refused(F, lambda: raw(hostbuf.ctypes.data, N, M), "gx is not device memory")
        refused(F, lambda: raw(gx.data_ptr(), N, M, dqp=hostbuf.ctypes.data), "dq is not device memory")
        refused(F, lambda: raw(None, N, M), "gx is NULL")
        refused(F, lambda: raw(gx.data_ptr(), N, M, tol=0.0), "tol is")
        refused(F, lambda: raw(gx.data_ptr(), N, M, tol=float("nan")), "tol is")
        refused(F, lambda: raw(gx.data_ptr(), N, M, sweeps=0), "max_sweeps is 0")
        raw(gx.data_ptr(), N, M)                                                                       # ... and the same call with nothing wrong launches
        assert F.adjoint_stats()["adjoint_calls"] == 3
        assert C.sizeof(solver.FleetAdjointStats) == 16
    finally:
        F.close(); G.close()


def streams():
    probs = list(fleet("B"))
    F = solver.Fleet(probs, adjoint=True, scaling=10, **ST)
    try:
        no, mo = F.packed_layout()
        gx = gpu(np.random.default_rng(8).standard_normal(int(no[-1])))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        F.solve_device()                                    # on the current stream ...
        with torch.cuda.stream(side):                       # ... the adjoint on another one: ordered by the fleet's event alone
            a = F.adjoint_device(gx, out=sentinel_out(F, False))
        a = host(a)
        b = host(F.adjoint_device(gx, out=sentinel_out(F, False)))
        assert a["status"][:, 0].tolist() == [0, 0]
        for k in ("dq", "dl", "du", "active", "status", "residual"):
            assert bit_equal(a[k].astype(np.float64), b[k].astype(np.float64)), k
        assert F.adjoint_stats()["adjoint_calls"] == 2
    finally:
        F.close()


def fleet_qp_layer():
    probs = list(fleet("P"))
    F = solver.Fleet(probs, matrix_updates=True, adjoint=True, scaling=10, **ST)
    try:
        no, mo = F.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        qv, av, _ = F.pack_matrix_values(Q=[p["Q"] for p in probs], A=[p["A"] for p in probs])
        rng = np.random.default_rng(21)
        w, z = gpu(rng.standard_normal(N)), gpu(rng.standard_normal(M))

        def leaves(req):
            vals = [np.concatenate([p["q"] for p in probs]), np.concatenate([p["l"] for p in probs]), np.concatenate([p["u"] for p in probs]), qv, av]
            return [gpu(v).requires_grad_(r) for v, r in zip(vals, req)]

        def loss_of(x, y):
            return (w * torch.nan_to_num(x)).sum() + (z * torch.nan_to_num(y)).sum()

        layer = FleetQP(F, on_failure="nan")
        t = leaves([True] * 5)
        x, y = layer(*t)
        loss_of(x, y).backward()
        direct = host(F.adjoint_device(w, z, matrices=True))
        got = [host(dict(g=v.grad))["g"] for v in t]
        for g, k in zip(got, ("dq", "dl", "du", "dQ_values", "dA_values")):
            assert bit_equal(g, direct[k]), k
        codes = layer.adjoint_status[:, 0].tolist()
        assert codes[:2] == [2, 2] and layer.status[:2, 0].tolist() == [-3, -4] and np.isnan(got[0][:int(no[2])]).all(), codes
        # inputs that do not require a gradient get none
        t2 = leaves([True, False, False, False, True])
        x, y = layer(*t2)
        loss_of(x, y).backward()
        assert t2[0].grad is not None and t2[4].grad is not None and all(v.grad is None for v in t2[1:4])
        d2 = host(F.adjoint_device(w, z, matrices=True))     # (this forward started from the last solution: its own x, y, hence its own gradients)
        assert bit_equal(host(dict(g=t2[0].grad))["g"], d2["dq"]) and bit_equal(host(dict(g=t2[4].grad))["g"], d2["dA_values"])
        # "zero": the slices of the items that were not delivered are zeros, the others keep their bits
        lz = FleetQP(F, on_failure="zero")
        t3 = leaves([True] * 5)
        x, y = lz(*t3)
        loss_of(x, y).backward()
        qo, ao = F.packed_matrix_layout()
        d3 = host(F.adjoint_device(w, z, matrices=True))
        codes = lz.adjoint_status[:, 0].tolist()           # (the KAT items: 2; an item whose dependent active rows make z inconsistent: 1)
        assert codes == d3["status"][:, 0].tolist() and codes[:2] == [2, 2] and codes.count(0) >= len(probs) - 3, codes
        for v, g, off in zip(t3, [d3[k] for k in ("dq", "dl", "du", "dQ_values", "dA_values")], (no, mo, mo, qo, ao)):
            gz = host(dict(g=v.grad))["g"]
            assert not np.isnan(gz).any()
            for i, c in enumerate(codes):
                a, b = int(off[i]), int(off[i + 1])
                assert (not bits(gz[a:b]).any() and np.isnan(g[a:b]).all()) if c else bit_equal(gz[a:b], g[a:b]), (i, c)
        # nothing passed: no update at all, the solve alone (from the last solution), no gradient to anybody
        x0, y0 = layer()
        assert not x0.requires_grad and bit_equal(host(dict(x=x0))["x"], host(F._dev_out)["x"]) and layer.status.shape == (len(probs), 3)
        # a backward that belongs to an earlier forward
        t4 = leaves([True] * 5)
        x1, y1 = layer(*t4)
        x2, y2 = layer(*t4)
        try:
            loss_of(x1, y1).backward()
        except RuntimeError as e:
            assert "solved again since this forward" in str(e), str(e)
        else:
            raise AssertionError("a stale backward was not refused")
        loss_of(x2, y2).backward()
    finally:
        F.close()


GOLDEN_BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fleet_adjoint_parent_bits.json")
BITS_KEYS = ("dq", "dl", "du", "dQ_values", "dA_values", "active", "residual")


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def single_call_bits():
    """The single call's outputs on fleet P / B / G, scaling 10 and 0, gy None and given (NaN on the inactive rows), matrices off and on, from
    fixed seeds: per case the SHA-256 of x and y of the solve and of every output array, and the status array in full.  Only solve_device and
    adjoint_device are used, so the same function records (--record, at the commit whose bits are to be kept) and recomputes."""
    cases = {}
    for name in ("P", "B", "G"):
        for scaling in (10, 0):
            F = solver.Fleet(list(fleet(name)), matrix_updates=True, adjoint=True, scaling=scaling, **ST)
            try:
                assert F.factor_layout() == LAYOUT[name]
                no, mo = F.packed_layout()
                sol = host(F.solve_device())
                rng = np.random.default_rng(900 + scaling)
                gx = rng.standard_normal(int(no[-1]))
                flags = host(F.adjoint_device(gpu(gx)))["active"]
                gy = rng.standard_normal(int(mo[-1]))
                gy[flags == 0] = np.nan
                for with_gy in (False, True):
                    for matrices in (False, True):
                        o = host(F.adjoint_device(gpu(gx), gpu(gy) if with_gy else None, matrices=matrices, out=sentinel_out(F, matrices), tol=TOL))
                        c = {"x": sha(sol["x"]), "y": sha(sol["y"]), "status": o["status"].tolist()}
                        c.update({k: sha(o[k]) for k in BITS_KEYS if o.get(k) is not None})
                        assert len(c) == 3 + len(BITS_KEYS) - (0 if matrices else 2), sorted(c)
                        cases["%s[%d] gy=%s matrices=%s" % (name, scaling, with_gy, matrices)] = c
            finally:
                F.close()
    return cases


def parent_bits():
    """the single call delivers the bits it delivered at the commit before this scenario was added (the recording)"""
    with open(GOLDEN_BITS) as f:
        want = json.load(f)["cases"]
    got = single_call_bits()
    assert sorted(got) == sorted(want) and len(want) == 24, (sorted(got), sorted(want))
    stale = [k for k in want if (got[k]["x"], got[k]["y"]) != (want[k]["x"], want[k]["y"])]
    assert not stale, ("the SOLVE's x / y are not the recorded ones: the recording is stale (a change to the solve; record again), "
                       "this says nothing about the adjoint", stale)
    moved = {k: [f for f in want[k] if got[k].get(f) != want[k][f]] for k in want if got[k] != want[k]}
    assert not moved, ("the single adjoint call's outputs are not the recorded ones", moved)


def record(path):
    with open(path, "w") as f:
        json.dump({"cases": single_call_bits()}, f, indent=1, sort_keys=True)
        f.write("\n")


SCENARIOS = {"fleet_%s[%d]" % (nm, sc): functools.partial(one_fleet, nm, sc) for nm in ("P", "B", "G") for sc in (10, 0)}
SCENARIOS.update({"no_bit_moves[%s]" % nm: functools.partial(no_bit_moves, nm) for nm in ("P", "B", "G")})
SCENARIOS.update({"not_accepted": not_accepted, "refusals_launch_nothing": refusals_launch_nothing, "streams": streams,
                  "fleet_qp_layer": fleet_qp_layer, "parent_bits": parent_bits})


def main():
    if sys.argv[1] == "--record":
        return record(sys.argv[2])
    out = {}
    for name, run in SCENARIOS.items():
        try:
            run()
            out[name] = "ok"
        except AssertionError:                      # a failed check: recorded, the other scenarios still run
            out[name] = traceback.format_exc()[-3000:]
        except Exception:                           # anything else may be a device error: nothing more is started on the GPU
            out[name] = traceback.format_exc()[-3000:]
            for rest in SCENARIOS:
                out.setdefault(rest, "not run: '%s' ended with an error" % name)
        out["notes"] = {k: (v if isinstance(v, (int, float, str)) else list(map(int, v))) for k, v in NOTES.items()}
        with open(sys.argv[1], "w") as f:
            json.dump(out, f)
        if len(out) >= len(SCENARIOS) + 1:
            break


if __name__ == "__main__":
    main()
