"""The fused small-QP kernel with the Newton matrix as a lower BAND in the workgroup's LDS (K_BAND, qpdo_small.hip small_factor_band /
small_ldl_solve_band; the rule: include/qpdo_amd_ext.h).  The contract: an item solved in the band layout returns what the global-memory
layout returns and what the CPU oracle returns, bit for bit, except that a zero may carry the other sign (a skipped subtraction of an exact
zero product).  Floats are therefore compared by bit pattern after adding +0.0; NaNs must match position by position; the elements that
differed in zero sign alone are counted and the count is printed (expected: 0).

The instances (qpdo_amd/problems.py) are chain-structured QPs whose packed factor does not fit one workgroup's LDS while the band image does:
  A banded_random_qp(1, 256, 12)  n 256 m 384  b 12   the plain case (alone: the latency kernel with the work vectors in LDS)
  B banded_qp(3, 301)             n 301 m 601  b 1    tridiagonal, n odd: the one-column steps
  C banded_random_qp(5, 333, 31)  n 333 m 499  b 31   n = 1 mod 4, b + 1 = 32
  D banded_random_qp(4, 610, 5)   n 610 m 915  b 5    long chain, b + 1 no multiple of 4, n beyond the packed one-wave solve
  E banded_qp(6, 512)             n 512 m 1023 b 1    m at the kernel's limit
  F banded_random_qp(2, 200, 70)  n 200 m 300  b 70   window wider than a wave, truncated windows for a third of the columns
With F in the launch the fixed part of (n 610, m 1023) leaves no room for F's 114 KB band image: that batch is the query's GLOBAL, and F
runs in the band layout as a batch of its own."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import binding as ob
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu
INFO_FIELDS = ("status_val", "iterations", "oterations", "objective", "res_prim_norm", "res_dual_norm", "res_prim_in_norm", "res_dual_in_norm")
GROUPS = ("ABCDEF", "ABCDE", "F", "A")


@functools.lru_cache(maxsize=None)
def shapes():
    return dict(A=problems.banded_random_qp(1, 256, 12), B=problems.banded_qp(3, 301), C=problems.banded_random_qp(5, 333, 31),
                D=problems.banded_random_qp(4, 610, 5), E=problems.banded_qp(6, 512), F=problems.banded_random_qp(2, 200, 70))


@functools.lru_cache(maxsize=None)
def oracle_cold(name, scaling):
    """the oracle's cold solve of one shape: computed once, shared by the tests"""
    o = ob.OracleSolver(shapes()[name], ob.default_settings(scaling=scaling, max_iter=1000, verbose=0))
    r = o.solve()
    o.close()
    return r


def bits_differ(a, b):
    """(number of elements that differ beyond the sign of a zero or where exactly one is NaN, number that differ in zero sign alone)"""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    if a.shape != b.shape:
        return max(a.size, b.size, 1), 0
    na, nb = np.isnan(a), np.isnan(b)
    ca, cb = (a + 0.0).view(np.int64), (b + 0.0).view(np.int64)          # -0.0 + 0.0 = +0.0
    bad = (na != nb) | (~na & ~nb & (ca != cb))
    sign_only = ~na & ~nb & (ca == cb) & (a.view(np.int64) != b.view(np.int64))
    return int(bad.sum()), int(sign_only.sum())


def compare(got, ref, what, certificates=False):
    """status, counts, objective, the four norms, x, y (and the certificates): returns (messages, zero-sign count)"""
    msgs, zs = [], 0
    gi, ri = got["info"], ref["info"]
    for f in INFO_FIELDS[:3]:
        if int(gi[f]) != int(ri[f]):
            msgs.append("%s: %s %r != %r" % (what, f, gi[f], ri[f]))
    fields = [(f, gi[f], ri[f]) for f in INFO_FIELDS[3:]] + [("x", got["x"], ref["x"]), ("y", got["y"], ref["y"])]
    if certificates:
        if int(ri["status_val"]) == -3:
            fields.append(("prim_inf_cert", got["prim_inf_cert"], ref["prim_inf_cert"]))
        if int(ri["status_val"]) == -4:
            fields.append(("dual_inf_cert", got["dual_inf_cert"], ref["dual_inf_cert"]))
    for f, g, r in fields:
        bad, z = bits_differ(g, r)
        zs += z
        if bad:
            msgs.append("%s: %s differs in %d element(s)" % (what, f, bad))
    return msgs, zs


def check_batch(res, names, scaling, what):
    msgs, zs = [], 0
    for k, r in zip(names, res):
        m, z = compare(r, oracle_cold(k, scaling), "%s, %s" % (what, k))
        msgs += m
        zs += z
    return msgs, zs


@functools.lru_cache(maxsize=None)
def batches(scaling):
    """every group once through solve_batch in this process: {group: (results, layout reported, layout by the query)}"""
    S, out = shapes(), {}
    for g in GROUPS:
        probs = [S[k] for k in g]
        res, failed = solver.solve_batch(probs, max_iter=1000, verbose=0, scaling=scaling)
        assert failed == 0
        out[g] = (res, solver.batch_factor_layout(), solver.small_factor_layout(probs, solver.KIND_BATCH, verbose=0)[0])
    return out


@pytest.mark.parametrize("scaling", [10, 0])
def test_batch_against_the_oracle(scaling, gpu_required):
    msgs, zs = [], 0
    for g, (res, reported, queried) in batches(scaling).items():
        assert reported == queried, (g, reported, queried)
        m, z = check_batch(res, g, scaling, "batch %s" % g)
        msgs += m
        zs += z
        assert [int(r["info"]["status_val"]) for r in res] == [1] * len(g), g
    lay = {g: v[1] for g, v in batches(scaling).items()}
    print("layouts %r; elements that differ in zero sign alone: %d" % (lay, zs))
    assert lay["ABCDE"] == solver.K_BAND and lay["A"] == solver.K_BAND, lay
    assert not msgs, msgs[:10]


@pytest.mark.parametrize("scaling", [10, 0])
def test_band_against_global_memory_in_the_same_build(scaling, gpu_required, tmp_path):
    """the same batches in a fresh child process with QPDO_SMALL_BAND=0: every launch reports GLOBAL and returns the same values"""
    out = str(tmp_path / "global.npz")
    env = dict(os.environ, QPDO_SMALL_BAND="0")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_small_band_worker.py")
    p = subprocess.run([sys.executable, worker, out, str(scaling), ",".join(GROUPS)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    rec = np.load(out)
    msgs, zs = [], 0
    for g, (res, reported, _) in batches(scaling).items():
        assert rec["%s_layout" % g].tolist() == [solver.K_GLOBAL, 0], (g, rec["%s_layout" % g])
        for k, r in zip(g, res):
            info = dict(zip(INFO_FIELDS, rec["%s_%s_info" % (g, k)]))
            m, z = compare(r, dict(info=info, x=rec["%s_%s_x" % (g, k)], y=rec["%s_%s_y" % (g, k)]), "%s, %s: this process against QPDO_SMALL_BAND=0" % (g, k))
            msgs += m
            zs += z
    print("elements that differ in zero sign alone: %d" % zs)
    assert batches(scaling)["ABCDE"][1] == solver.K_BAND
    assert not msgs, msgs[:10]


@pytest.mark.parametrize("scaling", [10, 0])
def test_stream_against_the_oracle(scaling, gpu_required):
    """a batch of a stream takes the wide kernel"""
    names = "ABCDE"
    probs = [shapes()[k] for k in names]
    assert solver.small_factor_layout(probs, solver.KIND_STREAM, verbose=0)[0] == solver.K_BAND
    bs = solver.BatchStream(depth=2)
    try:
        b1, b2 = solver.Batch(probs), solver.Batch(probs[::-1])
        st = dict(max_iter=1000, verbose=0, scaling=scaling)
        t1, t2 = bs.submit(b1, **st), bs.submit(b2, **st)
        r1, _ = bs.wait(t1)
        r2, _ = bs.wait(t2)
    finally:
        bs.close()
    m1, z1 = check_batch(r1, names, scaling, "stream")
    m2, z2 = check_batch(r2, names[::-1], scaling, "stream, reversed")
    print("elements that differ in zero sign alone: %d" % (z1 + z2))
    assert not (m1 + m2), (m1 + m2)[:10]


def finite(v):
    return np.nan_to_num(np.asarray(v, float), nan=0.0)


def clipped(v):
    return np.clip(np.asarray(v, float), -1e20, 1e20)


@pytest.mark.parametrize("scaling", [10, 0])
def test_fleet_sequence_against_one_oracle_per_item(scaling, gpu_required):
    """the seven steps of tests/test_gpu_fleet.py (re-stated): cold, warm starts, partial bound update, update_q, warm start then update_q,
    warm_start_last then update of q and bounds -- on a fleet in the band layout with both infeasible KATs and an item with m = 0"""
    S = shapes()
    probs = [problems.infeasibility_kat("primal_infeasible"), problems.infeasibility_kat("dual_infeasible"), S["A"], S["B"], S["C"],
             problems.random_qp(21, 30, 0, 0.2)]
    st = dict(scaling=scaling, max_iter=1000, verbose=0)
    os_ = [ob.OracleSolver(p, ob.default_settings(**st)) for p in probs]
    F = solver.Fleet(probs, **st)
    rng = np.random.default_rng(7)
    msgs, zs, statuses = [], 0, []
    try:
        assert F.factor_layout() == solver.K_BAND == solver.small_factor_layout(probs, solver.KIND_FLEET, verbose=0)[0]

        def solve(name):
            nonlocal zs
            rg, ro = F.solve(), [o.solve() for o in os_]
            for i, (g, o) in enumerate(zip(rg, ro)):
                m, z = compare(g, o, "%s, item %d" % (name, i), certificates=True)
                msgs.extend(m)
                zs += z
            statuses.append([int(r["info"]["status_val"]) for r in rg])
            return ro

        ro = solve("1 cold")
        xw = [finite(r["x"]) + 1e-3 * rng.standard_normal(p["n"]) for r, p in zip(ro, probs)]
        yw = [finite(r["y"]) + 1e-3 * rng.standard_normal(p["m"]) for r, p in zip(ro, probs)]
        F.warm_start(xw, yw)
        for o, x, y in zip(os_, xw, yw):
            o.warm_start(x, y)
        solve("2 warm start x, y")
        F.warm_start(xw, None)
        for o, x in zip(os_, xw):
            o.warm_start(x, None)
        solve("3 warm start x only")
        l2 = [p["l"] - 0.1 if i % 2 == 0 else None for i, p in enumerate(probs)]
        u2 = [p["u"] + 0.05 if i % 2 == 0 else None for i, p in enumerate(probs)]
        F.update(l=l2, u=u2)
        for o, l, u in zip(os_, l2, u2):
            if l is not None:
                o.update_bounds(clipped(l), clipped(u))
        solve("4 update bounds, even items")
        q2 = [1.5 * p["q"] + 0.1 for p in probs]
        F.update(q=q2)
        for o, q in zip(os_, q2):
            o.update_q(q)
        ro = solve("5 update q")
        xs, ys = [finite(r["x"]) for r in ro], [finite(r["y"]) for r in ro]
        q3 = [q + 0.01 * rng.standard_normal(len(q)) for q in q2]
        F.warm_start(xs, ys)
        F.update(q=q3)
        for o, x, y, q in zip(os_, xs, ys, q3):
            o.warm_start(x, y)
            o.update_q(q)
        ro = solve("6 warm start, then update q")
        q4 = [q - 0.02 * rng.standard_normal(len(q)) for q in q3]
        l4, u4 = [p["l"] - 0.05 for p in probs], [p["u"] + 0.1 for p in probs]
        F.warm_start_last()
        F.update(q=q4, l=l4, u=u4)
        for o, r, q, l, u in zip(os_, ro, q4, l4, u4):
            if r["info"]["status_val"] in (-3, -4):
                o.warm_start(None, None)
            else:
                o.warm_start(r["x"], r["y"])
            o.update_bounds(clipped(l), clipped(u))
            o.update_q(q)
        solve("7 warm_start_last, then update q and bounds")
        assert F.factor_layout() == solver.K_BAND
    finally:
        F.close()
        for o in os_:
            o.close()
    print("statuses of the cold solve %r; elements that differ in zero sign alone: %d" % (statuses[0], zs))
    assert len(statuses) == 7 and statuses[0][0] == -3 and statuses[0][1] == -4 and statuses[0].count(1) >= 3, statuses
    assert not msgs, msgs[:10]


@pytest.mark.parametrize("scaling", [10, 0])
def test_matrix_updates_keep_the_band(scaling, gpu_required):
    """new Q and A values in the same pattern, then the real-time-iteration step update -> warm_start_last -> solve, against an oracle set
    up on the new matrices"""
    S = shapes()
    probs = [S["A"], S["C"]]
    st = dict(scaling=scaling, max_iter=1000, verbose=0)
    rng = np.random.default_rng(11)
    F = solver.Fleet(probs, matrix_updates=True, **st)
    os_ = []
    try:
        assert F.factor_layout() == solver.K_BAND
        r0 = F.solve()
        msgs, zs = check_batch(r0, "AC", scaling, "fleet, cold")
        new = []
        for p in probs:
            Qn, An = p["Q"].copy(), p["A"].copy()
            Qn.data = Qn.data * 1.25                                      # (stays positive semidefinite)
            An.data = An.data * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, An.nnz))
            new.append(dict(p, Q=Qn, A=An, l=clipped(p["l"]), u=clipped(p["u"])))
        F.update_matrices(Q=[p["Q"] for p in new], A=[p["A"] for p in new])
        q2 = [1.1 * p["q"] + 0.05 for p in probs]
        l2, u2 = [p["l"] - 0.02 for p in probs], [p["u"] + 0.03 for p in probs]
        F.update(q=q2, l=l2, u=u2)
        F.warm_start_last()
        r1 = F.solve()
        assert F.factor_layout() == solver.K_BAND
        for i, p in enumerate(new):
            o = ob.OracleSolver(p, ob.default_settings(**st))
            os_.append(o)
            o.update_bounds(clipped(l2[i]), clipped(u2[i]))
            o.update_q(q2[i])
            o.warm_start(r0[i]["x"], r0[i]["y"])
            m, z = compare(r1[i], o.solve(), "after update_matrices, item %d" % i, certificates=True)
            msgs += m
            zs += z
    finally:
        F.close()
        for o in os_:
            o.close()
    print("elements that differ in zero sign alone: %d" % zs)
    assert [int(r["info"]["status_val"]) for r in r0] == [1, 1]
    assert not msgs, msgs[:10]


def test_two_runs_give_the_same_bits(gpu_required):
    first = batches(10)["ABCDE"][0]
    again, failed = solver.solve_batch([shapes()[k] for k in "ABCDE"], max_iter=1000, verbose=0, scaling=10)
    assert failed == 0 and solver.batch_factor_layout() == solver.K_BAND
    for k, a, b in zip("ABCDE", first, again):
        for f in INFO_FIELDS:
            assert np.asarray(a["info"][f], float).tobytes() == np.asarray(b["info"][f], float).tobytes(), (k, f)
        assert a["x"].tobytes() == b["x"].tobytes() and a["y"].tobytes() == b["y"].tobytes(), k
