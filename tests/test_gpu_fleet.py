"""A resident FLEET of small QPs (qpdo_amd_fleet_*, solver.Fleet; qpdo_small.hip k_small_fleet*): set up once, then update / warm start /
solve as one launch each for all items.  The contract: item i carries the BITS of a workspace of its own driven through the reference's
API in the same order -- checked here against one OracleSolver per item (status, counts, x, y, objective, the four residual norms and the
certificates), over a sequence that exercises the reference's quirks: a solve clears `initialized`, update_q reads whatever x / Qx the
last solve or warm start left, a solve that runs out of passes keeps an earlier status."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from qpdo_amd import problems, solver
from test_gpu_small import assert_identical, same_bits

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fleet_problems(with_big=True):
    """heterogeneous on purpose: n = 2 infeasible KATs, two C3 items (n = 120, m = 360), m = 0, equality rows and, with_big, an item whose
    packed factor (200 * 201 / 2 * 8 B = 160 800 B) exceeds one workgroup's LDS.  Where K lives is decided per FLEET: with that item every
    item keeps K and its work vectors in global memory and factors without look-ahead; without it every item has the packed factor and the
    work vectors in LDS, the look-ahead factorization and the factor restore from global memory -- the layout of a fleet of C3 items.  Both
    are run through the whole sequence."""
    big = (problems.random_qp(22, 200, 300, 0.05),) if with_big else ()
    return (problems.infeasibility_kat("primal_infeasible"), problems.infeasibility_kat("dual_infeasible"),
            problems.config_qp("C3", 0), problems.config_qp("C3", 5),
            problems.random_qp(21, 30, 0, 0.2)) + big + (problems.random_qp(23, 40, 60, 0.2, 10),)


def finite(v):
    """an infeasible item returns NaN: there is no solution to start from, the warm start of such an item uses zeros (fleet and oracle alike)"""
    return np.nan_to_num(np.asarray(v, float), nan=0.0)


@functools.lru_cache(maxsize=None)
def run_sequence(scaling, with_big=True):
    """the seven steps on one fleet and on one oracle per item; returns [(step name, fleet results, oracle results)] and the fleet's
    statistics after create, after every solve, and after the partial update of step 4"""
    probs = fleet_problems(with_big)
    st = dict(scaling=scaling, max_iter=1000, verbose=0)
    os_ = [ob.OracleSolver(p, ob.default_settings(**st)) for p in probs]
    F = solver.Fleet(list(probs), **st)
    N = len(probs)
    rng = np.random.default_rng(7)
    out, stats = [], dict(create=F.stats(), solves=[])

    def solve(name):
        rg, ro = F.solve(), [o.solve() for o in os_]
        out.append((name, rg, ro))
        stats["solves"].append(F.stats())
        return ro

    ro = solve("1 cold")
    xw = [finite(r["x"]) + 1e-3 * rng.standard_normal(p["n"]) for r, p in zip(ro, probs)]
    yw = [finite(r["y"]) + 1e-3 * rng.standard_normal(p["m"]) for r, p in zip(ro, probs)]
    F.warm_start(xw, yw)
    for o, x, y in zip(os_, xw, yw):
        o.warm_start(x, y)
    ro = solve("2 warm start x, y")
    F.warm_start(xw, None)
    for o, x in zip(os_, xw):
        o.warm_start(x, None)
    ro = solve("3 warm start x only")
    l2 = [p["l"] - 0.1 if i % 2 == 0 else None for i, p in enumerate(probs)]
    u2 = [p["u"] + 0.05 if i % 2 == 0 else None for i, p in enumerate(probs)]
    F.update(l=l2, u=u2)
    stats["partial_update"] = (F.stats(), 8 * sum(2 * p["m"] for i, p in enumerate(probs) if i % 2 == 0) + solver.FLEET_TABLE_BYTES * N)
    for o, l, u in zip(os_, l2, u2):
        if l is not None:
            o.update_bounds(np.clip(l, -1e20, 1e20), np.clip(u, -1e20, 1e20))
    ro = solve("4 update bounds, even items")
    q2 = [1.5 * p["q"] + 0.1 for p in probs]
    F.update(q=q2)
    for o, q in zip(os_, q2):
        o.update_q(q)
    ro = solve("5 update q")
    xs, ys = [finite(r["x"]) for r in ro], [finite(r["y"]) for r in ro]
    q3 = [q + 0.01 * rng.standard_normal(len(q)) for q in q2]
    F.warm_start(xs, ys)
    F.update(q=q3)                                     # update_q after a warm start reads the warm-started Qx, x (qpdo.c:556-560)
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
        o.update_bounds(np.clip(l, -1e20, 1e20), np.clip(u, -1e20, 1e20))
        o.update_q(q)
    solve("7 warm_start_last, then update q and bounds")
    F.close()
    for o in os_:
        o.close()
    return out, stats


@pytest.mark.parametrize("with_big", [True, False], ids=["K_in_global_memory", "K_in_LDS"])
@pytest.mark.parametrize("scaling", [10, 0])
def test_sequence_parity_on_a_heterogeneous_fleet(scaling, with_big, gpu_required):
    out, _ = run_sequence(scaling, with_big)
    assert len(out) == 7
    bad = []
    for name, rg, ro in out:
        for i, (g, o) in enumerate(zip(rg, ro)):
            try:
                assert_identical(g, o, what="%s, item %d" % (name, i))
            except AssertionError as e:
                bad.append(str(e)[:400])
    assert not bad, bad
    # the fleet exercised what it is meant to: both infeasible statuses and solved items in the cold solve
    sts = [r["info"]["status_val"] for r in out[0][1]]
    assert sts[0] == -3 and sts[1] == -4 and sts.count(1) >= 4, sts


def test_cold_solve_equals_the_batch_path(gpu_required):
    probs = list(fleet_problems())
    st = dict(max_iter=1000, verbose=0)
    rb, failed = solver.solve_batch(probs, **st)
    assert failed == 0
    F = solver.Fleet(probs, **st)
    rf = F.solve()
    F.close()
    for i, (a, b) in enumerate(zip(rf, rb)):
        ai, bi = a["info"], b["info"]
        for f in ("status_val", "iterations", "oterations", "objective", "res_prim_norm", "res_dual_norm", "res_prim_in_norm", "res_dual_in_norm"):
            assert ai[f] == bi[f], (i, f, ai[f], bi[f])
        assert same_bits(a["x"], b["x"]) and same_bits(a["y"], b["y"]), i


def two_steps(probs):
    F = solver.Fleet(probs, max_iter=1000, verbose=0)
    r1 = F.solve()
    F.warm_start_last()
    F.update(q=[1.2 * p["q"] - 0.05 for p in probs], l=[p["l"] - 0.02 for p in probs])
    r2 = F.solve()
    F.close()
    return r1, r2


def identical_results(a, b):
    return (a["info"]["status_val"], a["info"]["iterations"], a["info"]["oterations"], a["info"]["objective"]) == \
        (b["info"]["status_val"], b["info"]["iterations"], b["info"]["oterations"], b["info"]["objective"]) and \
        same_bits(a["x"], b["x"]) and same_bits(a["y"], b["y"])


def test_items_are_independent_and_runs_are_deterministic(gpu_required):
    a, b, c = problems.config_qp("C3", 1), problems.random_qp(31, 50, 80, 0.2, 5), problems.random_qp(32, 33, 47, 0.3)
    abc, ca, again = two_steps([a, b, c]), two_steps([c, a]), two_steps([a, b, c])
    for s in range(2):
        assert identical_results(abc[s][0], ca[s][1]), ("a", s)
        assert identical_results(abc[s][2], ca[s][0]), ("c", s)
        for i in range(3):
            assert identical_results(abc[s][i], again[s][i]), (i, s)


@pytest.mark.parametrize("with_big", [True, False], ids=["K_in_global_memory", "K_in_LDS"])
def test_iteration_cap_and_warm_start_last(with_big, gpu_required):
    probs = [problems.config_qp("C3", 2)] + ([problems.random_qp(22, 200, 300, 0.05)] if with_big else []) + [problems.random_qp(23, 40, 60, 0.2, 10)]
    st = dict(max_iter=5, verbose=0)
    os_ = [ob.OracleSolver(p, ob.default_settings(**st)) for p in probs]
    F = solver.Fleet(probs, **st)
    r1, o1 = F.solve(), [o.solve() for o in os_]
    assert [r["info"]["status_val"] for r in r1] == [-5] * len(probs)
    F.warm_start_last()
    for o, r in zip(os_, o1):
        o.warm_start(r["x"], r["y"])
    r2, o2 = F.solve(), [o.solve() for o in os_]
    for i in range(len(probs)):
        assert_identical(r1[i], o1[i], what="capped, item %d" % i)
        assert_identical(r2[i], o2[i], what="capped + warm_start_last, item %d" % i)
    F.close()
    for o in os_:
        o.close()


def test_a_solve_that_runs_out_of_passes_keeps_the_earlier_status(gpu_required):
    """qpdo.c:451-453: MAX_ITER_REACHED overwrites an UNSOLVED status only.  max_iter = 22 lets the cold solve of the first item end solved
    (21 passes on the oracle); after the update of q the next solve, from zero, needs 36 and runs out: the status stays 1 while the
    iteration count says 22 -- on the oracle, and bit for bit on the fleet."""
    probs = [problems.random_qp(32, 33, 47, 0.3), problems.infeasibility_kat("primal_infeasible")]
    st = dict(max_iter=22, verbose=0)
    os_ = [ob.OracleSolver(p, ob.default_settings(**st)) for p in probs]
    F = solver.Fleet(probs, **st)
    r1, o1 = F.solve(), [o.solve() for o in os_]
    q2 = [3.0 * p["q"] + 0.5 for p in probs]
    F.update(q=q2)
    for o, q in zip(os_, q2):
        o.update_q(q)
    r2, o2 = F.solve(), [o.solve() for o in os_]
    assert (o1[0]["info"]["status_val"], o2[0]["info"]["status_val"], o2[0]["info"]["iterations"]) == (1, 1, 22)      # the scenario itself
    for i in range(len(probs)):
        assert_identical(r1[i], o1[i], what="cold, item %d" % i)
        assert_identical(r2[i], o2[i], what="out of passes after a solved solve, item %d" % i)
    F.close()
    for o in os_:
        o.close()


@pytest.mark.parametrize("with_big", [True, False], ids=["K_in_global_memory", "K_in_LDS"])
def test_the_fleet_stays_resident(with_big, gpu_required):
    _, stats = run_sequence(10, with_big)
    created = stats["create"]
    assert created["count"] == len(fleet_problems(with_big)) and created["matrix_bytes_uploaded"] > 0 and created["solves"] == 0
    for k, s in enumerate(stats["solves"]):
        assert s["matrix_bytes_uploaded"] == created["matrix_bytes_uploaded"], k
        assert s["solve_launches"] == s["solves"] == k + 1
        assert s["last_kernel_seconds"] > 0
    s, expected = stats["partial_update"]
    assert s["vector_bytes_uploaded_last_call"] == expected


def test_refusals(gpu_required):
    ok = [problems.config_qp("C3", 3), problems.random_qp(32, 33, 47, 0.3)]
    big = problems.random_qp(41, 1500, 10, 0.002)
    with pytest.raises(RuntimeError, match="item 1 does not fit the fused kernel"):
        solver.Fleet([ok[0], big], verbose=0)
    F = solver.Fleet(ok, verbose=0)                     # a refused create leaves nothing behind: the next fleet works
    os_ = [ob.OracleSolver(p, ob.default_settings(verbose=0)) for p in ok]
    for g, o in zip(F.solve(), os_):
        assert_identical(g, o.solve(), what="after a refused create")
        o.close()
    n0, m0 = ok[0]["n"], ok[0]["m"]
    with pytest.raises(ValueError):
        F.update(q=[np.zeros(n0)])                      # wrong list length
    with pytest.raises(ValueError):
        F.update(q=[np.zeros(n0 + 1), None])            # wrong vector shape
    with pytest.raises(ValueError):
        F.warm_start([None, None], [np.zeros(m0), np.zeros(3)])
    with pytest.raises(RuntimeError, match="greater than upper bound"):
        F.update(l=[ok[0]["u"] + 1.0, None], u=[ok[0]["u"], None])
    F.close()
