"""New Q / A values for the items of a resident fleet (qpdo_amd_fleet_update_matrices, solver.Fleet.update_matrices; k_small_fleet_matrices in
qpdo_small.hip).  The contract is exact: an item that received an entry is afterwards, bit for bit, the workspace qpdo_setup leaves for its
new matrices, the latest unscaled q, l, u and the fleet's settings; an item without an entry is not touched.  So the oracle twin of an
updated item is a NEW OracleSolver on the new problem, which then receives the same later calls; the other items keep their oracle.
warm_start_last of an updated item starts from the x, y its last solve returned."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import binding as ob
from qpdo_amd import problems, solver
from test_gpu_small import assert_identical, same_bits

pytestmark = pytest.mark.gpu


def rescale(M, seed, spread=3.0, zeros=0):
    """the same pattern, new values: entries times r_i * c_j (log-uniform over 10^+-spread) times a random factor; `zeros` entries set to
    an explicit 0.0"""
    rng = np.random.default_rng(seed)
    M = sp.csc_matrix(M, copy=True)
    M.sort_indices()
    r = 10.0 ** rng.uniform(-spread, spread, M.shape[0])
    c = 10.0 ** rng.uniform(-spread, spread, M.shape[1])
    cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    M.data = M.data * r[M.indices] * c[cols] * rng.uniform(0.5, 2.0, len(M.data))
    if zeros:
        M.data[rng.choice(len(M.data), min(zeros, len(M.data)), replace=False)] = 0.0
    return M


def rescale_Q(Qf, seed, spread=2.0):
    """S Q S (positive diagonal S, a convex Q stays convex) in the same pattern"""
    rng = np.random.default_rng(seed)
    Qf = sp.csc_matrix(Qf, copy=True)
    Qf.sort_indices()
    s = 10.0 ** rng.uniform(-spread, spread, Qf.shape[0])
    cols = np.repeat(np.arange(Qf.shape[1]), np.diff(Qf.indptr))
    Qf.data = Qf.data * s[Qf.indices] * s[cols] * 3.7
    return Qf


def stored(Qf, st):
    """the storage of the full symmetric Qf for stype st, in the pattern the same call gave at create (explicit zeros stay)"""
    Qf = sp.csc_matrix(Qf)
    if st == 0:
        return Qf
    coo = Qf.tocoo()
    keep = coo.row >= coo.col if st < 0 else coo.row <= coo.col
    return sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=Qf.shape)


def with_stype(p, st):
    return dict(p, Q=stored(problems.full_Q(p), st), Qstype=st)


def new_Q(p, seed):
    """(s_i q_ij) s_j and (s_j q_ji) s_i round differently: the lower triangle is mirrored, so that the full storage (stype 0) is symmetric in bits"""
    L = sp.tril(rescale_Q(problems.full_Q(p), seed)).tocsc()
    return stored(problems.full_Q(dict(Q=L, Qstype=-1)), p["Qstype"])


def new_A(p, seed):
    """positive factors: the infeasible KATs stay infeasible; a few explicit zeros in the larger items"""
    return rescale(p["A"], seed, 3.0, zeros=3 if p["n"] > 2 else 0)


@functools.lru_cache(maxsize=None)
def fleet_problems(with_big=True):
    """the heterogeneous fleet of test_gpu_fleet.py (both of its C3 items: with one, the fleet without the big item could not have the four
    solved items asserted below); Qstype -1, +1, 0 in turn (the three mapQ rules).  with_big: an item whose packed factor exceeds one
    workgroup's LDS -- the whole fleet then keeps K in global memory."""
    big = (problems.random_qp(22, 200, 300, 0.05),) if with_big else ()
    ps = (problems.infeasibility_kat("primal_infeasible"), problems.infeasibility_kat("dual_infeasible"), problems.config_qp("C3", 0),
          problems.config_qp("C3", 5), problems.random_qp(21, 30, 0, 0.2)) + big + (problems.random_qp(23, 40, 60, 0.2, 10),)
    return tuple(with_stype(p, (-1, 1, 0)[i % 3]) for i, p in enumerate(ps))


def finite(v):
    return np.nan_to_num(np.asarray(v, float), nan=0.0)


def clipped(v):
    return np.clip(np.asarray(v, float), -1e20, 1e20)


class Twins:
    """one oracle per item plus what a fresh setup of the item would be given: its current matrices and its latest unscaled q, l, u"""

    def __init__(self, probs, st):
        self.st = st
        self.cur = [dict(p, l=clipped(p["l"]), u=clipped(p["u"])) for p in probs]
        self.os = [ob.OracleSolver(p, ob.default_settings(**st)) for p in self.cur]

    def update(self, q=None, l=None, u=None):
        for i, o in enumerate(self.os):
            if l is not None and l[i] is not None or u is not None and u[i] is not None:
                li = None if l is None or l[i] is None else clipped(l[i])
                ui = None if u is None or u[i] is None else clipped(u[i])
                o.update_bounds(li, ui)
                self.cur[i] = dict(self.cur[i], **{k: v for k, v in (("l", li), ("u", ui)) if v is not None})
            if q is not None and q[i] is not None:
                o.update_q(q[i])
                self.cur[i] = dict(self.cur[i], q=np.asarray(q[i], float))

    def update_matrices(self, Q=None, A=None):
        """a NEW oracle for every item that has an entry"""
        for i in range(len(self.os)):
            Qi, Ai = None if Q is None else Q[i], None if A is None else A[i]
            if Qi is None and Ai is None:
                continue
            self.cur[i] = dict(self.cur[i], **{k: v for k, v in (("Q", Qi), ("A", Ai)) if v is not None})
            self.os[i].close()
            self.os[i] = ob.OracleSolver(self.cur[i], ob.default_settings(**self.st))

    def warm_start(self, x, y):
        for i, o in enumerate(self.os):
            o.warm_start(None if x is None else x[i], None if y is None else y[i])

    def warm_start_last(self, last):
        for o, r in zip(self.os, last):
            if r["info"]["status_val"] in (-3, -4, -10, -99):
                o.warm_start(None, None)
            else:
                o.warm_start(r["x"], r["y"])

    def solve(self):
        return [o.solve() for o in self.os]

    def close(self):
        for o in self.os:
            o.close()


def pick(vals, idx):
    return [v if i in idx else None for i, v in enumerate(vals)]


@functools.lru_cache(maxsize=None)
def run_sequence(scaling, with_big=True):
    """the six steps on one fleet and on the twins; returns [(step, fleet results, oracle results)] and, per step, the items left out of
    its matrix call(s)"""
    probs = fleet_problems(with_big)
    N = len(probs)
    st = dict(scaling=scaling, max_iter=1000, verbose=0)
    T = Twins(probs, st)
    F = solver.Fleet(list(probs), matrix_updates=True, **st)
    rng = np.random.default_rng(11)
    out, left_out = [], {}

    def solve(name):
        rg, ro = F.solve(), T.solve()
        out.append((name, rg, ro))
        return ro

    def both(method, *a, **kw):
        getattr(F, method)(*a, **kw)
        getattr(T, method)(*a, **kw)

    def matrices(step, idx_Q, idx_A, seed):
        Q = pick([new_Q(p, seed + 10 * i) for i, p in enumerate(probs)], idx_Q) if idx_Q else None
        A = pick([new_A(p, seed + 10 * i + 1) for i, p in enumerate(probs)], idx_A) if idx_A else None
        both("update_matrices", Q=Q, A=A)
        left_out.setdefault(step, set(range(N)))
        left_out[step] &= set(range(N)) - set(idx_Q) - set(idx_A)

    all_items, even, odd = set(range(N)), set(range(0, N, 2)), set(range(1, N, 2))
    solve("1 cold")
    both("update", q=[1.5 * p["q"] + 0.1 for p in probs], l=[p["l"] - 0.1 for p in probs], u=[p["u"] + 0.05 for p in probs])
    matrices(2, even, even, 100)
    ro = solve("2 update q, l, u; new Q and A on the even items; from zero")
    matrices(3, {i for i in all_items if i % 3 == 1}, {i for i in all_items if i % 3 == 0}, 200)
    F.warm_start_last()
    T.warm_start_last(ro)
    ro = solve("3 A only / Q only / neither; warm_start_last")
    xw = [finite(r["x"]) + 1e-3 * rng.standard_normal(p["n"]) for r, p in zip(ro, probs)]
    yw = [finite(r["y"]) + 1e-3 * rng.standard_normal(p["m"]) for r, p in zip(ro, probs)]
    both("warm_start", xw, yw)
    matrices(4, odd, odd, 300)                           # the warm start of the odd items is discarded, the even items keep theirs
    solve("4 warm start, then new Q and A on the odd items")
    some = {0, 3, N - 1}
    matrices(5, some, some, 400)
    both("update", q=[p["q"] * 0.7 - 0.2 for p in probs])      # qpdo_update_q on a fresh workspace: x = Qx = 0 and setup's c
    solve("5 new Q and A on some items, then update q")
    matrices(6, even, even, 500)
    same = {1}                                           # the values the item already has: a fresh setup on them
    Q = pick([new_Q(p, 600 + 10 * i) for i, p in enumerate(probs)], even)
    A = pick([new_A(p, 601 + 10 * i) for i, p in enumerate(probs)], even)
    for i in same:
        Q[i], A[i] = T.cur[i]["Q"], T.cur[i]["A"]
    both("update_matrices", Q=Q, A=A)
    left_out[6] &= all_items - even - same
    solve("6 two matrix calls in a row; the values an item already has")
    F.close()
    T.close()
    return out, left_out


@pytest.mark.parametrize("with_big", [True, False], ids=["K_in_global_memory", "K_in_LDS"])
@pytest.mark.parametrize("scaling", [10, 0])
def test_sequence_parity_with_fresh_oracles(scaling, with_big, gpu_required):
    out, left_out = run_sequence(scaling, with_big)
    assert len(out) == 6
    bad = []
    for name, rg, ro in out:
        for i, (g, o) in enumerate(zip(rg, ro)):
            try:
                assert_identical(g, o, what="%s, item %d" % (name, i))
            except AssertionError as e:
                bad.append(str(e)[:400])
    assert not bad, bad
    # the run exercised what it claims: both infeasible statuses and solved items in the cold solve, an untouched item in every matrix step
    sts = [r["info"]["status_val"] for r in out[0][1]]
    assert sts[0] == -3 and sts[1] == -4 and sts.count(1) >= 4, sts
    assert sorted(left_out) == [2, 3, 4, 5, 6] and all(left_out[s] for s in left_out), left_out


# random_qp(32, 33, 47, 0.3) ends solved in 21 passes from zero (test_gpu_fleet.py); with these values the oracle needs 33, more than the 22 allowed
QUIRK_SEED = 7


def quirk_problems():
    p = with_stype(problems.random_qp(32, 33, 47, 0.3), -1)
    return p, dict(p, Q=new_Q(p, QUIRK_SEED), A=new_A(p, QUIRK_SEED + 1))


def test_new_matrices_reset_the_status_an_out_of_passes_solve_would_keep(gpu_required):
    """qpdo.c:451-453: MAX_ITER_REACHED overwrites an UNSOLVED status only.  After update_matrices the status IS unsolved, as in a fresh
    workspace: a solve that runs out of passes reports that, not the 1 the item had before."""
    p, pn = quirk_problems()
    kat = with_stype(problems.infeasibility_kat("primal_infeasible"), -1)
    st = dict(max_iter=22, verbose=0)
    o_old, o_new = ob.OracleSolver(p, ob.default_settings(**st)), ob.OracleSolver(pn, ob.default_settings(**st))
    o_kat = ob.OracleSolver(kat, ob.default_settings(**st))
    F = solver.Fleet([p, kat], matrix_updates=True, **st)
    r1, o1 = F.solve(), [o_old.solve(), o_kat.solve()]
    F.update_matrices(Q=[pn["Q"], None], A=[pn["A"], None])
    r2, o2 = F.solve(), [o_new.solve(), o_kat.solve()]
    assert o1[0]["info"]["status_val"] == 1 and (o2[0]["info"]["status_val"], o2[0]["info"]["iterations"]) == (-5, 22)      # the scenario itself
    for i in range(2):
        assert_identical(r1[i], o1[i], what="cold, item %d" % i)
        assert_identical(r2[i], o2[i], what="out of passes after new matrices, item %d" % i)
    F.close()
    for o in (o_old, o_new, o_kat):
        o.close()


def three_steps(probs, a_index, a_new, matrix_call=True):
    F = solver.Fleet(probs, matrix_updates=True, max_iter=1000, verbose=0)
    r1 = F.solve()
    if matrix_call:
        F.update_matrices(Q=pick([a_new["Q"]] * len(probs), {a_index}), A=pick([a_new["A"]] * len(probs), {a_index}))
    F.warm_start_last()
    r2 = F.solve()
    F.close()
    return r1, r2


def identical_results(a, b):
    return (a["info"]["status_val"], a["info"]["iterations"], a["info"]["oterations"], a["info"]["objective"]) == \
        (b["info"]["status_val"], b["info"]["iterations"], b["info"]["oterations"], b["info"]["objective"]) and \
        same_bits(a["x"], b["x"]) and same_bits(a["y"], b["y"])


def test_items_are_independent_and_runs_are_deterministic(gpu_required):
    a, b, c = problems.config_qp("C3", 1), problems.random_qp(31, 50, 80, 0.2, 5), problems.random_qp(32, 33, 47, 0.3)
    a, b, c = with_stype(a, 1), with_stype(b, -1), with_stype(c, 0)
    an = dict(a, Q=new_Q(a, 71), A=new_A(a, 72))
    abc, ca, again = three_steps([a, b, c], 0, an), three_steps([c, a], 1, an), three_steps([a, b, c], 0, an)
    plain = three_steps([a, b, c], 0, an, matrix_call=False)
    for s in range(2):
        assert identical_results(abc[s][0], ca[s][1]), ("a", s)
        assert identical_results(abc[s][2], ca[s][0]), ("c", s)
        for i in range(3):
            assert identical_results(abc[s][i], again[s][i]), (i, s)
        for i in (1, 2):                                 # no entry: as if the matrix call had never been made
            assert identical_results(abc[s][i], plain[s][i]), (i, s)
    assert not identical_results(abc[1][0], plain[1][0])  # (and a's new values did arrive)


def test_refusals_and_atomicity(gpu_required):
    ok = [with_stype(problems.config_qp("C3", 3), -1), with_stype(problems.random_qp(32, 33, 47, 0.3), -1)]
    st = dict(max_iter=1000, verbose=0)
    plain = solver.Fleet(ok, **st)
    with pytest.raises(RuntimeError, match="QPDO_AMD_FLEET_MATRIX_UPDATES"):
        plain.update_matrices(A=[ok[0]["A"], None])
    plain.close()
    F = solver.Fleet(ok, matrix_updates=True, **st)
    A1, Q1 = sp.csc_matrix(ok[1]["A"]), sp.csc_matrix(ok[1]["Q"])
    A1.sort_indices()
    good_A0, good_Q0 = new_A(ok[0], 5), new_Q(ok[0], 6)

    fewer = A1.copy()
    fewer.data[0] = 0.0
    fewer.eliminate_zeros()
    with pytest.raises(RuntimeError, match="item 1: A has a different number of entries"):
        F.update_matrices(A=[good_A0, fewer])            # (a valid item 0 rides along: the call is all-or-nothing)
    moved = A1.copy()
    last = moved.indptr[1:] - 1                          # the last entry of a column: moving it one row down keeps the column sorted
    k = [k for j, k in enumerate(last) if k >= moved.indptr[j] and moved.indices[k] < moved.shape[0] - 1][0]
    moved.indices[k] += 1
    with pytest.raises(RuntimeError, match="item 1: A has a row index that differs"):
        F.update_matrices(Q=[good_Q0, None], A=[good_A0, moved])
    with pytest.raises(ValueError, match="expected a list of 2"):
        F.update_matrices(A=[good_A0])
    with pytest.raises(ValueError, match=r"A\[1\]: expected shape"):
        F.update_matrices(A=[good_A0, sp.csc_matrix((A1.shape[0], A1.shape[1] + 1))])
    with pytest.raises(ValueError, match=r"Q\[0\]: expected shape"):
        F.update_matrices(Q=[sp.csc_matrix((3, 3)), None])

    # what the Python front end cannot produce: a different stype, a different ncol and a NULL x, through ctypes
    L, keep = solver.lib(), []
    arr = (C.POINTER(solver.CholmodSparse) * 2)()

    def call(which, view):
        arr[0], arr[1] = C.pointer(solver._sparse_view(good_A0 if which == "A" else good_Q0, 0 if which == "A" else -1, keep)), C.pointer(view)
        rc = L.qpdo_amd_fleet_update_matrices(F._h, arr if which == "Q" else None, arr if which == "A" else None)
        return rc, (L.qpdo_amd_last_error() or b"").decode()

    v = solver._sparse_view(Q1, 1, keep)
    rc, msg = call("Q", v)
    assert rc != 0 and "item 1: Q has a different stype" in msg, msg
    v = solver._sparse_view(A1, 0, keep)
    v.ncol = A1.shape[1] - 1
    rc, msg = call("A", v)
    assert rc != 0 and "item 1: A has a different number of columns" in msg, msg
    v = solver._sparse_view(A1, 0, keep)
    v.x = None
    rc, msg = call("A", v)
    assert rc != 0 and "item 1: A has a NULL value array x" in msg, msg

    # every refused call carried a valid item 0: nothing of it arrived
    os_ = [ob.OracleSolver(p, ob.default_settings(**st)) for p in ok]
    for i, (g, o) in enumerate(zip(F.solve(), os_)):
        assert_identical(g, o.solve(), what="after refused matrix calls, item %d" % i)
        o.close()
    assert F.matrix_stats()["calls"] == 0
    F.close()


def test_stats(gpu_required):
    probs = [with_stype(problems.random_qp(23, 40, 60, 0.2, 10), 1), with_stype(problems.random_qp(21, 30, 0, 0.2), 0),
             with_stype(problems.random_qp(32, 33, 47, 0.3), -1)]
    st = dict(max_iter=1000, verbose=0)
    plain, flags0 = solver.Fleet(probs, **st), None
    F = solver.Fleet(probs, matrix_updates=True, **st)
    assert plain.matrix_stats() == dict(calls=0, items_last_call=0, value_bytes_uploaded_last_call=0, resident_extra_bytes=0, last_kernel_seconds=0.0)
    # create_ex with flags 0 is create
    img = solver.Batch(probs)
    arr = (C.POINTER(solver.QPDOData) * 3)(*[img.items[i].data for i in range(3)])
    h = solver.lib().qpdo_amd_fleet_create_ex(3, arr, C.byref(solver.default_settings(**st)), 0)
    assert h
    flags0 = solver.FleetStats()
    assert solver.lib().qpdo_amd_fleet_get_stats(h, C.byref(flags0)) == 0
    solver.lib().qpdo_amd_fleet_destroy(h)
    assert flags0.matrix_bytes_uploaded == plain.stats()["matrix_bytes_uploaded"]
    nnzA = [sp.csc_matrix(p["A"]).nnz for p in probs]
    nnzQ = [sp.csc_matrix(p["Q"]).nnz for p in probs]
    # the flag's maps ride in create's upload: 4 bytes per entry of A and of the full Q (none for stype 0), in 256-byte aligned regions
    full = [problems.full_Q(p).nnz for p in probs]
    maps = sum(4 * a + 4 for a in nnzA) + sum(4 * f + 4 for f, p in zip(full, probs) if p["Qstype"] != 0)
    grown = F.stats()["matrix_bytes_uploaded"] - plain.stats()["matrix_bytes_uploaded"]
    assert maps <= grown <= maps + 256 * 2 * len(probs), (maps, grown)
    assert F.matrix_stats()["resident_extra_bytes"] >= grown + 8 * (sum(nnzA) + sum(nnzQ))
    F.solve()
    before = F.stats()
    F.update_matrices(Q=[new_Q(probs[0], 1), None, None], A=[new_A(probs[0], 2), None, new_A(probs[2], 3)])
    ms = F.matrix_stats()
    assert ms["calls"] == 1 and ms["items_last_call"] == 2 and ms["last_kernel_seconds"] > 0
    assert ms["value_bytes_uploaded_last_call"] == 8 * (nnzQ[0] + nnzA[0] + nnzA[2]) + solver.FLEET_MATRIX_TABLE_BYTES * 3
    after = F.stats()
    for f in ("matrix_bytes_uploaded", "solve_launches", "solves"):
        assert after[f] == before[f], f
    F.update_matrices()                                  # both None: returns, launches nothing
    assert F.matrix_stats()["calls"] == 1
    F.update_matrices(Q=[None, new_Q(probs[1], 4), None])
    ms = F.matrix_stats()
    assert ms["calls"] == 2 and ms["items_last_call"] == 1
    assert ms["value_bytes_uploaded_last_call"] == 8 * nnzQ[1] + solver.FLEET_MATRIX_TABLE_BYTES * 3
    plain.close()
    F.close()
