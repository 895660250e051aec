"""qpdo_amd_update_matrices (QPDO.update_matrices): new values of Q and A in the setup's pattern.  The contract is exact: afterwards the
workspace is, bit for bit, the one qpdo_setup returns for the new matrices with the latest unscaled q, l, u and the current settings.  Each
case sets up W1 on the old problem and solves it, updates W1, optionally warm-starts it from the old solution and solves again; its twin
W2 is set up fresh on the new problem and gets the same calls.  Products, counts, iterates, norms and every trace field must agree."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import assert_same_trace
from oracle import binding as ob
from qpdo_amd import problems, solver
from test_gpu_small import TRACE_FIELDS, assert_identical, oracle_run, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return sp.tril(Qf).tocsc() if st < 0 else sp.triu(Qf).tocsc() if st > 0 else sp.csc_matrix(Qf)


def new_problem(p, seed, zerosA=3, spread=1.0):
    """spread 1: values that move by orders of magnitude (a stale D / E, factor or norm_q would show); small: an SQP-like step"""
    Qf = rescale_Q(problems.full_Q(p), seed, 2.0 * spread)
    return dict(p, Qfull=Qf, A=rescale(p["A"], seed + 1, 3.0 * spread, zeros=zerosA))


def products(s, n, m, seed=5):
    rng = np.random.default_rng(seed)
    vn, vm = rng.standard_normal(n), rng.standard_normal(m)
    return (s.spmv(0, vn) if m else np.zeros(0), s.spmv(1, vm) if m else np.zeros(n), s.spmv(2, vn))


def assert_twins(a, b, what=""):
    (pa, ra, ta), (pb, rb, tb) = a, b
    for u, v in zip(pa, pb):
        assert np.array_equal(u, v), what
    assert_identical(ra, rb, what=what)
    assert len(ta) == len(tb), what
    for k, (g, r) in enumerate(zip(ta, tb)):
        for f in TRACE_FIELDS:
            assert same_bits(g[f], r[f]), (what, k, f, g[f], r[f])


def run_case(p, seed=11, st=-1, idt=None, settings=None, pre=None, post=None, warm=True, which="QA", settings_change=None, zerosA=3):
    """returns ((products, result, trace) of W1 after the update, the same of its fresh twin W2)"""
    settings = dict(dict(verbose=0, max_iter=300), **(settings or {}))
    pn = new_problem(p, seed, zerosA)
    Qf_old = problems.full_Q(p)
    Qn = pn["Qfull"] if "Q" in which else Qf_old
    An = pn["A"] if "A" in which else p["A"]
    w1 = solver.QPDO().setup(stored(Qf_old, st), p["q"], p["A"], p["l"], p["u"], Qstype=st, index_dtype=idt, **settings)
    r_old = w1.solve()
    q, l, u = p["q"], p["l"], p["u"]
    if settings_change:
        w1.update_settings(**settings_change)
        settings = dict(settings, **settings_change)
    if pre:
        q, l, u = pre(w1, q, l, u)
    w1.update_matrices(Q=stored(Qn, st) if "Q" in which else None, A=An if "A" in which else None)
    out = []
    x0, y0 = r_old["x"], r_old["y"]
    ws = warm and np.all(np.isfinite(x0)) and np.all(np.isfinite(y0))
    w2 = solver.QPDO().setup(stored(Qn, st), q, An, l, u, Qstype=st, index_dtype=idt, **settings)
    for w in (w1, w2):
        if post:
            post(w)
        prods = products(w, p["n"], p["m"])
        if ws:
            w.warm_start(x0, y0)
        r = solve(w)
        out.append((prods, r, r["trace"]))
        w.delete()
    return out


def solve(w):
    r = w.solve()
    r["stats"], r["trace"] = w.stats(), w.trace()
    return r


def shift_q(w, q, l, u):
    q2 = q * 1.5 + 0.01
    w.update_q(q2)
    return q2, l, u


def shift_bounds(w, q, l, u):
    l2, u2 = l - 0.05, u + 0.1
    w.update_bounds(l2, u2)
    return q, l2, u2


def post_q(w):
    w.update_q(np.linspace(-1.0, 1.0, w.n))


def post_bounds(w):
    w.update_bounds(None, np.full(w.m, 2.0))


ROUTES = {
    "fused_C3": (lambda: problems.config_qp("C3"), {}),
    "generic_C3": (lambda: problems.config_qp("C3"), {"QPDO_SMALL_FUSED": "0"}),
    "mid_C1": (lambda: problems.config_qp("C1"), {}),
    "mid_1000": (lambda: problems.random_qp(31, 1000, 2000, 0.01, 0), {}),
    "woodbury_1000": (lambda: problems.random_qp(32, 1000, 2000, 0.01, 0), {"QPDO_DENSE_LOWRANK": "1"}),
    "pcg_C1": (lambda: problems.config_qp("C1"), {"QPDO_LINSOLVE": "pcg"}),
    "band_2048": (lambda: problems.banded_qp(7, 2048, q_reg=0.01), {}),
    "host_setup_C1": (lambda: problems.config_qp("C1"), {"QPDO_SETUP_HOST": "1"}),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_update_equals_fresh_setup_on_every_route(route, gpu_required, monkeypatch):
    make, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = make()
    a, b = run_case(p, seed=100 + sorted(ROUTES).index(route))
    assert_twins(a, b, route)
    st = b[1]["stats"]
    if route == "fused_C3":
        assert st["linsolve"] == 2
    if route == "band_2048":
        assert st["linsolve"] == 3
    if route == "pcg_C1":
        assert st["linsolve"] == 0
    if route == "woodbury_1000":
        assert a[1]["stats"]["lowrank_solves"] == st["lowrank_solves"]


def test_woodbury_kept_factor_is_dropped(gpu_required, monkeypatch):
    """the old solve leaves a kept factor (and Woodbury slots): the update must not reuse it"""
    monkeypatch.setenv("QPDO_DENSE_LOWRANK", "1")
    p = problems.random_qp(33, 1000, 2000, 0.01, 0)
    w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
    r = solve(w)
    assert r["stats"]["factor_count"] > 0 and r["stats"]["lowrank_solves"] > 0, r["stats"]
    w.delete()
    a, b = run_case(p, seed=34)
    assert_twins(a, b, "woodbury")


@pytest.mark.parametrize("st,idt", [(-1, np.int32), (1, np.int64), (0, np.int32), (-1, np.int64), (1, np.int32), (0, np.int64)])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_storage_and_index_types(st, idt, fused, gpu_required, monkeypatch):
    monkeypatch.setenv("QPDO_SMALL_FUSED", fused)
    p = problems.config_qp("C3") if fused == "1" else problems.config_qp("C1")
    a, b = run_case(p, seed=40 + st, st=st, idt=idt)
    assert_twins(a, b, (st, idt, fused))


@pytest.mark.parametrize("scaling", [0, 10])
@pytest.mark.parametrize("which", ["Q", "A", "QA"])
def test_partial_updates_and_scaling(scaling, which, gpu_required):
    p = problems.config_qp("C1")
    a, b = run_case(p, seed=50, which=which, settings=dict(scaling=scaling))
    assert_twins(a, b, (scaling, which))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_settings_change_before_update(fused, gpu_required, monkeypatch):
    """update_settings raises scaling after setup: the update scales with the CURRENT settings, from scratch"""
    monkeypatch.setenv("QPDO_SMALL_FUSED", fused)
    p = problems.config_qp("C3")
    a, b = run_case(p, seed=60, settings=dict(scaling=2), settings_change=dict(scaling=10))
    assert_twins(a, b, fused)


@pytest.mark.parametrize("pre,post", [(shift_q, None), (shift_bounds, None), (None, post_q), (None, post_bounds), (shift_q, post_bounds)])
@pytest.mark.parametrize("route", ["fused_C3", "mid_C1"])
def test_update_q_and_bounds_around_the_call(pre, post, route, gpu_required, monkeypatch):
    make, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, b = run_case(make(), seed=70, pre=pre, post=post)
    assert_twins(a, b, route)


def test_cold_start_after_update(gpu_required):
    a, b = run_case(problems.config_qp("C1"), seed=80, warm=False)
    assert_twins(a, b, "cold")


@pytest.mark.parametrize("route", ["fused_C3", "mid_C1", "pcg_C1"])
def test_ten_consecutive_updates_sqp_loop(route, gpu_required, monkeypatch):
    """an SQP-like loop: 1 % perturbations of the values, warm start from the previous solution; every step equals its fresh twin
    (the maps are built once and reused)"""
    make, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = make()
    Qf, A = problems.full_Q(p), sp.csc_matrix(p["A"])
    w = solver.QPDO().setup(sp.tril(Qf).tocsc(), p["q"], A, p["l"], p["u"], verbose=0, max_iter=300)
    r = w.solve()
    rng = np.random.default_rng(90)
    for it in range(10):
        Qf = sp.csc_matrix(Qf, copy=True); s = 1.0 + 0.01 * rng.uniform(-1, 1, p["n"])
        cols = np.repeat(np.arange(p["n"]), np.diff(Qf.indptr)); Qf.data = Qf.data * s[Qf.indices] * s[cols]
        A = sp.csc_matrix(A, copy=True); A.data = A.data * (1.0 + 0.01 * rng.uniform(-1, 1, len(A.data)))
        w.update_matrices(Q=Qf, A=A)
        t = solver.QPDO().setup(sp.tril(Qf).tocsc(), p["q"], A, p["l"], p["u"], verbose=0, max_iter=300)
        outs = []
        for s_ in (w, t):
            prods = products(s_, p["n"], p["m"], seed=it)
            s_.warm_start(r["x"], r["y"])
            rr = s_.solve()
            outs.append((prods, rr, s_.trace()))
        t.delete()
        assert_twins(outs[0], outs[1], (route, it))
        r = outs[0][1]
    w.delete()


def test_fused_route_carries_the_oracles_bits_after_an_update(gpu_required):
    for p in (problems.config_qp("C3"), problems.infeasibility_kat("degenerate")):
        st = dict(verbose=0, max_iter=p.get("max_iter", 300))
        pn = new_problem(p, 100, zerosA=0)
        w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], **st)
        w.solve()
        w.update_matrices(Q=pn["Qfull"], A=pn["A"])
        r = solve(w)
        assert r["stats"]["linsolve"] == 2
        newp = dict(p, Q=sp.tril(pn["Qfull"]).tocsc(), Qstype=-1, A=pn["A"])
        ro, tro = oracle_run(newp, max_iter=st["max_iter"])
        assert_identical(r, ro, r["trace"], tro, "oracle")
        w.delete()


def test_generic_route_follows_the_oracle_after_an_update(gpu_required, monkeypatch):
    monkeypatch.setenv("QPDO_SMALL_FUSED", "0")
    p = problems.config_qp("C1")
    pn = new_problem(p, 110, zerosA=0, spread=0.1)      # (the oracle's tolerances are for well-scaled instances)
    w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
    w.solve()
    w.update_matrices(Q=pn["Qfull"], A=pn["A"])
    r = solve(w)
    newp = dict(p, Q=sp.tril(pn["Qfull"]).tocsc(), Qstype=-1, A=pn["A"])
    o = ob.OracleSolver(newp, ob.default_settings())
    ro = o.solve()
    tro = o.trace()
    o.close()
    w.delete()
    gi, oi = r["info"], ro["info"]
    assert (gi["status_val"], gi["iterations"], gi["oterations"]) == (oi["status_val"], oi["iterations"], oi["oterations"])
    assert_same_trace(r["trace"], tro)


def _cholmod(M, stype, idt=np.int32):
    keep = []
    return solver._sparse_view(M, stype, keep, idt), keep


@pytest.mark.parametrize("fused", ["1", "0"])
def test_refusals_leave_the_workspace_untouched(fused, gpu_required, monkeypatch):
    """each bad call returns nonzero with a message, and the following solve equals the solve with the bad call left out"""
    import ctypes as C
    monkeypatch.setenv("QPDO_SMALL_FUSED", fused)
    p = problems.config_qp("C3")
    Ql = sp.tril(problems.full_Q(p)).tocsc()
    A = sp.csc_matrix(p["A"]); A.sort_indices()
    moved = A.copy()
    j = int(np.flatnonzero(np.diff(moved.indptr) > 0)[0]); k = moved.indptr[j]      # first entry of a nonempty column: move its row index
    rows = set(moved.indices[moved.indptr[j]:moved.indptr[j + 1]].tolist())
    moved.indices[k] = next(r for r in range(p["m"]) if r not in rows)
    moved.has_sorted_indices = False; moved.sort_indices()
    fewer = A.copy(); fewer.data[:] = 1.0; fewer.data[0] = 0.0; fewer.eliminate_zeros()      # one entry less
    bad = [("dims", None, sp.csc_matrix((p["m"] + 1, p["n"]))),
           ("stype", (Ql, 1), None),
           ("count", None, fewer),
           ("moved", None, moved)]
    for name, qarg, aarg in bad:
        w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
        ref = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
        solve(w); solve(ref)
        qv = _cholmod(*qarg) if qarg else (None, None)
        av = _cholmod(aarg, 0) if aarg is not None else (None, None)
        rc = solver.lib().qpdo_amd_update_matrices(w._w, C.byref(qv[0]) if qv[0] is not None else None, C.byref(av[0]) if av[0] is not None else None)
        assert rc != 0, name
        assert solver.lib().qpdo_amd_last_error(), name
        ra, rb = solve(w), solve(ref)
        assert_identical(ra, rb, ra["trace"], rb["trace"], name)
        w.delete(); ref.delete()
    # in Python: an entry outside the pattern
    w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
    with pytest.raises(ValueError):
        w.update_matrices(A=moved)
    w.delete()


def test_subset_pattern_is_projected(gpu_required):
    """a matrix whose pattern is a subset of the setup's: the dropped entries are explicit zeros -- the same as passing them"""
    p = problems.config_qp("C1")
    A = sp.csc_matrix(p["A"]); A.sort_indices()
    An = rescale(A, 120, zeros=10)
    sub = An.copy(); sub.eliminate_zeros()
    assert sub.nnz < An.nnz
    outs = []
    for M in (An, sub):
        w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
        w.update_matrices(A=M)
        outs.append((products(w, p["n"], p["m"]), w.solve(), w.trace()))
        w.delete()
    assert_twins(outs[0], outs[1], "subset")


def test_row_partitioned_workspace_is_refused(gpu_required):
    code = """
import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from qpdo_amd import problems, solver
from test_gpu_small import assert_identical
assert solver.dist_config(0, 1, mode="rccl", force=True) == 0
p = problems.random_qp(61, 300, 600, 0.03, 0)
w = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], verbose=0)
def solve(w):
    r = w.solve(); r["trace"] = w.trace(); return r
r0 = solve(w)
try:
    w.update_matrices(A=p["A"] * 2.0)
    print("ACCEPTED")
except RuntimeError as e:
    assert "row-partitioned" in str(e), e
r1 = solve(w)
assert_identical(r1, r0, r1["trace"], r0["trace"], "dist")
print("REFUSED_OK")
""" % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "REFUSED_OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
