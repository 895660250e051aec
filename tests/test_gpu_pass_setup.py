"""The per-pass set-up of the PCG path with its two switches on (the default) against the former sequences, bit for bit:
QPDO_COMPACT_ONE_READ (A_c's CSR copy, slab image and Schur diagonal from one read of the weighted rows, instead of k_copy_rows,
k_build_slab_ptr, k_slab_permute and k_schur_diag), QPDO_COMPACT_T_ONE_READ (A_c': slab pointers from the counting pass, CSR and image
from one compaction, instead of k_count_flagged_bits, k_compact_rows_bits, k_build_slab_ptr and k_slab_permute).  Nothing moves an
operation of a floating-point sum, so every array that qpdo_amd_download_compact hands out -- the slab-major images
included (which >= 64) --, K v, whole linear solves and whole QP solves must come out the same to the bit.  A further check rebuilds
each image by the lazy path (slab_major_build) and finds it unchanged: CSR, sp, seg and image are consistent after a build.
Every integer scan of a pass (flag words, row pointers, the linesearch sort's histograms) is the one device-wide scan, dev_scan; its
results are compared with NumPy: the index space and the compact matrices with tests/pcg_ref.py, the sorted order with a stable argsort.
The whole file runs in about 12 s on the MI355X."""
import numpy as np
import pytest
import scipy.sparse as sp

import pcg_ref as R
from oracle import binding as ob
from qpdo_amd import problems, solver

pytestmark = pytest.mark.gpu

SWITCHES = ("QPDO_COMPACT_ONE_READ", "QPDO_COMPACT_T_ONE_READ")
VECS = ("rowlist", "cidx", "dc", "flag_bits", "flag_wprefix")
INFO_KEYS = ("status_val", "iterations", "oterations", "objective", "res_prim_norm", "res_dual_norm")


def _system(n, m, k, seed):
    """A with ~60 entries per row (64 lanes per row), m no multiple of 64, and k weights.  Weighted: rows without entries, rows whose
    entries lie in columns < 400 only (first slab), the last row m - 1.  Column 1 of A has entries in unweighted rows only (a row of A'
    without a kept entry), column 2 none at all."""
    rng = np.random.default_rng(seed)
    per = 60 if n >= 60 else n
    rows = np.repeat(np.arange(m), per)
    cols = rng.integers(0, n, m * per)
    order = rng.permutation(m)
    weighted, rest = order[:k], order[k:]
    if k < m and m - 1 not in weighted and k > 0:          # the last weighted row is m - 1
        j = np.where(rest == m - 1)[0][0]
        weighted[0], rest[j] = rest[j], weighted[0]
    special = weighted[1:1 + min(8, max(0, k - 1))]
    empty, first = special[:len(special) // 2], special[len(special) // 2:]
    keep = ~np.isin(rows, empty)
    narrow = np.isin(rows, first)
    cols[narrow] = rng.integers(0, min(n, 400), narrow.sum())
    is_w = np.zeros(m, bool); is_w[weighted] = True
    keep &= ~((cols == 1) & is_w[rows]) & (cols != 2)
    if len(rest):
        rows = np.concatenate([rows, rest[:1]]); cols = np.concatenate([cols, [1]]); keep = np.concatenate([keep, [True]])
    A = sp.csr_matrix((rng.standard_normal(keep.sum()), (rows[keep], cols[keep])), shape=(m, n))
    A.sum_duplicates(); A.sort_indices()
    dw = np.zeros(m)
    dw[weighted] = 0.1 + 9.9 * rng.random(k)
    return R.dominant_Q(rng, n), A, dw, dict(empty=empty, first=first)


def _workspace(monkeypatch, Qf, A, on, idx16):
    """on: "0" / "1" for both switches, or the name of the one switch that is on"""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_SPMV", "slab")
    monkeypatch.setenv("QPDO_IDX16", idx16)
    for s in SWITCHES:
        monkeypatch.setenv(s, on if on in ("0", "1") else ("1" if s == on else "0"))
    n, m = Qf.shape[0], A.shape[0]
    ws = solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
    assert ws.stats()["linsolve"] == 0
    return ws


def _everything(ws):
    got = {name: ws.download_compact_vector(name) for name in VECS}
    for name in ("Arc", "Atc"):
        got[name] = ws.download_compact_matrix(name)
        got[name + "_image"] = ws.download_compact_image(name)
    return got


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                                          b.view(np.uint64) if b.dtype == np.float64 else b)
    return a == b


def _first_difference(a, b):
    for k in a:
        if not _same(a[k], b[k]):
            if isinstance(a[k], dict):
                return k, [q for q in a[k] if not _same(a[k][q], b[k][q])]
            return k
    return None


def _image_from_csr(mat, img):
    """the image that slab_major_build defines, from the downloaded CSR, sp and seg"""
    nslabs, W = mat["nslabs"], mat["W"]
    vsm = np.zeros(mat["nnz"]); idx = np.zeros(mat["nnz"], img["idx"].dtype)
    spt, seg = mat["sp"], img["seg"]
    for s in range(nslabs):
        ln = seg[:, s, 1].astype(np.int64)
        assert np.array_equal(ln, spt[:, s + 1] - spt[:, s])
        src = np.repeat(spt[:, s].astype(np.int64) - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(ln.sum())
        dst = np.repeat(seg[:, s, 0].astype(np.int64) - np.concatenate([[0], np.cumsum(ln)[:-1]]), ln) + np.arange(ln.sum())
        vsm[dst] = mat["val"][src]
        idx[dst] = mat["ci"][src] - s * W
    return vsm, idx


def _probe(monkeypatch, Qf, A, dw, sigma, v, on, idx16, schur):
    """one workspace: a mode-0 probe and everything it left; with the A_c switch on, the lazy rebuild of the images; with schur, one
    linear solve, which must take its diagonal from the build exactly when the A_c switch is on"""
    ws = _workspace(monkeypatch, Qf, A, on, idx16)
    try:
        Kv, info = ws.pcg_K_product(dw, sigma, v)
        got = _everything(ws)
        got["Kv"], got["partials"], got["kact"] = Kv, info["partials"], info["kact"]
        if on != "0":
            # the lazy path: images marked stale, one product each; slab_major_build must reproduce what the build wrote
            ws.rebuild_compact_images()
            for name in ("Arc", "Atc"):
                again = ws.download_compact_image(name)
                assert _same(again, got[name + "_image"]), (name, "lazy rebuild")
        if schur:
            x, sinfo = ws.pcg_solve(dw, sigma, v)
            assert sinfo["schur"] and sinfo["inner_steps"] > 0
            assert sinfo["diag_from_build"] == (on in ("1", "QPDO_COMPACT_ONE_READ")), on
            got["x"], got["solve"] = x, {q: sinfo[q] for q in ("iters", "outer", "inner_solves", "inner_steps", "rnorm", "bnorm")}
            got["s_diag"] = ws.download_compact_vector("s_diag")
            got["after_solve"] = _everything(ws)
    finally:
        ws.delete()
    return got


# n, m, k, A_c on the slab kernel (k >= 4096), A_c' on it (k >= 1024), slabs of A_c, of A_c'
SHAPES = [(3000, 9000, 4500, 1, 1, 1, 1), (30000, 52000, 22000, 1, 1, 2, 2), (3000, 9000, 2000, 0, 1, 0, 1), (3000, 9000, 700, 0, 0, 0, 0),
          (300, 600, 1, 0, 0, 0, 0), (300, 600, 600, 0, 0, 0, 0)]


@pytest.mark.parametrize("idx16", ["1", "0"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-m%d-k%d" % s[:3])
def test_set_up_matches_former_sequence_bitwise(shape, idx16, gpu_required, monkeypatch):
    n, m, k, slab_r, slab_t, ns_r, ns_t = shape
    Qf, A, dw, rows = _system(n, m, k, 11 + n + k)
    assert m % 64 and (k == m or k == 1 or dw[m - 1] != 0.0)
    v = np.random.default_rng(5).standard_normal(n)
    sigma = 0.37
    schur = k >= 4096 and k <= 0.8 * n                       # a linear solve as well: the Schur diagonal that the one read leaves
    res = {on: _probe(monkeypatch, Qf, A, dw, sigma, v, on, idx16, schur) for on in ("0", "1")}
    off, on = res["0"], res["1"]
    assert on["kact"] == k
    assert _first_difference(off, on) is None, _first_difference(off, on)
    # the index space (flag words, their scan) and both compact matrices (row-pointer scans of up to 15 tiles) against NumPy
    ix, ref_arc, ref_atc = R.compact_matrices(A, dw)
    bad = R.compaction_mismatch(dict(on, k=on["kact"]), ix, ref_arc, ref_atc)
    assert bad is None, bad
    # the cases are what the table says, and the inputs hold what they should
    arc, atc = on["Arc"], on["Atc"]
    assert (arc["use_slab"], atc["use_slab"], arc["nslabs"], atc["nslabs"]) == (slab_r, slab_t, ns_r, ns_t)
    cidx = on["cidx"]
    if k > 8:
        for r in rows["empty"]:
            assert arc["rp"][cidx[r]] == arc["rp"][cidx[r] + 1]
        for r in rows["first"]:
            j = cidx[r]
            assert arc["rp"][j + 1] > arc["rp"][j] and arc["ci"][arc["rp"][j + 1] - 1] < 400
        assert atc["rp"][1] == atc["rp"][2] == atc["rp"][3] < atc["rp"][-1] and (k == m or A[:, 1].nnz > 0)
        assert on["rowlist"][-1] == m - 1
    # an independent reading of the image: each (row, slab) segment of the CSR sits at seg's place
    for name in ("Arc", "Atc"):
        img, mat = on[name + "_image"], on[name]
        if img is None:
            continue
        assert np.any(img["seg"][:, :, 0] % 2 == 1)          # odd segment starts
        vsm, idx = _image_from_csr(mat, img)
        assert np.array_equal(vsm.view(np.uint64), img["vsm"].view(np.uint64)) and np.array_equal(idx, img["idx"]), name
    if arc["use_slab"] and ns_r > 1:
        j = cidx[rows["first"][0]]
        assert arc["sp"][j, 1] == arc["rp"][j + 1]            # nothing beyond the first slab


@pytest.fixture(scope="module")
def two_slab_system():
    n, m, k = SHAPES[1][:3]
    return _system(n, m, k, 11 + n + k)


def test_each_switch_alone_bitwise(two_slab_system, gpu_required, monkeypatch):
    """the mixed states: each switch on by itself (the other off) against both off, at the shape where both matrices take the slab
    kernel with two slabs and the linear solve runs in the Schur mode"""
    Qf, A, dw, _ = two_slab_system
    v = np.random.default_rng(5).standard_normal(Qf.shape[0])
    off = _probe(monkeypatch, Qf, A, dw, 0.37, v, "0", "1", True)
    for switch in SWITCHES:
        one = _probe(monkeypatch, Qf, A, dw, 0.37, v, switch, "1", True)
        assert _first_difference(off, one) is None, (switch, _first_difference(off, one))


def _solve(p, monkeypatch, on):
    for s in SWITCHES:
        monkeypatch.setenv(s, on)
    return solver.solve_problem(p, verbose=0)


def _assert_same_solve(r0, r1):
    for q in INFO_KEYS:
        assert r0["info"][q] == r1["info"][q], q
    assert r0["stats"]["lin_iters"] == r1["stats"]["lin_iters"]
    assert np.array_equal(r0["x"].view(np.uint64), r1["x"].view(np.uint64)) and np.array_equal(r0["y"].view(np.uint64), r1["y"].view(np.uint64))


@pytest.mark.parametrize("args", [(8200, 3000, 16000, 0.004, 0), (0, 6400, 20000, 0.003, 0)], ids=["n3000", "n6400"])
def test_schur_mode_solve_bitwise(args, gpu_required, monkeypatch):
    """whole solves in the Schur mode with the slab kernels, every switch off against every switch on.  n = 3000: A_c' on the slab
    kernel, A_c on the plain one; 2 m = 32000 breakpoints take the radix sort in every Newton step.  n = 6400: passes with
    4096 <= k <= 0.8 n have A_c on the slab kernel too (16 lanes per row: k_schur_diag stays)."""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")
    monkeypatch.setenv("QPDO_PCG_SCHUR", "1")
    monkeypatch.setenv("QPDO_SPMV", "slab")
    p = problems.random_qp(*args)
    assert 2 * p["m"] > 8192
    on = _solve(p, monkeypatch, "1")
    assert on["stats"]["schur_passes"] > 0 and on["info"]["iterations"] > 3
    _assert_same_solve(_solve(p, monkeypatch, "0"), on)


@pytest.mark.parametrize("m", [8000, 10001, 16000])
def test_linesearch_sort_bitwise(m, gpu_required, monkeypatch):
    """the radix path of the linesearch on its own (2 m > 8192 breakpoints; ties and non-candidates in the input): the sorted order is
    the stable order of numpy, exactly, and tau is the oracle's.  The digit histograms have 256 entries per 2048 breakpoints and are
    scanned in 2048-entry tiles: m = 8000 gives exactly one tile (the single launch), 10001 a ragged second one, 16000 exactly two."""
    monkeypatch.setenv("QPDO_LINSOLVE", "pcg")                # (the order is read through qpdo_amd_download_compact)
    assert 2 * m > 8192 and 256 * -(-2 * m // 2048) == {8000: 2048, 10001: 2560, 16000: 4096}[m]
    rng = np.random.default_rng(9)
    p = problems.random_qp(1, 4, m, 0.5)
    delta = rng.standard_normal(2 * m); alpha = rng.standard_normal(2 * m) * np.abs(delta)
    alpha[::7] = delta[::7]                                   # ties at t = 1
    delta[5::11] = np.abs(delta[5::11]); alpha[5::11] = -np.abs(alpha[5::11])      # t < 0: not candidates
    t = alpha / delta
    ref_order = np.argsort(np.where(t > 0, t, np.inf), kind="stable")
    ref_tau = ob.pwa_linesearch(3.0, -2.0, delta, alpha)
    s = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, verbose=0, scaling=0)
    try:
        tau = s.linesearch(3.0, -2.0, delta, alpha)
        order = s.download_linesearch_order()
    finally:
        s.delete()
    print("m = %d: tau %.17g, oracle %.17g" % (m, tau, ref_tau))
    assert np.array_equal(order, ref_order) and np.sum(t > 0) > 8192
    assert np.isfinite(tau) and abs(tau - ref_tau) <= 1e-10 * max(1.0, abs(ref_tau))
