"""The fp32 inner CG of the Schur mode with fp32 OPERAND vectors (QPDO_INNER_X32, the default): the two products stage fp32 copies of
u and t, so one LDS fill holds the x slices of two column slabs and k_spmv_slab walks slab PAIRS; the images of the compact matrices
keep the two segments of a row in a pair adjacent (pair order, k_slab_seg).

(a) The pair-wide instance on its own (qpdo_amd_pcg_probe modes 34 / 35) on the three shapes of test_gpu_inner_refine.SHAPES -- 1 slab,
2 slabs, 6 / 5 slabs, so a single slab alone, one whole pair, and an odd count that leaves a single last slab behind whole pairs -- and
on a small matrix under QPDO_SLAB_MAX_W=1280 (5 and 4 slabs at n = 6400).  Reference: numpy in longdouble with the values AND x rounded
to float32; bound |y - y_ref| <= 1e-13 (|M32| |x32|) componentwise.  A float times a float is exact in double, so the only rounding is
that of the fp64 row sums: (row length + 1) 2^-53 (|M32| |x32|) = 8e-14 for the longest row here (700 entries) -- the bound of
test_gpu_inner_refine carries over.  The same product with x NOT rounded is outside the bound on more than half the rows (x32 is 6e-8
away from x), so the check tells the operand widths apart.  (b) The image: seg[:, 2S + 1, 0] == seg[:, 2S, 0] + seg[:, 2S, 1].
(c) Whole solves of the n6400 problem of test_gpu_inner_refine, slab kernels forced, plain and with QPDO_SLAB_MAX_W=1280: the default
against QPDO_INNER_X32=0 and against the oracle's recorded solve; fold on / off and repeats bit for bit."""
import os

import numpy as np
import pytest

import pcg_ref as R
import test_gpu_inner_refine as T
from helpers import ITERATE_RTOL_PCG, close_vec
from qpdo_amd import solver

pytestmark = pytest.mark.gpu

X32_ENV = ("QPDO_INNER_X32", "QPDO_SLAB_MAX_W")
_probe_cache = {}


def _env(monkeypatch, **env):
    for k in X32_ENV:
        monkeypatch.delenv(k, raising=False)
    T._slab_env(monkeypatch, **env)


def _ref_product_x32(M, x):
    """(M32 x32, |M32| |x32|, M32 x) from a downloaded compact matrix, in longdouble"""
    rp, ci = M["rp"].astype(np.int64), M["ci"]
    row_of = np.repeat(np.arange(M["nrows"]), np.diff(rp))
    v32 = M["val"].astype(np.float32).astype(np.longdouble)
    x32 = x.astype(np.float32).astype(np.longdouble)[ci]
    y, ab, yx64 = (np.zeros(M["nrows"], np.longdouble) for _ in range(3))
    np.add.at(y, row_of, v32 * x32)
    np.add.at(ab, row_of, np.abs(v32 * x32))
    np.add.at(yx64, row_of, v32 * x.astype(np.longdouble)[ci])
    return y, ab, yx64


def _probe(ws, dw, v):
    """both pair-wide products (twice each), the compact matrices and their images, from one workspace"""
    out = {}
    for name in ("Arc", "Atc"):
        y, kk = ws.pcg_f32_product(dw, name, v, x32=True)
        M = ws.download_compact_matrix(name)
        img = ws.download_compact_image(name)
        y2, _ = ws.pcg_f32_product(dw, name, v, x32=True)
        ys, _ = ws.pcg_f32_product(dw, name, v)                    # slab by slab, fp64 operand: modes 32 / 33 on the same image
        out[name] = dict(y=y, y2=y2, ys=ys, k=kk, M=M, seg=img["seg"])
    return out


def _shape_probe(shape):
    if shape not in _probe_cache:
        n, m, k, _, _, _ = T.SHAPES[shape]
        rng = np.random.default_rng(n + 3 * m)
        A = T._matrix(rng, m, n, long_rows=((3, 300), (k // 2, 700)), long_cols=((5, 300), (n // 2, 700)), empty_rows=(7, k - 1), empty_cols=(11, n - 1))
        Qf = R.dominant_Q(rng, n)
        dw = np.zeros(m)
        dw[:k] = 0.1 + rng.random(k)
        v = rng.standard_normal(n)
        ws = solver.QPDO().setup(Qf, np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)
        try:
            _probe_cache[shape] = (_probe(ws, dw, v), v)
        finally:
            ws.delete()
    return _probe_cache[shape]


def _check_products(tag, res, v, k, slabs, cases=True):
    """the checks of (a) on both products of one probe; returns the longest pair segment per matrix.  cases: the matrix was built to hold
    empty rows and every kind of pair (the shapes of SHAPES), and must"""
    longest = {}
    for name in ("Arc", "Atc"):
        p = res[name]
        M, y = p["M"], p["y"]
        nslabs = M["nslabs"]
        assert p["k"] == k and M["use_slab"] == 1 and M["has_ci16"] == 1
        assert nslabs == slabs[name], (name, nslabs)
        seglen = np.diff(M["sp"].astype(np.int64), axis=1)
        assert not cases or (np.diff(M["rp"]) == 0).any()                    # empty rows
        npairs = nslabs // 2
        if npairs:
            a, b = seglen[:, 0:2 * npairs:2], seglen[:, 1:2 * npairs:2]
            # a pair with an empty first half, an empty second half, both empty, neither
            assert not cases or (((a == 0) & (b > 0)).any() and ((a > 0) & (b == 0)).any() and ((a == 0) & (b == 0)).any() and ((a > 0) & (b > 0)).any())
            pairlen = (a + b).max()
        else:
            pairlen = seglen.max()
        if nslabs % 2:
            assert (seglen[:, -1] > 0).any() and (not cases or (seglen[:, -1] == 0).any())   # the single last slab: a pair with an empty second half
        yr, ab, yx64 = _ref_product_x32(M, v[:M["ncols"]])
        err = np.abs(y.astype(np.longdouble) - yr)
        bound = 1e-13 * ab
        worst = float((err / np.where(ab > 0, bound, 1)).max())
        print("%s %s: k = %d, %d slabs, longest pair segment %d, worst |y - y_ref| / (1e-13 |M32||x32|) = %.3g" % (tag, name, k, nslabs, pairlen, worst))
        assert (err <= bound).all(), (name, worst)
        assert (np.abs(yx64 - yr) > bound).sum() > M["nrows"] // 2          # the unrounded operand is far outside
        assert (np.abs(p["ys"].astype(np.longdouble) - yr) > bound).sum() > M["nrows"] // 2      # and so is the instance that stages it
        assert np.array_equal(p["y2"].view(np.uint64), y.view(np.uint64))
        longest[name] = pairlen
    return longest


# ---- (a) the products ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(T.SHAPES))
def test_pair_wide_products_against_rounded_numpy(shape, gpu_required, monkeypatch):
    n, m, k, slabs_r, slabs_t, _ = T.SHAPES[shape]
    _env(monkeypatch)
    res, v = _shape_probe(shape)
    for name, pairlen in _check_products(shape, res, v, k, dict(Arc=slabs_r, Atc=slabs_t)).items():
        if shape != "six_slabs":
            assert pairlen > 512, (name, pairlen)             # a pair segment longer than two trips of a lane group (256 entries each): a ragged third one


def test_pair_wide_products_with_capped_slab_width(gpu_required, monkeypatch):
    """QPDO_SLAB_MAX_W=1280 at n = 6400: 5 slabs for A_c (two pairs and a single slab), 4 for A_c' -- the geometry of the capped solves of (c)"""
    _env(monkeypatch, QPDO_SLAB_MAX_W="1280")
    p = T._problem("n6400")
    n, m, k = p["n"], p["m"], 5000
    rng = np.random.default_rng(6400)
    dw = np.zeros(m)
    dw[:k] = 0.1 + rng.random(k)
    v = rng.standard_normal(n)
    ws = solver.QPDO().setup(p["Q"], p["q"], p["A"], p["l"], p["u"], Qstype=-1, scaling=0, verbose=0)
    try:
        res = _probe(ws, dw, v)
    finally:
        ws.delete()
    _check_products("capped", res, v, k, dict(Arc=5, Atc=4), cases=False)      # (a generated QP: no empty rows)
    assert res["Arc"]["M"]["W"] == 1280 and res["Atc"]["M"]["W"] <= 1280


# ---- (b) the image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(T.SHAPES))
def test_pair_order_keeps_the_segments_of_a_pair_adjacent(shape, gpu_required, monkeypatch):
    _env(monkeypatch)
    res, _ = _shape_probe(shape)
    for name in ("Arc", "Atc"):
        seg = res[name]["seg"].astype(np.int64)
        nslabs = seg.shape[1]
        for S in range(nslabs // 2):
            assert np.array_equal(seg[:, 2 * S + 1, 0], seg[:, 2 * S, 0] + seg[:, 2 * S, 1]), (name, S)
        # the segments tile the image: every entry belongs to exactly one
        assert seg[:, :, 1].sum() == res[name]["M"]["nnz"]


# ---- (c) whole solves ----------------------------------------------------------------------------------------------------------------
def _oracle_n6400():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_random_qp_0_6400_20000.npz"))
    return dict(info={k: int(z[k]) for k in T.INFO_KEYS}, x=z["x"], y=z["y"])


@pytest.mark.parametrize("cap", ["plain", "max_w_1280"])
def test_x32_solve_matches_fp64_operands_and_oracle(cap, gpu_required, monkeypatch):
    env = {} if cap == "plain" else {"QPDO_SLAB_MAX_W": "1280"}
    _env(monkeypatch)
    r1 = T._solve("n6400", monkeypatch, **env)
    r0 = T._solve("n6400", monkeypatch, QPDO_INNER_X32="0", **env)
    st, st0 = r1["stats"], r0["stats"]
    print(cap, {k: st[k] for k in st if k.startswith("inner_")}, "x64:", {k: st0[k] for k in st0 if k.startswith("inner_")})
    for r in (r1, r0):
        T._assert_accepted(r["stats"])
        assert r["stats"]["inner_refine_fallbacks"] == 0 and r["stats"]["inner_refine_sweeps"] >= 1
    assert 0 < st["inner_x32_steps"] <= st["inner_steps"] and st0["inner_x32_steps"] == 0
    T._assert_same_outcome(r1, r0)
    ro = _oracle_n6400()
    for r in (r1, r0):              # (the capped run with QPDO_INNER_X32=0 checks the cap alone)
        for k in T.INFO_KEYS:
            assert r["info"][k] == ro["info"][k], k
        assert close_vec(r["x"], ro["x"], ITERATE_RTOL_PCG) and close_vec(r["y"], ro["y"], ITERATE_RTOL_PCG)


@pytest.mark.parametrize("cap", ["plain", "max_w_1280"])
def test_x32_fold_on_and_off_and_repeats_are_bitwise(cap, gpu_required, monkeypatch):
    env = {} if cap == "plain" else {"QPDO_SLAB_MAX_W": "1280"}
    _env(monkeypatch)
    a = T._solve("n6400", monkeypatch, **env)
    b = T._solve("n6400", monkeypatch, QPDO_INNER_FOLD="0", **env)
    _env(monkeypatch, **env)
    c = solver.solve_problem(T._problem("n6400"), verbose=0)                  # (not from the cache: a second run)
    assert a["stats"]["inner_x32_steps"] > 0
    for r in (b, c):
        for k in T.INFO_KEYS + ("objective", "res_prim_norm", "res_dual_norm"):
            assert r["info"][k] == a["info"][k], k
        for k in ("lin_iters", "inner_steps", "inner_x32_steps", "inner_solves", "inner_refine_sweeps", "inner_refine_fallbacks", "inner_refine_max_res_over_tol"):
            assert r["stats"][k] == a["stats"][k], k
        assert np.array_equal(r["x"], a["x"]) and np.array_equal(r["y"], a["y"])
