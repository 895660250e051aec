"""The pair-wide slab products (k_spmv_slab with the fp32 operand: half-precision and fp32 values) on their pair-local index image.

The pair-wide instances gather xs[index] with the image's PAIR-LOCAL 16-bit indices (DevCsr::p16sm: the slab-local index of i16sm, plus W
for an entry of the odd slab of a pair), and the half-precision instance masks the OPERAND of an entry slot that does not count and adds
the slot with one fma.  The arithmetic itself is held by test_gpu_slab_trips (the emulated summation order, the recorded solves); its
helpers and its crafted matrix are used here.
1. the new image: p16sm == i16sm + W [the position belongs to the odd slab of a pair], rebuilt from the downloaded seg; five slabs (two
   pairs and a single one, which has no offset anywhere) and four, as A_c and as A_c'.
2. stale tail: on one workspace a pass that keeps most rows, then one that keeps about a third -- its images end inside the first's, with
   fewer and narrower slabs for A_c' (what lies behind them are the first pass's pair-local indices, up to 2 W_old).  The operand is NaN at
   every column that no kept row touches: the products are finite and equal the emulation of test_gpu_slab_trips bit for bit.
   (The crafted 4096-row matrix cannot lose rows: a compact matrix takes the slab kernel from 4096 rows on, and the narrow products need
   k <= n.  The matrix here is 12288 x 12288 under QPDO_SLAB_MAX_W=2560.)
3. masked and zero-valued slots: entries at the top of the scaled half range, in half's subnormal range and underflowing to 0 in half;
   Inf at one operand column and NaN at another.  Rows without an entry there equal the clean product bit for bit; rows with one -- an
   entry that underflowed to 0 included: 0 Inf and 0 NaN are NaN -- are not finite.
4. every product runs twice: same bits."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_slab_trips as S
from qpdo_amd import solver

pytestmark = pytest.mark.gpu

PAIRWIDE = ("f32_x32", "h16_x32")


def _workspace(A, q):
    m, n = A.shape
    return solver.QPDO().setup(sp.diags(q).tocsc(), np.zeros(n), A, -np.ones(m), np.ones(m), scaling=0, verbose=0)


# ---- 1. the image -----------------------------------------------------------------------------------------------------------------------
def _expected_pair_index(img, geo):
    """i16sm + W on the positions of the odd slabs' segments; the number of positions with an offset"""
    seg, W, nslabs = img["seg"].astype(np.int64), geo["W"], geo["nslabs"]
    want = img["idx"].astype(np.int64)
    odd = np.zeros(want.size, bool)
    for sl in range(1, nslabs, 2):
        assert (seg[:, sl, 0] == seg[:, sl - 1, 0] + seg[:, sl - 1, 1]).all()        # pair order: mid = the even segment's end
        L = seg[:, sl, 1]
        odd[np.repeat(seg[:, sl, 0], L) + np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)] = True
    return want + W * odd, odd


@pytest.mark.parametrize("orient", ["rows", "transposed"])
def test_pair_local_index_is_the_slab_local_index_plus_w_in_odd_slabs(orient, gpu_required, monkeypatch):
    S._env(monkeypatch, QPDO_SLAB_MAX_W=str(S.MAX_W))
    cols, W, nslabs = S.ORIENT[orient]
    C = S._crafted(cols, W)
    A = C if orient == "rows" else sp.csr_matrix(C.T)
    m, n = A.shape
    rng = np.random.default_rng(17 + m)
    q, dw, v = 1.0 + rng.random(n), 0.1 + rng.random(m), rng.standard_normal(n)
    ws = _workspace(A, q)
    try:
        ws.pcg_h16_product(dw, "Arc", v)                  # a pass: both compact matrices and their images
        geo = {name: ws.download_compact_matrix(name) for name in ("Arc", "Atc")}
        img = {name: ws.download_compact_image(name) for name in ("Arc", "Atc")}
        p16 = {name: ws.download_compact_pair_index(name) for name in ("Arc", "Atc")}
        ws.rebuild_compact_images()                       # the lazy builder writes the same image
        p16_lazy = {name: ws.download_compact_pair_index(name) for name in ("Arc", "Atc")}
    finally:
        ws.delete()
    name = "Arc" if orient == "rows" else "Atc"           # the compact matrix that is C
    assert (geo[name]["ncols"], geo[name]["W"], geo[name]["nslabs"]) == S.ORIENT[orient]
    counts = set()
    for nm in ("Arc", "Atc"):
        g, im = geo[nm], img[nm]
        assert g["use_slab"] == 1 and g["has_ci16"] == 1 and im is not None and p16[nm] is not None, nm
        assert 2 * g["W"] <= 65536 and im["idx"].dtype == np.uint16 and p16[nm].dtype == np.uint16
        want, odd = _expected_pair_index(im, g)
        assert 0 < odd.sum() < want.size and (im["idx"] < g["W"]).all()
        print("%s %s: %d slabs, W = %d, %d of %d entries in odd slabs" % (orient, nm, g["nslabs"], g["W"], odd.sum(), want.size))
        assert np.array_equal(p16[nm].astype(np.int64), want), nm
        assert np.array_equal(p16_lazy[nm], p16[nm]), nm
        if g["nslabs"] % 2:                               # the last single slab: no offset anywhere
            seg = im["seg"].astype(np.int64)
            L = seg[:, -1, 1]
            last = np.repeat(seg[:, -1, 0], L) + np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)
            assert last.size > 0 and np.array_equal(p16[nm][last], im["idx"][last])
        counts.add(g["nslabs"])
    if orient == "rows":
        assert counts == {4, 5}                           # A_c = C: five slabs; A_c' (6400 x 4096): four


# ---- 2. stale tail -------------------------------------------------------------------------------------------------------------------------
STALE_N, STALE_W = 12288, 2560


def _stale_kept(r):
    """the rows that the second pass keeps: 4305 of 12288"""
    return r % 20 < 7


def _stale_matrix():
    """12288 x 12288: every eighth row long (up to 639 entries: pair segments of up to three trips), the others 0 .. 12 entries (empty
    rows among them); every 512th column in every fifth row (long segments for the transposed product)"""
    if "stale" not in S._cache:
        n = STALE_N
        rng = np.random.default_rng(n)
        rows, cols = [], []
        for r in range(n):
            L = (r * 53) % 640 if r % 8 == 0 else r % 13
            step = 6 * int(rng.integers(1, n // 6)) + 1            # coprime to n = 2^12 * 3: L distinct columns
            c = (int(rng.integers(n)) + step * np.arange(L)) % n
            rows.append(np.full(L, r)); cols.append(c)
        for c in range(0, n, 512):
            rr = np.arange(c % 5, n, 5)
            rr = rr[rr % 13 != 0]                                  # (the empty rows stay empty)
            rows.append(rr); cols.append(np.full(rr.size, c))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        keep = ~((cols % 16 == 5) & _stale_kept(rows))              # columns that only rows outside the second pass touch
        rows, cols = rows[keep], cols[keep]
        A = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))       # (duplicates summed away)
        A.data = rng.standard_normal(A.nnz)
        A.sort_indices()
        S._cache["stale"] = A
    return S._cache["stale"]


def test_products_on_an_image_that_ends_inside_an_earlier_larger_one(gpu_required, monkeypatch):
    S._env(monkeypatch, QPDO_SLAB_MAX_W=str(STALE_W))
    A = _stale_matrix()
    n = STALE_N
    rng = np.random.default_rng(5)
    q, v = 1.0 + rng.random(n), rng.standard_normal(n)
    r = np.arange(n)
    dw_most = np.where(r % 10 != 3, 0.1 + rng.random(n), 0.0)
    dw_third = np.where(_stale_kept(r), 0.1 + rng.random(n), 0.0)
    kept = np.nonzero(dw_third)[0]
    Ak = A[kept]
    # the operands of the second pass: NaN at every column that no kept row touches (A_c), at every kept row without entries (A_c')
    vA = v.copy()
    vA[np.diff(Ak.tocsc().indptr) == 0] = np.nan
    vT = v.copy()
    vT[:kept.size][np.diff(Ak.indptr) == 0] = np.nan
    assert 0 < np.isnan(vA).sum() < n // 2 and 0 < np.isnan(vT[:kept.size]).sum() < kept.size // 2
    ws = _workspace(A, q)
    try:
        first = {}
        for inst in PAIRWIDE:
            for name in ("Arc", "Atc"):
                first[inst, name] = S._device_product(ws, inst, dw_most, name, v)
        geo1 = {name: ws.download_compact_matrix(name) for name in ("Arc", "Atc")}
        y, y2 = {}, {}
        for inst in PAIRWIDE:
            for name, x in (("Arc", vA), ("Atc", vT)):
                y[inst, name] = S._device_product(ws, inst, dw_third, name, x)
                y2[inst, name] = S._device_product(ws, inst, dw_third, name, x)
        geo = {name: ws.download_compact_matrix(name) for name in ("Arc", "Atc")}
        img = {name: ws.download_compact_image(name) for name in ("Arc", "Atc")}
    finally:
        ws.delete()
    for name in ("Arc", "Atc"):
        assert geo[name]["use_slab"] == 1 and geo1[name]["use_slab"] == 1
        assert geo[name]["nnz"] < geo1[name]["nnz"] // 2          # the second image ends inside the first
        print("%s: first pass %d slabs of %d, nnz %d; second %d slabs of %d, nnz %d" % (
            name, geo1[name]["nslabs"], geo1[name]["W"], geo1[name]["nnz"], geo[name]["nslabs"], geo[name]["W"], geo[name]["nnz"]))
    assert geo["Atc"]["nslabs"] < geo1["Atc"]["nslabs"] and geo["Atc"]["W"] < geo1["Atc"]["W"]      # stale indices of a wider slab
    assert geo["Arc"]["nrows"] == kept.size >= 4096
    for inst in PAIRWIDE:
        for name, x in (("Arc", vA), ("Atc", vT[:kept.size])):
            ref = S._emulated_product(inst, img[name], geo[name], np.r_[x, np.zeros(max(0, geo[name]["ncols"] - x.size))])
            got = y[inst, name]
            assert np.isfinite(got).all() and np.isfinite(first[inst, name]).all(), (inst, name)
            bad = np.nonzero(got != ref)[0]
            print("%s %s: %d rows, %d differ from the emulation" % (inst, name, got.size, bad.size))
            assert got.size == ref.size and bad.size == 0, (inst, name, bad[:8], got[bad[:8]], ref[bad[:8]])
            assert S._same_bits(got, y2[inst, name]), (inst, name)


# ---- 3. masked and zero-valued slots --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", PAIRWIDE)
def test_inf_and_nan_reach_the_rows_with_an_entry_even_one_that_underflowed(inst, gpu_required, monkeypatch):
    S._env(monkeypatch, QPDO_SLAB_MAX_W=str(S.MAX_W))
    C = S._crafted(S.COLS, S.MAX_W).copy()
    c_nan, c_inf = 777, 4 * S.MAX_W + 100                # first pair; the single last slab
    rng = np.random.default_rng(99)
    # max |a| = 4 = 2^2 exactly: the image's scale is 2^12 and 4 lands on 2^14, the bottom of [2^14, 2^15); 3.99 sits just under it.
    # a 2^-33: scaled 2^-21 |a|, in half's subnormal range (2^-24 .. 2^-14); a 2^-50: scaled 2^-38 |a| rounds to 0
    C.data = np.clip(C.data, -3.5, 3.5)
    coo = C.tocoo()
    pick = rng.random(coo.nnz)
    tiny = ((coo.col == c_inf) | (coo.col == c_nan)) & (coo.row % 2 == 0)        # half of the entries under Inf / NaN underflow to 0
    data = np.where(pick < 0.02, 4.0, np.where(pick < 0.04, 3.99, np.where(pick < 0.1, coo.data * 2.0 ** -33, coo.data)))
    data = np.where(tiny | ((pick > 0.1) & (pick < 0.16)), coo.data * 2.0 ** -50, data)
    C = sp.csr_matrix((data, (coo.row, coo.col)), shape=C.shape)
    C.sort_indices()
    assert np.abs(C.data).max() == 4.0 and (C.data != 0).all()
    m, n = C.shape
    q, dw, v = 1.0 + rng.random(n), 0.1 + rng.random(m), rng.standard_normal(n)
    vb = v.copy()
    vb[c_nan], vb[c_inf] = np.nan, np.inf
    ws = _workspace(C, q)
    try:
        clean, clean2 = S._device_product(ws, inst, dw, "Arc", v), S._device_product(ws, inst, dw, "Arc", v)
        y, y2 = S._device_product(ws, inst, dw, "Arc", vb), S._device_product(ws, inst, dw, "Arc", vb)
        img, geo = ws.download_compact_image("Arc"), ws.download_compact_matrix("Arc")
    finally:
        ws.delete()
    h = np.abs(img["vsm16"].astype(np.float64))
    assert img["h16_e"] == 12 and h.max() == 2.0 ** 14 and np.isfinite(h).all()
    assert ((h > 0) & (h < 2.0 ** -14)).any() and ((h == 0) & (img["vsm"] != 0)).any()        # subnormal halves; underflowed ones
    touched = np.asarray((C[:, [c_nan, c_inf]] != 0).sum(axis=1)).ravel() > 0
    under = np.asarray((abs(C[:, [c_nan, c_inf]]) > 2.0 ** -40).sum(axis=1)).ravel() == 0     # ... whose entries there are all tiny
    assert 0 < touched.sum() < m and (touched & under).any() and (touched & ~under).any()
    assert np.isfinite(clean).all() and S._same_bits(clean, clean2) and S._same_bits(y, y2)
    ref = S._emulated_product(inst, img, geo, v)
    assert np.array_equal(clean, ref)
    assert S._same_bits(y[~touched], clean[~touched])
    assert not np.isfinite(y[touched]).any()
