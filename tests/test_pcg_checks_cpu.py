"""The checks of tests/test_gpu_pcg_pieces.py have teeth, and their bounds hold for the reference alone: on the CPU, tests/pcg_ref.py's own
output passes every check; a compact matrix that lost a row of tiny weight, a renumbering that is off by one from a word boundary on, a
Jacobi diagonal without sigma and a p.Kp that misses one block's partial sum fail theirs -- the exact ones by inequality, the bounded ones
by an order of magnitude or more.  Also here: the fp64 reference CG's own residual ratios, which fix the constant c of the residual bound
(pcg_ref.C_RESID), the Schur preconditioner needing fewer outer steps than Jacobi on the test systems, and the argument checks of the
two entry points from a stand-alone C program (tests/pcg_probe_args_driver.c), plain and under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import pcg_ref as R
from qpdo_amd import _build


def _as_got(ix, arc, atc, slab=None):
    """the reference's structures in the shape the device's downloads have"""
    def mat(M):
        g = dict(M, nnz=len(M["ci"]), use_slab=0, nslabs=0, W=0, ci16=None, sp=None)
        if slab:
            nsl, W = slab
            c16, spt = R.slab_tables(M["rp"], M["ci"], nsl, W)
            g.update(use_slab=1, nslabs=nsl, W=W, ci16=c16, sp=spt)
        return g
    return dict(k=ix["k"], rowlist=ix["rows"], cidx=ix["cidx"], dc=ix["dc"], flag_bits=ix["flag_bits"], flag_wprefix=ix["flag_wprefix"],
                Arc=mat(arc) if ix["k"] else None, Atc=mat(atc) if ix["k"] else None)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1025])
def test_reference_index_space_is_consistent(m):
    Qf, A = R.system(200, m, 1, empty_row=m // 2)
    for name, dw in R.weight_patterns(m).items():
        ix, arc, atc = R.compact_matrices(A, dw)
        flag = np.array([not (v == 0.0) for v in dw])                # the kernels' test, one row at a time
        assert ix["k"] == int(flag.sum()) and np.array_equal(ix["rows"], np.flatnonzero(flag)), name
        for i in range(m):
            assert ix["cidx"][i] == int(flag[:i].sum())
            assert bool((int(ix["flag_bits"][i // 64]) >> (i % 64)) & 1) == bool(flag[i])
        assert all(ix["flag_wprefix"][w] == int(flag[:64 * w].sum()) for w in range((m + 63) // 64))
        # A_c' is the transpose of A_c, entry for entry
        if ix["k"]:
            Ac = sp.csr_matrix((arc["val"], arc["ci"], arc["rp"]), shape=(ix["k"], 200))
            Atc = sp.csr_matrix((atc["val"], atc["ci"], atc["rp"]), shape=(200, ix["k"]))
            assert (Ac.T != Atc).nnz == 0 and Atc.has_sorted_indices
        assert R.compaction_mismatch(_as_got(ix, arc, atc), ix, arc, atc) is None, name
    z = R.weight_patterns(m)["negative_zero"]
    assert np.any(np.signbit(z) & (z == 0)) or m < 3
    assert R.index_space(z)["k"] == int((z > 0).sum())
    assert R.index_space(R.weight_patterns(m)["subnormal"])["k"] >= 1


def test_slab_tables_match_a_searchsorted_per_row():
    Qf, A = R.system(700, 300, 2, per_row=9)
    ix, arc, atc = R.compact_matrices(A, R.weight_patterns(300)["random30"])
    W, nsl = 256, 3
    c16, spt = R.slab_tables(arc["rp"], arc["ci"], nsl, W)
    for r in range(arc["nrows"]):
        cols = arc["ci"][arc["rp"][r]:arc["rp"][r + 1]]
        assert np.array_equal(spt[r], np.concatenate([arc["rp"][r] + np.searchsorted(cols, W * np.arange(nsl)), [arc["rp"][r + 1]]]))
    assert np.array_equal(c16, arc["ci"] % W)
    assert R.compaction_mismatch(_as_got(ix, arc, atc, slab=(nsl, W)), ix, arc, atc) is None


def test_exact_checks_catch_a_dropped_row_of_tiny_weight():
    """the whole-solve tests cannot see this: the row's weight is 2^-30 of the largest"""
    m, n = 1025, 300
    Qf, A = R.system(n, m, 3)
    dw = R.weight_patterns(m)["random30"]
    dw[dw != 0] = 8.0
    victim = int(np.flatnonzero(dw)[7])
    dw[victim] = 8.0 * 2.0 ** -30
    ix, arc, atc = R.compact_matrices(A, dw)
    assert R.compaction_mismatch(_as_got(ix, arc, atc), ix, arc, atc) is None
    lost = dw.copy()
    lost[victim] = 0.0
    ixm, arcm, atcm = R.compact_matrices(A, lost)
    bad = R.compaction_mismatch(_as_got(ixm, arcm, atcm), ix, arc, atc)
    assert bad is not None and bad.startswith("k = ")
    # the same loss inside A_c' alone (k, the row list and A_c intact): the first differing array is named
    got = _as_got(ix, arc, atc)
    keep = atc["ci"] != ix["cidx"][victim]
    assert not keep.all()
    rows = np.repeat(np.arange(n), np.diff(atc["rp"]))
    got["Atc"] = dict(got["Atc"], ci=atc["ci"][keep], val=atc["val"][keep], nnz=int(keep.sum()),
                      rp=np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32))
    assert R.compaction_mismatch(got, ix, arc, atc).startswith("Atc geometry")
    # and what a whole solve would see of it: a relative change of K of 2^-30 at most
    p = R.probe_vectors(n)["random"]
    full, absvec, r = R.K_product(Qf, A, 1.0, dw, p)
    part, _, _ = R.K_product(Qf, A, 1.0, lost, p)
    assert 0 < float(np.abs(full - part).max() / np.abs(full).max()) < 1e-8
    # ... which the K product bound still catches, by orders of magnitude
    assert R.K_product_ratio(part.astype(np.float64), full, absvec, r) > 1e4


@pytest.mark.parametrize("word", [1, 9, 16])
def test_exact_checks_catch_a_renumbering_off_by_one_from_a_word_boundary(word):
    m, n = 1089, 300
    Qf, A = R.system(n, m, 4)
    dw = R.weight_patterns(m)["random30"]
    ix, arc, atc = R.compact_matrices(A, dw)
    got = _as_got(ix, arc, atc)
    # the LDS-table kernel renumbers through wprefix: a prefix that is one too large from word `word` on (a wave segment that was not counted)
    first = int(ix["flag_wprefix"][word])
    ci = atc["ci"].copy()
    ci[ci >= first] += 1
    assert not np.array_equal(ci, atc["ci"])
    got["Atc"] = dict(got["Atc"], ci=ci)
    bad = R.compaction_mismatch(got, ix, arc, atc)
    assert bad is not None and bad.startswith("Atc.ci["), bad
    got = _as_got(ix, arc, atc)
    wp = ix["flag_wprefix"].copy()
    wp[word:] += 1
    got["flag_wprefix"] = wp
    assert R.compaction_mismatch(got, ix, arc, atc).startswith("flag_wprefix[%d]" % word)


@pytest.mark.parametrize("pattern,sigma", [("random30", 1.0), ("all", 1.0), ("late_pass", 1e-7), ("subnormal", 1.0), ("none", 1.0)])
def test_K_product_bounds_hold_for_fp64_and_catch_a_missing_partial(pattern, sigma):
    n, m = 400, 1025
    Qf, A = R.system(n, m, 5, empty_row=m // 2)
    dw = R.weight_patterns(m)[pattern]
    K = R.K_sparse(Qf, A, sigma, dw)
    for vname, p in R.probe_vectors(n).items():
        ref, absvec, r = R.K_product(Qf, A, sigma, dw, p)
        Kp = K @ p                                                     # fp64, another summation order than the device's
        ratio = R.K_product_ratio(Kp, ref, absvec, r, R.underflow_term(A, r))
        assert ratio <= 1.0, (vname, ratio)
        parts = np.array([float(p[i:i + 256] @ Kp[i:i + 256]) for i in range(0, n, 256)])
        assert R.pKp_ratio(parts, p, ref, absvec, r) <= 1.0
        if vname == "random":
            assert R.pKp_ratio(parts[1:], p, ref, absvec, r) >= 10.0       # one block's partial sum missing
            assert R.pKp_ratio(parts[:-1], p, ref, absvec, r) >= 10.0
            bad = Kp.copy()
            j = int(np.argmax(np.abs(Kp)))
            bad[j] *= 1.0 + 1e-11                                       # far below what a whole solve notices
            assert R.K_product_ratio(bad, ref, absvec, r) >= 10.0


def test_diagonal_bounds_hold_for_fp64_and_catch_a_missing_sigma():
    n, m = 400, 1025
    Qf, A = R.system(n, m, 6)
    for pattern, sigma in (("random30", 1.0), ("all", 1.0), ("late_pass", 1e-7)):
        dw = R.weight_patterns(m)[pattern]
        ref, cnt = R.jacobi_diagonal(Qf, A, sigma, dw)
        Ac = sp.csc_matrix(A)
        fp64 = np.asarray(Qf.diagonal() + sigma + np.asarray(Ac.multiply(Ac).T @ dw).ravel(), np.float64)
        assert R.diagonal_ratio(fp64, ref, cnt) <= 1.0
        assert R.diagonal_ratio(fp64 - sigma, ref, cnt) >= 10.0, pattern            # the sigma term missing: 1e-7 of the diagonal at least
        dq, sd, lens = R.schur_diagonals(Qf, A, sigma, dw)
        rows = np.flatnonzero(dw)
        Ar = sp.csr_matrix(A)[rows]
        dq64 = Qf.diagonal() + sigma
        sd64 = 1.0 / dw[rows] + np.asarray(Ar.multiply(Ar) @ (1.0 / dq64)).ravel()
        assert R.diagonal_ratio(dq64, dq, np.zeros(n)) <= 1.0 and R.diagonal_ratio(sd64, sd, lens) <= 1.0
        assert R.diagonal_ratio(dq64 - sigma, dq, np.zeros(n)) >= 10.0
        assert R.diagonal_ratio(sd64 - 1.0 / dw[rows], sd, lens) >= 10.0             # the 1 / d term missing


REF_RATIOS = {}


@pytest.mark.parametrize("name", list(R.SOLVE_CASES))
def test_reference_cg_meets_the_residual_bound_with_half_of_c(name):
    Qf, A, sigma, dw, env, route = R.solve_case(name)
    knorm = R.norm2(R.K_sparse(Qf, A, sigma, dw))
    worst = -np.inf
    for rname, b in R.solve_rhs(Qf, A, sigma, dw).items():
        x, it = R.jacobi_pcg(Qf, A, sigma, dw, b)
        if rname == "zero":
            assert it == 0 and not x.any()
            continue
        assert 0 < it < 2000
        ratio = R.residual_ratio(Qf, A, sigma, dw, x, b, knorm)
        worst = max(worst, ratio)
        if route == "schur":
            xs, its = R.schur_pcg(Qf, A, sigma, dw, b)
            assert its < it, (rname, its, it)                  # the condition the device's outer-step count is held to is not vacuous
            worst = max(worst, R.residual_ratio(Qf, A, sigma, dw, xs, b, knorm))
    REF_RATIOS[name] = worst
    assert 2.0 * worst <= R.C_RESID, worst
    # a solve stopped one decade early misses the bound by far more than an order of magnitude
    b = R.solve_rhs(Qf, A, sigma, dw)["random"]
    x, _ = R.jacobi_pcg(Qf, A, sigma, dw, b, tol=1e-10)
    assert R.residual_ratio(Qf, A, sigma, dw, x, b, knorm) >= 10.0 * R.C_RESID


def test_reference_deflation_pieces():
    Qf, A, sigma, dw = R.deflation_case()
    ix = R.index_space(dw)
    thr = R.deflation_threshold(ix["dc"])
    heavy = np.flatnonzero(ix["dc"] > thr)
    assert thr == 1.0 and len(heavy) == 40
    light = np.where(dw > thr, 0.0, dw)
    P, _ = R.jacobi_diagonal(Qf, A, sigma, light)
    full, _ = R.jacobi_diagonal(Qf, A, sigma, dw)
    assert np.all(P > 1e-6 * full)                                  # the floor of k_jacobi_diag2 is not active on this system
    S = R.deflation_S(A, dw, ix["rows"], heavy, P)
    S64 = S.astype(np.float64)
    Sinv = np.linalg.inv(S64)
    kappa = np.linalg.cond(S64)
    assert np.abs(Sinv @ S64 - np.eye(40)).max() <= 1e-10 * kappa
    assert np.abs((Sinv * (1 + 1e-2)) @ S64 - np.eye(40)).max() > 10 * 1e-10 * kappa          # (kappa(S) = 3e5 here)
    x, it = R.jacobi_pcg(Qf, A, sigma, dw, R.solve_rhs(Qf, A, sigma, dw)["random"])
    knorm = R.norm2(R.K_sparse(Qf, A, sigma, dw))
    ratio = R.residual_ratio(Qf, A, sigma, dw, x, R.solve_rhs(Qf, A, sigma, dw)["random"], knorm)
    REF_RATIOS["deflation"] = ratio
    assert 2.0 * ratio <= R.C_RESID


def test_zz_report():
    print("\nreference CG residual ratios (c needed): " + ", ".join("%s %.3g" % kv for kv in sorted(REF_RATIOS.items())))


def _run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="pcg_probe_args_driver.c")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    if sanitize:
        supp = tmp_path / "lsan.supp"
        supp.write_text("leak:libhsa-runtime64\nleak:libamdhip64\nleak:librccl\n")
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
                   LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % supp)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    return out.returncode, out.stdout + out.stderr


def test_probe_argument_checks_from_a_c_caller(tmp_path):
    rc, txt = _run_driver(tmp_path, False)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]


def test_probe_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """the host driver (qpdo_api.c) and the C caller with -fsanitize=address,undefined, as a stand-alone program on the CPU"""
    rc, txt = _run_driver(tmp_path, True)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]
    assert "AddressSanitizer" not in txt and "runtime error" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
