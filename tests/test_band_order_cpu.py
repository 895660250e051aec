"""The band solver's variable order (qpdo_amd/csrc/band_order.c) on its own, on the CPU: a stand-alone C program (tests/band_order_driver.c)
links only that translation unit -- no device library, no HIP -- reads the patterns from a file and writes the orders back; the same program
runs a second time under AddressSanitizer + UBSan.

Quality is measured against scipy.sparse.csgraph.reverse_cuthill_mckee on the explicitly formed graph of Q + A'A.  The C code never forms
A'A; it uses exact degrees, as scipy does.  Over the family below -- banded_random_qp(7, n, bw) for (64, 3), (260, 4), (520, 16), (1040, 31),
(2100, 63), (1100, 130) and banded_qp(1, 4096), each relabelled even/odd and at random -- scipy gives 3, 4, 18, 41, 83-84, 190 and 1; this
implementation 3, 4, 18, 41, 83, 190 and 1.  The largest ratio b_ordered / b_scipy, measured on the CPU, is 1.000 (the smallest 83 / 84):
QUALITY_PIN is that rounded up to the next 0.05.  The heuristic is deterministic, so the pin is a regression pin, not a noise allowance.
(With the O(nnz) degree bound instead of exact degrees the same code gave 21, 47-48, 94 and 204: ratio 1.17.)"""
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import reverse_cuthill_mckee

from qpdo_amd import _build, problems

QUALITY_PIN = 1.00
FAMILY = ((64, 3), (260, 4), (520, 16), (1040, 31), (2100, 63), (1100, 130))
NARROW = ("bw3", "bw4", "chain4096")          # come back at their original half-bandwidth


def even_odd(n):
    return np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])


def pattern(prob):
    return dict(n=prob["n"], m=prob["m"], stype=prob.get("Qstype", -1), Q=prob["Q"].tocsc(), A=prob["A"].tocsc())


def custom(n, q_entries, rows, stype=-1):
    """a pattern from lists: q_entries (i, j) as stored, rows = the column lists of A"""
    qi, qj = (np.array([e[0] for e in q_entries], dtype=np.int64), np.array([e[1] for e in q_entries], dtype=np.int64)) if q_entries else (np.zeros(0, np.int64),) * 2
    Q = sp.csc_matrix((np.ones(len(qi)), (qi, qj)), shape=(n, n))
    ar = np.concatenate([np.full(len(c), r, dtype=np.int64) for r, c in enumerate(rows)]) if rows else np.zeros(0, np.int64)
    ac = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows]) if rows else np.zeros(0, np.int64)
    A = sp.csc_matrix((np.ones(len(ar)), (ar, ac)), shape=(len(rows), n))
    Q.sort_indices(); A.sort_indices()
    return dict(n=n, m=len(rows), stype=stype, Q=Q, A=A)


def cases():
    out = {}
    for n, bw in FAMILY:
        p = problems.banded_random_qp(7, n, bw)
        out["bw%d even/odd" % bw] = (pattern(problems.permute_variables(p, even_odd(n))), bw)
        out["bw%d random" % bw] = (pattern(problems.permute_variables(p, np.random.default_rng(n).permutation(n))), bw)
    p = problems.banded_qp(1, 4096)
    out["chain4096 even/odd"] = (pattern(problems.permute_variables(p, even_odd(4096))), 1)
    out["chain4096 random"] = (pattern(problems.permute_variables(p, np.random.default_rng(4096).permutation(4096))), 1)
    out["chain4096 natural"] = (pattern(p), 1)                                   # already optimal: b_ordered == b_natural
    # two chains that share nothing, interleaved: 0-2-4-... through Q, 1-3-5-... through rows of A
    n = 40
    out["two chains"] = (custom(n, [(i + 2, i) for i in range(0, n - 2, 2)] + [(i, i) for i in range(n)], [[i, i + 2] for i in range(1, n - 2, 2)]), None)
    # variable 7 appears nowhere (not even on Q's diagonal); column 3 of A is empty as well
    out["isolated variable"] = (custom(12, [(i + 1, i) for i in range(11) if i not in (6, 7)] + [(8, 6)], [[0, 5], [9, 11]]), None)
    p = problems.banded_random_qp(7, 64, 3)
    q0 = pattern(problems.permute_variables(p, even_odd(64)))
    out["m = 0"] = (dict(q0, m=0, A=sp.csc_matrix((0, 64))), None)
    out["upper triangle"] = (dict(q0, stype=1, Q=q0["Q"].T.tocsc()), None)
    out["full storage"] = (dict(q0, stype=0, Q=(q0["Q"] + sp.tril(q0["Q"], -1).T).tocsc()), None)
    # stype -1 with entries stored above the diagonal: ignored, as the setup ignores them
    junk = q0["Q"].tolil(); junk[0, 63] = 1.0; junk[1, 40] = 1.0
    out["wrong-side entries"] = (dict(q0, Q=junk.tocsc()), None)
    out["row of 1025"] = (custom(1100, [(i, i) for i in range(1100)], [list(range(0, 1025))] + [[i, i + 1] for i in range(1099)]), None)
    out["row of 1024"] = (custom(1100, [(i, i) for i in range(1100)], [list(range(0, 1024))]), None)
    return out


def bandwidth(c, oldnew):
    Q, A, st = c["Q"].tocoo(), c["A"].tocsr(), c["stype"]
    keep = np.ones(Q.nnz, bool) if st == 0 else (Q.row >= Q.col if st < 0 else Q.row <= Q.col)
    b = int(np.abs(oldnew[Q.row[keep]] - oldnew[Q.col[keep]]).max()) if keep.any() else 0
    for r in range(A.shape[0]):
        cols = oldnew[A.indices[A.indptr[r]:A.indptr[r + 1]]]
        if len(cols):
            b = max(b, int(cols.max() - cols.min()))
    return b


def scipy_rcm_bandwidth(c):
    Q, A, st = c["Q"], c["A"], c["stype"]
    T = Q if st == 0 else sp.tril(Q) if st < 0 else sp.triu(Q)
    G = abs(T) + abs(T).T + abs(A).T @ abs(A)
    G = sp.csr_matrix((np.ones(G.nnz), G.indices, G.indptr), shape=G.shape)
    perm = reverse_cuthill_mckee(G, symmetric_mode=True)
    oldnew = np.empty(c["n"], np.int64); oldnew[perm] = np.arange(c["n"])
    C = G.tocoo()
    return int(np.abs(oldnew[C.row] - oldnew[C.col]).max())


def build_driver(out_dir, sanitize):
    root = os.path.dirname(_build.INCLUDE)
    exe = os.path.join(out_dir, "band_order_driver" + ("_asan" if sanitize else ""))
    san = ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else ["-O3"]
    subprocess.check_call(["gcc", "-std=gnu11", *san, "-Wall", "-Werror", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(root, "tests", "band_order_driver.c"), os.path.join(_build.CSRC, "band_order.c"), "-o", exe, "-lpthread"])
    return exe


def run_order(exe, d, tag, cs, itype):
    words = [np.array([len(cs)], np.int64)]
    for c in cs.values():
        Q, A = c["Q"], c["A"]
        words += [np.array([itype, c["stype"], c["n"], c["m"], Q.nnz, A.nnz], np.int64), Q.indptr.astype(np.int64), Q.indices.astype(np.int64),
                  A.indptr.astype(np.int64), A.indices.astype(np.int64)]
    fin, fout = os.path.join(d, tag + ".in"), os.path.join(d, tag + ".out")
    np.concatenate(words).tofile(fin)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "order", fin, fout], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(fout, np.int64)
    res, pos = {}, 0
    for name, c in cs.items():
        head = w[pos:pos + 8]; pos += 8
        res[name] = dict(rc=int(head[0]), b_natural=int(head[1]), b_ordered=int(head[2]), components=int(head[3]), early_out=int(head[4]),
                         same=int(head[5]), bw_natural=int(head[6]), bw_ordered=int(head[7]), newold=w[pos:pos + c["n"]].copy())
        pos += c["n"]
    assert pos == len(w)
    return res


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("band_order"))
    full = cases()
    cs = {k: v[0] for k, v in full.items()}
    exe = build_driver(d, False)
    return dict(dir=d, cases=cs, bw={k: v[1] for k, v in full.items()}, exe=exe, r32=run_order(exe, d, "i32", cs, 0), r64=run_order(exe, d, "i64", cs, 2))


def test_permutation_deterministic_both_itypes(job):
    for name, c in job["cases"].items():
        r, r64 = job["r32"][name], job["r64"][name]
        assert r["rc"] == 0 and r64["rc"] == 0, name
        assert np.array_equal(np.sort(r["newold"]), np.arange(c["n"])), name
        assert r["same"] == 1 and r64["same"] == 1, name                       # two calls, equal output
        assert np.array_equal(r["newold"], r64["newold"]), name
        assert [r[k] for k in ("b_natural", "b_ordered", "components", "early_out")] == [r64[k] for k in ("b_natural", "b_ordered", "components", "early_out")], name


def test_bandwidths_are_exact(job):
    for name, c in job["cases"].items():
        r = job["r32"][name]
        oldnew = np.empty(c["n"], np.int64); oldnew[r["newold"]] = np.arange(c["n"])
        assert r["b_natural"] == bandwidth(c, np.arange(c["n"])) == r["bw_natural"], name
        assert r["b_ordered"] == bandwidth(c, oldnew) == r["bw_ordered"], name


def test_quality_against_scipy(job):
    worst = 0.0
    for name, c in job["cases"].items():
        bw = job["bw"][name]
        if bw is None or name.endswith("natural"):
            continue
        r = job["r32"][name]
        ref = scipy_rcm_bandwidth(c)
        ratio = r["b_ordered"] / ref
        worst = max(worst, ratio)
        print("%-22s natural %5d  ordered %4d  scipy %4d  ratio %.3f" % (name, r["b_natural"], r["b_ordered"], ref, ratio))
        assert ratio <= QUALITY_PIN, (name, r["b_ordered"], ref)
        # the two conditions that do not depend on that measurement
        if name.split()[0] in NARROW:
            assert r["b_ordered"] == bw, name
        if bw <= 63:
            assert r["b_ordered"] <= 127, name
    print("largest ratio %.4f" % worst)
    assert math.ceil(worst / 0.05 - 1e-9) * 0.05 <= QUALITY_PIN + 1e-12


def test_edge_cases(job):
    r = job["r32"]
    assert r["chain4096 natural"]["b_ordered"] == r["chain4096 natural"]["b_natural"] == 1       # hence not adopted by the RCM mode
    assert r["two chains"]["components"] == 2 and r["two chains"]["b_natural"] == 2 and r["two chains"]["b_ordered"] == 1
    # components in order of their smallest index, the whole reversed: the chain of variable 0 comes last
    assert set(r["two chains"]["newold"][20:]) == set(range(0, 40, 2))
    iso = r["isolated variable"]                                     # {0 .. 6, 8 .. 11} (6 - 8 through Q, 0 - 5 and 9 - 11 through rows), {7}
    assert iso["components"] == 2 and iso["b_natural"] == 5 and iso["b_ordered"] == 2 and iso["newold"][0] == 7
    q0 = r["m = 0"]
    assert q0["b_natural"] == 33 and q0["b_ordered"] == 3
    for name in ("upper triangle", "full storage", "wrong-side entries"):          # the same graph from every storage of Q
        assert r[name]["b_natural"] == 33 and np.array_equal(r[name]["newold"], q0["newold"]), name
    big = r["row of 1025"]
    assert big["early_out"] == 1 and np.array_equal(big["newold"], np.arange(1100)) and big["b_ordered"] == big["b_natural"] == 1024
    assert r["row of 1024"]["early_out"] == 0 and r["row of 1024"]["b_ordered"] == 1023


def test_config_refusals(job):
    r = subprocess.run([job["exe"], "config"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL PASS" in r.stdout, r.stdout + r.stderr


def test_under_sanitizers(job):
    """the same runs with AddressSanitizer + UBSan on the stand-alone program: same output, no report"""
    exe = build_driver(job["dir"], True)
    ra = run_order(exe, job["dir"], "asan", job["cases"], 0)
    for name in job["cases"]:
        assert np.array_equal(ra[name]["newold"], job["r32"][name]["newold"]) and ra[name]["b_ordered"] == job["r32"][name]["b_ordered"], name
    r = subprocess.run([exe, "config"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and "ALL PASS" in r.stdout, r.stdout + r.stderr
