"""The bordered band of QPDO_BAND_BORDER on the CPU.  (a) The detection (qpdo_amd/csrc/band_border.c) on its own: a stand-alone C program
(tests/band_border_driver.c) links only that translation unit -- no device library, no HIP --, reads the patterns from a file and writes
{n_core, c, b_core, reason} back; it is compared with the numpy statement of the rule (tests/band_border_ref.detect), and the same program
runs a second time under AddressSanitizer + UBSan.  (b) The instances tests/test_gpu_band_border.py solves: the oracle ends each with
status 1 and the recorded counts, and on at least three of the five a border variable lies more than 1e-3 off its bound.  (c) A float64
emulation of the block elimination, pass by pass on the oracle's Newton systems of those instances, stays at a normwise backward error
of at most 4 n u -- the bound the device's solves are held to."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import band_border_ref as ref
from helpers import U64
from oracle import binding as ob
from qpdo_amd import _build, problems


def pattern(prob):
    return dict(n=prob["n"], m=prob["m"], stype=prob.get("Qstype", -1), Q=sp.csc_matrix(prob["Q"]), A=sp.csc_matrix(prob["A"]), max_border=64)


def custom(n, q_entries, rows, stype=-1, max_border=64):
    """a pattern from lists: q_entries (i, j) as stored, rows = the column lists of A"""
    qi = np.array([e[0] for e in q_entries], dtype=np.int64)
    qj = np.array([e[1] for e in q_entries], dtype=np.int64)
    Q = sp.csc_matrix((np.ones(len(qi)), (qi, qj)), shape=(n, n))
    ar = np.concatenate([np.full(len(c), r, dtype=np.int64) for r, c in enumerate(rows)]) if rows else np.zeros(0, np.int64)
    ac = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows]) if rows else np.zeros(0, np.int64)
    A = sp.csc_matrix((np.ones(len(ar)), (ar, ac)), shape=(len(rows), n))
    Q.sort_indices(); A.sort_indices()
    return dict(n=n, m=len(rows), stype=stype, Q=Q, A=A, max_border=max_border)


def reversed_columns(c):
    """the same pattern with the row indices of every column in descending order"""
    out = dict(c)
    for name in ("Q", "A"):
        M = c[name].copy()
        for j in range(M.shape[1]):
            M.indices[M.indptr[j]:M.indptr[j + 1]] = M.indices[M.indptr[j]:M.indptr[j + 1]][::-1]
        M.has_sorted_indices = False
        out[name] = M
    return out


def cases():
    out = {}
    for n, bw in ((64, 3), (260, 4), (1100, 127)):
        out["banded bw%d" % bw] = pattern(problems.banded_random_qp(7, n, bw))
    out["banded bw130"] = pattern(problems.banded_random_qp(7, 1100, 130))               # wider than T everywhere: n_core collapses, c > 64
    for c in (1, 2, 64, 65):
        out["border %d" % c] = pattern(problems.bordered_banded_qp(7, 300, 6, c))
    out["border 3 of 2"] = dict(pattern(problems.bordered_banded_qp(7, 300, 6, 3)), max_border=2)
    out["border 2, no Q links"] = pattern(problems.bordered_banded_qp(7, 300, 6, 2, q_links=0))
    diag = [(i, i) for i in range(200)]
    chain = [(i + 1, i) for i in range(199)]
    out["Q-only border"] = custom(200, diag + chain + [(198, 3), (199, 60)], [[i, i + 2] for i in range(190)])
    out["Q-only border, upper"] = custom(200, diag + [(i, i + 1) for i in range(199)] + [(3, 198), (60, 199)], [[i, i + 2] for i in range(190)], stype=1)
    out["Q-only border, full"] = custom(200, diag + chain + [(i, i + 1) for i in range(199)] + [(198, 3), (3, 198)], [], stype=0)
    out["wrong-side entry"] = custom(200, diag + chain + [(3, 198)], [[i, i + 2] for i in range(190)])          # stype -1 ignores it
    out["A-only border"] = custom(200, diag + chain, [[i, i + 3] for i in range(150)] + [[10, 11, 199], [0, 198, 199]])
    out["row ends inside the band"] = custom(200, diag, [[60, 187], [61, 100, 188]])                            # span 127 is still a band
    out["row one past the band"] = custom(200, diag, [[60, 188]])
    out["second column of a row"] = custom(400, diag + [(i, i) for i in range(200, 400)], [[5, 100, 150, 300, 399]])
    out["empty row"] = custom(200, diag + chain, [[0, 1], [], [5, 199], []])
    p = pattern(problems.bordered_banded_qp(7, 300, 6, 2))
    out["m = 0"] = dict(p, m=0, A=sp.csc_matrix((0, p["n"])))
    out["A = NULL"] = dict(p, m=-1, A=sp.csc_matrix((0, p["n"])))
    out["unsorted columns"] = reversed_columns(pattern(problems.bordered_banded_qp(7, 300, 6, 3)))
    return out


def build_driver(out_dir, sanitize):
    root = os.path.dirname(_build.INCLUDE)
    exe = os.path.join(out_dir, "band_border_driver" + ("_asan" if sanitize else ""))
    san = ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else ["-O3"]
    subprocess.check_call(["gcc", "-std=gnu11", *san, "-Wall", "-Werror", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(root, "tests", "band_border_driver.c"), os.path.join(_build.CSRC, "band_border.c"), "-o", exe])
    return exe


def run_detect(exe, d, tag, cs, itype):
    words = [np.array([len(cs)], np.int64)]
    for c in cs.values():
        Q, A = c["Q"], c["A"]
        words += [np.array([itype, c["stype"], c["n"], c["m"], Q.nnz, A.nnz, c["max_border"]], np.int64), Q.indptr.astype(np.int64),
                  Q.indices.astype(np.int64), A.indptr.astype(np.int64), A.indices.astype(np.int64)]
    fin, fout = os.path.join(d, tag + ".in"), os.path.join(d, tag + ".out")
    np.concatenate(words).tofile(fin)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "detect", fin, fout], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(fout, np.int64).reshape(len(cs), 6)
    return {name: dict(rc=int(h[0]), n_core=int(h[1]), c=int(h[2]), b_core=int(h[3]), reason=int(h[4]), same=int(h[5])) for name, h in zip(cs, w)}


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("band_border"))
    cs = cases()
    exe = build_driver(d, False)
    return dict(dir=d, cases=cs, exe=exe, r32=run_detect(exe, d, "i32", cs, 0), r64=run_detect(exe, d, "i64", cs, 2))


def test_driver_agrees_with_the_rule(job):
    for name, c in job["cases"].items():
        r, r64 = job["r32"][name], job["r64"][name]
        assert r["rc"] == 0 and r["same"] == 1 and r == r64, (name, r, r64)
        n_core, cc, b_core = ref.detect(c["Q"], c["A"], c["stype"])
        assert (r["n_core"], r["c"], r["b_core"]) == (n_core, cc, b_core), (name, r, (n_core, cc, b_core))
        assert r["n_core"] + r["c"] == c["n"] and 3 <= r["b_core"] <= 127, (name, r)
        assert r["reason"] == (1 if cc > c["max_border"] else 0), (name, r)


def test_known_answers(job):
    r = job["r32"]
    for name, bw in (("banded bw3", 3), ("banded bw4", 4), ("banded bw127", 127)):
        assert r[name]["c"] == 0 and r[name]["b_core"] == bw, (name, r[name])
    assert r["banded bw130"]["c"] > 64 and r["banded bw130"]["reason"] == 1
    for c in (1, 2, 64, 65):
        assert (r["border %d" % c]["n_core"], r["border %d" % c]["c"], r["border %d" % c]["b_core"]) == (300, c, 6)
        assert r["border %d" % c]["reason"] == (1 if c == 65 else 0)
    assert r["border 3 of 2"]["c"] == 3 and r["border 3 of 2"]["reason"] == 1
    assert (r["border 2, no Q links"]["n_core"], r["border 2, no Q links"]["c"]) == (300, 2)
    for name in ("Q-only border", "Q-only border, upper", "Q-only border, full"):
        assert (r[name]["n_core"], r[name]["c"]) == (198, 2), (name, r[name])
    assert r["wrong-side entry"]["c"] == 0
    assert (r["A-only border"]["n_core"], r["A-only border"]["c"], r["A-only border"]["b_core"]) == (198, 2, 3)
    assert r["row ends inside the band"]["c"] == 0 and r["row ends inside the band"]["b_core"] == 127
    assert (r["row one past the band"]["n_core"], r["row one past the band"]["c"]) == (188, 12)
    assert (r["second column of a row"]["n_core"], r["second column of a row"]["b_core"]) == (150, 95)       # 150 is the first column beyond 5 + 127
    assert (r["empty row"]["n_core"], r["empty row"]["c"]) == (199, 1)
    for name in ("m = 0", "A = NULL"):                                                                         # Q's links alone carry the border
        assert (r[name]["n_core"], r[name]["c"], r[name]["b_core"]) == (300, 2, 6), (name, r[name])
    assert (r["unsorted columns"]["n_core"], r["unsorted columns"]["c"], r["unsorted columns"]["b_core"]) == (300, 3, 6)


def test_refusals(job):
    r = subprocess.run([job["exe"], "args"], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL PASS" in r.stdout, r.stdout + r.stderr


def test_under_sanitizers(job):
    """the same runs with AddressSanitizer + UBSan on the stand-alone program: same output, no report"""
    exe = build_driver(job["dir"], True)
    assert run_detect(exe, job["dir"], "asan", job["cases"], 0) == job["r32"]
    assert run_detect(exe, job["dir"], "asan64", job["cases"], 2) == job["r64"]
    r = subprocess.run([exe, "args"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and "ALL PASS" in r.stdout, r.stdout + r.stderr


# ---- the instances of the whole-solve tests ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_solutions():
    out = {}
    for key in ref.ORACLE_RESULTS:
        o = ob.OracleSolver(ref.bordered_qp(key), ob.default_settings())
        out[key] = o.solve()
        o.close()
    return out


def test_generator_reproduces_the_recorded_oracle_runs(oracle_solutions):
    off = []
    for key, ro in oracle_solutions.items():
        n_core, bw, c = key
        p = ref.bordered_qp(key)
        assert ref.detect(p["Q"], p["A"]) == (n_core, c, max(3, bw)), key
        # the first border variable meets a row that starts 128 or more columns before it: without that the problem is plainly banded
        A = sp.csr_matrix(p["A"])
        first = min(A.indices[A.indptr[r]] for r in A[:, n_core].nonzero()[0])
        assert n_core - first >= 128, key
        assert (ro["info"]["status_val"], ro["info"]["iterations"], ro["info"]["oterations"]) == ref.ORACLE_RESULTS[key], key
        if np.any(ro["x"][n_core:] > 1e-3):
            off.append(key)
    assert off == ref.BORDER_OFF_BOUND and len(off) >= 3, off


@pytest.mark.parametrize("key", list(ref.ORACLE_RESULTS))
def test_emulation_is_backward_stable_on_every_newton_pass_of_the_oracle(key):
    p = ref.bordered_qp(key)
    n, n_core = p["n"], key[0]
    passes, worst = 0, 0.0
    for s in ref.oracle_newton_systems(p):
        K, rhs = s["K"], s["rhs"]
        scale = np.abs(K).sum(axis=1).max() * np.abs(s["dx"]).max() + np.abs(rhs).max()
        assert np.abs(K @ s["dx"] - rhs).max() <= 1e-9 * scale, s["pass_no"]          # the pieces are the oracle's: K dx = rhs for its own direction
        x = ref.eliminate_solve(K, n_core, rhs)
        eta = ref.dense_backward_error(K, x, rhs) / (n * U64)
        worst = max(worst, eta)
        assert eta <= 4.0, (key, s["pass_no"], eta)
        passes += 1
    print("%s: %d Newton passes, largest eta / (n u) %.3g" % (key, passes, worst))
    assert passes > 0
