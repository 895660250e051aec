"""The host CSC -> CSR conversions (qpdo_amd/csrc/csc_convert.c) on their own, against scipy, exactly: CSR(A) with its map, CSR(A') (the
narrowed CSC arrays), the full symmetric CSR(Q) from a lower / upper triangle or full storage with its map and its entry count, and the
row-partition cut.  A stand-alone C program (tests/csc_convert_driver.c) links only that translation unit -- no device library, no HIP --
reads raw arrays from a file and writes the results back; the same program runs a second time under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from qpdo_amd import _build

THREADS = (1, 7, 16)
ITYPES = ((0, np.int32), (2, np.int64))


A_NAMES = ["1x5", "0xn", "n=1", "empty rows and columns", "stored zeros", "300x500", "3000x70000"]
Q_SIZES = (("n=1", 1, 1.0), ("n=7", 7, 0.5), ("n=120", 120, 0.1), ("n=3000", 3000, 0.05))      # the last: above the threading threshold
WRONG_SIDE = (" lower, entries above the diagonal too", " upper, entries below the diagonal too")
Q_NAMES = [b + s for b, n, _ in Q_SIZES for s in (" lower", " upper", " full") + (WRONG_SIDE if n in (7, 120) else ())] + \
    ["strictly lower, stored zeros", "n=0"]


def rand_csc(rng, m, n, density):
    M = sp.random(m, n, density=density, format="csc", random_state=rng, data_rvs=rng.standard_normal)
    M.sort_indices()
    return M


def a_cases():
    rng = np.random.default_rng(20240611)
    holes = rand_csc(rng, 40, 30, 0.2).tolil()
    holes[[0, 7, 8, 39], :] = 0
    holes[:, [0, 3, 29]] = 0                                   # empty rows and empty columns, first and last included
    zeros = rand_csc(rng, 9, 11, 0.4)
    zeros.data[::3] = 0.0                                      # explicit stored zeros stay entries
    wide = rand_csc(rng, 3000, 70000, 0.002)                   # ~420k entries: above the threading threshold, ragged column ranges
    return {
        "1x5": sp.csc_matrix(np.array([[1.5, 0.0, -2.0, 0.0, 3.0]])),
        "0xn": sp.csc_matrix((0, 6)),
        "n=1": sp.csc_matrix(np.array([[0.0], [4.0], [0.0], [-1.0]])),
        "empty rows and columns": sp.csc_matrix(holes),
        "stored zeros": zeros,
        "300x500": rand_csc(rng, 300, 500, 0.05),
        "3000x70000": wide,
    }


def q_cases():
    """name -> (stored matrix, stype); the stored matrices of stype -1 / +1 may carry entries on the wrong side"""
    rng = np.random.default_rng(977)
    out = {}
    for name, n, density in Q_SIZES:
        S = rand_csc(rng, n, n, density)
        S = (S + sp.diags(rng.standard_normal(n) + 3.0)).tocsc()
        S.sort_indices()
        out[name + " lower"] = (sp.tril(S, format="csc"), -1)
        out[name + " upper"] = (sp.triu(S, format="csc"), 1)
        out[name + " full"] = ((S + S.T).tocsc(), 0)
        if n in (7, 120):
            out[name + WRONG_SIDE[0]] = (S, -1)
            out[name + WRONG_SIDE[1]] = (S, 1)
    D = sp.tril(rand_csc(rng, 12, 12, 0.5), -1, format="csc")      # no diagonal at all, one empty column, stored zeros
    D.data[::4] = 0.0
    out["strictly lower, stored zeros"] = (D, -1)
    out["n=0"] = (sp.csc_matrix((0, 0)), -1)
    return out


def matrix_bytes(M, itype, dtype, stype=0):
    M = M.tocsc()
    return b"".join((np.array([M.shape[0], M.shape[1], M.nnz, itype, stype], np.int64).tobytes(), M.indptr.astype(dtype).tobytes(),
                     M.indices.astype(dtype).tobytes(), M.data.astype(np.float64).tobytes()))


def record(op, threads, world, mats):
    return np.array([op, threads, world, len(mats)], np.int64).tobytes() + b"".join(mats)


class Reader:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def take(self, dtype, count):
        a = np.frombuffer(self.buf, dtype, count, self.pos)
        self.pos += a.nbytes
        return a

    def csr(self, nrows):
        rp = self.take(np.int32, nrows + 1)
        return rp, self.take(np.int32, int(rp[-1])), self.take(np.float64, int(rp[-1]))


PARTITION = {"m=5 over 4": (5, 9, 4), "n=3 over 4": (7, 3, 4), "one rank": (6, 5, 1), "60x45 over 7": (60, 45, 7)}


def build_driver(out_dir, sanitize):
    root = os.path.dirname(_build.INCLUDE)
    exe = os.path.join(out_dir, "csc_convert_driver" + ("_asan" if sanitize else ""))
    san = ["-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else ["-O3"]
    subprocess.check_call(["gcc", "-std=gnu11", *san, "-ffp-contract=off", "-fopenmp", "-Wall", "-Werror", "-I", _build.INCLUDE, "-I", _build.CSRC,
                           os.path.join(root, "tests", "csc_convert_driver.c"), os.path.join(_build.CSRC, "csc_convert.c"), "-o", exe, "-lm"])
    return exe


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """every case as one input file (written once), the order of its records, and the plain build's output"""
    d = tmp_path_factory.mktemp("csc_convert")
    A, Q = a_cases(), q_cases()
    assert list(A) == A_NAMES and sorted(Q) == sorted(Q_NAMES)
    # the cases meant for the threaded branches are above the 200000-entry threshold, whatever the generator gave
    assert A["3000x70000"].nnz > 200000 and all(Q["n=3000" + s][0].nnz > 200000 for s in (" lower", " upper", " full"))
    order, blobs = [], []
    for name, M in A.items():
        for itype, dtype in ITYPES:
            for t in THREADS + ((0,) if M.nnz > 200000 else ()):      # 0: the default team, which threads only above 200000 entries
                order.append(("A", name, itype, t))
                blobs.append(record(0, t, 1, [matrix_bytes(M, itype, dtype)]))
    for name, (S, stype) in Q.items():
        for itype, dtype in ITYPES:
            for t in THREADS:
                order.append(("Q", name, itype, t))
                blobs.append(record(1, t, 1, [matrix_bytes(S, itype, dtype, stype)]))
    rng = np.random.default_rng(5)
    cuts = {}
    for name, (m, n, world) in PARTITION.items():
        a = rand_csc(rng, m, n, 0.5)
        q = sp.tril(rand_csc(rng, n, n, 0.6) + sp.identity(n), format="csc")
        cuts[name] = (a, q, world)
        order.append(("P", name, 0, 1))
        blobs.append(record(2, 1, world, [matrix_bytes(a, 0, np.int32), matrix_bytes(q, 0, np.int32, -1)]))
    fin = d / "in.bin"
    fin.write_bytes(b"".join(blobs))
    exe = build_driver(str(d), False)
    out = subprocess.run([exe, str(fin), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "converted %d records" % len(order) in out.stdout, out.stdout + out.stderr
    return dict(dir=d, fin=fin, exe=exe, A=A, Q=Q, cuts=cuts, order=order, out=(d / "out.bin").read_bytes())


@pytest.fixture(scope="module")
def results(job):
    """the output parsed record by record: {(kind, name, itype, threads): arrays}"""
    R, res = Reader(job["out"]), {}
    for key in job["order"]:
        kind, name = key[:2]
        if kind == "A":
            M = job["A"][name]
            rc = int(R.take(np.int64, 1)[0])
            rp, ci, val = R.csr(M.shape[0])
            res[key] = dict(rc=rc, rp=rp, ci=ci, val=val, map=R.take(np.int32, M.nnz), T=R.csr(M.shape[1]))
        elif kind == "Q":
            S = job["Q"][name][0]
            count, rc = (int(v) for v in R.take(np.int64, 2))
            res[key] = dict(count=count, rc=rc)
            if rc == 0:
                rp, ci, val = R.csr(S.shape[0])
                res[key].update(rp=rp, ci=ci, val=val, map=R.take(np.int32, count))
        else:
            a, q, world = job["cuts"][name]
            ranks = []
            for _ in range(world):
                m0, mloc, n0, nloc = (int(v) for v in R.take(np.int32, 4))
                ranks.append(dict(m0=m0, mloc=mloc, n0=n0, nloc=nloc, Al=R.csr(mloc), Tl=R.csr(a.shape[1]), Ql=R.csr(nloc)))
            res[key] = ranks
    assert R.pos == len(job["out"])
    return res


def keys(job, kind, name):
    return [k for k in job["order"] if k[0] == kind and k[1] == name]


def same(got, rp, ci, val):
    return np.array_equal(got[0], rp) and np.array_equal(got[1], ci) and np.array_equal(got[2].view(np.int64), np.asarray(val, np.float64).view(np.int64))


def expected_full(S, stype):
    """the full symmetric matrix of a stored triangle, stored zeros kept, as sorted CSR: (tril + tril(-1)') or (triu + triu(1)')"""
    C = S.tocoo()
    if stype == 0:
        F = C
    else:
        own = (C.row >= C.col) if stype < 0 else (C.row <= C.col)
        strict = (C.row > C.col) if stype < 0 else (C.row < C.col)
        F = sp.coo_matrix((np.concatenate((C.data[own], C.data[strict])),
                           (np.concatenate((C.row[own], C.col[strict])), np.concatenate((C.col[own], C.row[strict])))), shape=S.shape)
    F = F.tocsr()
    F.sort_indices()
    return F


@pytest.mark.parametrize("name", A_NAMES)
def test_csr_of_a_and_of_its_transpose_match_scipy(job, results, name):
    M = job["A"][name]
    E = M.tocsr()
    E.sort_indices()
    assert E.nnz == M.nnz                                                 # scipy kept the stored zeros
    ks = keys(job, "A", name)
    assert len(ks) == len(ITYPES) * (len(THREADS) + (M.nnz > 200000))
    for k in ks:
        r = results[k]
        assert r["rc"] == 0, k
        assert same((r["rp"], r["ci"], r["val"]), E.indptr, E.indices, E.data), k
        assert same(r["T"], M.indptr, M.indices, M.data), k               # CSR(A') is the CSC arrays, narrowed
        assert np.array_equal(np.sort(r["map"]), np.arange(M.nnz)), k     # a permutation of the CSC positions
        assert np.array_equal(r["val"].view(np.int64), M.data[r["map"]].view(np.int64)), k
        assert np.array_equal(M.indices[r["map"]], np.repeat(np.arange(M.shape[0]), np.diff(r["rp"]))), k
        for other in ("rp", "ci", "val", "map"):                          # identical for every thread count and index width
            assert np.array_equal(r[other], results[ks[0]][other]), (k, other)


@pytest.mark.parametrize("name", Q_NAMES)
def test_full_symmetric_q_matches_scipy_in_the_order_of_the_rule(job, results, name):
    S, stype = job["Q"][name]
    n = S.shape[0]
    E = expected_full(S, stype)
    if stype and not (S.data == 0).any():                                 # the expression of the contract itself, where no stored zero is in the way
        tri = (sp.tril(S) + sp.tril(S, -1).T) if stype < 0 else (sp.triu(S) + sp.triu(S, 1).T)
        tri = tri.tocsr()
        tri.sort_indices()
        assert same((E.indptr, E.indices, E.data), tri.indptr, tri.indices, tri.data)
    col_of = np.repeat(np.arange(n), np.diff(S.indptr))                   # column of every stored position
    on_diag = S.indices == col_of
    kept = np.ones(S.nnz, bool) if stype == 0 else (S.indices >= col_of) if stype < 0 else (S.indices <= col_of)
    ks = keys(job, "Q", name)
    assert len(ks) == len(ITYPES) * len(THREADS)
    for k in ks:
        r = results[k]
        assert r["rc"] == 0 and r["count"] == E.nnz, k                    # the count function agrees with the arrays
        assert same((r["rp"], r["ci"], r["val"]), E.indptr, E.indices, E.data), k
        mp = r["map"]
        assert np.array_equal(r["val"].view(np.int64), S.data[mp].view(np.int64)), k
        uses = np.bincount(mp, minlength=S.nnz)
        if stype == 0:
            assert np.array_equal(mp, np.arange(S.nnz)), k
            continue
        # every diagonal position once, every stored off-diagonal position twice, the wrong side never
        assert np.array_equal(uses, np.where(kept, np.where(on_diag, 1, 2), 0)), k
        # the rule: row i is the triangle's own row i (each entry taken from column `col`, row i of the stored matrix), and the stored
        # column i beyond the diagonal in stored order -- own part first for lower storage, last for upper storage
        row = np.repeat(np.arange(n), np.diff(r["rp"]))
        own = (r["ci"] <= row) if stype < 0 else (r["ci"] >= row)
        assert np.array_equal(col_of[mp[own]], r["ci"][own]) and np.array_equal(S.indices[mp[own]], row[own]), k
        assert np.array_equal(col_of[mp[~own]], row[~own]) and np.array_equal(S.indices[mp[~own]], r["ci"][~own]), k
        first = own if stype < 0 else ~own                                # within a row: `first` entries, then the others
        flips = np.diff(first.astype(np.int8))
        assert not ((flips == 1) & (np.diff(row) == 0)).any(), k
        same_part = (np.diff(row) == 0) & (flips == 0) & ~own[1:]
        assert (np.diff(mp)[same_part] > 0).all(), k                      # the mirrored column in stored order
        for other in ("rp", "ci", "val", "map"):
            assert np.array_equal(r[other], results[ks[0]][other]), (k, other)


@pytest.mark.parametrize("name", list(PARTITION))
def test_row_partition_cut(job, results, name):
    a, q, world = job["cuts"][name]
    m, n = a.shape
    Ar = a.tocsr()
    Ar.sort_indices()
    Qf = expected_full(q, -1)
    ranks = results[("P", name, 0, 1)]
    rpm, rpn = -(-m // world), -(-n // world)
    if name == "m=5 over 4":
        assert [r["mloc"] for r in ranks] == [2, 2, 1, 0]
    if name == "n=3 over 4":
        assert [r["nloc"] for r in ranks] == [1, 1, 1, 0]
    for k, r in enumerate(ranks):
        assert (r["m0"], r["mloc"]) == (min(k * rpm, m), min((k + 1) * rpm, m) - min(k * rpm, m))
        assert (r["n0"], r["nloc"]) == (min(k * rpn, n), min((k + 1) * rpn, n) - min(k * rpn, n))
        # A' of the rank: exactly the columns of its row range, renumbered from 0
        Tl = a.T.tocsr()[:, r["m0"]:r["m0"] + r["mloc"]]
        Tl.sort_indices()
        assert same(r["Tl"], Tl.indptr, Tl.indices, Tl.data), (name, k)
    for part, E in (("Al", Ar), ("Ql", Qf)):                              # the slices in rank order give the whole matrix back
        rp = np.concatenate([[0]] + [r[part][0][1:] + sum(int(p[part][0][-1]) for p in ranks[:k]) for k, r in enumerate(ranks)])
        assert same((rp, np.concatenate([r[part][1] for r in ranks]), np.concatenate([r[part][2] for r in ranks])), E.indptr, E.indices, E.data), (name, part)
        assert all(r[part][0][0] == 0 for r in ranks)


def test_a_runtime_that_grants_fewer_threads_than_asked_for_changes_nothing(job):
    """the threaded conversions split their work by range, not by thread number: 7 or 16 ranges on a team of at most 3 give the same bytes"""
    fout = job["dir"] / "out_limit3.bin"
    out = subprocess.run([job["exe"], str(job["fin"]), str(fout)], capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_THREAD_LIMIT="3"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert fout.read_bytes() == job["out"]


def test_the_same_run_under_address_and_ub_sanitizers(job):
    """the conversion unit and its C caller with -fsanitize=address,undefined, as a stand-alone program: no report, the same bytes"""
    exe = build_driver(str(job["dir"]), True)
    fout = job["dir"] / "out_asan.bin"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe, str(job["fin"]), str(fout)], capture_output=True, text=True, timeout=600, env=env)
    txt = out.stdout + out.stderr
    assert out.returncode == 0 and "converted %d records" % len(job["order"]) in txt, txt[-3000:]
    assert "AddressSanitizer" not in txt and "runtime error" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
    assert fout.read_bytes() == job["out"]
