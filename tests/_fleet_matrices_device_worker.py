"""Child process of tests/test_gpu_fleet_matrices_device.py: the scenarios of new fleet matrix values from device arrays
(qpdo_amd_fleet_update_matrices_dev; solver.Fleet.pack_matrix_values / update_matrices_device), each run once, their outcomes written as
JSON.  A process of its own because torch comes FIRST here (one HIP runtime in the process; tests/_fleet_device_worker.py).

Every scenario drives one fleet H through the host calls and a second one D, built from the same problems, through the device calls, and
compares bit patterns.  Both receive the same numbers: the matrices of tests/test_gpu_fleet_matrices.py (new_Q / new_A), packed by
pack_matrix_values for D.  The places of the packed arrays that belong to items WITHOUT an entry are filled with NaN before the upload: a
gather that ignored the mask, or read a neighbour's slice, could not go unnoticed.

The fleet is the small heterogeneous one of that file -- the two infeasibility KATs (1 - 4 entries), two C3 items (A has more than 256
entries and no multiple of it), an m = 0 item between items that have A entries (equal adjacent offsets), random_qp(23, 40, 60, ..), stypes
-1 / +1 / 0 in turn (the three mapQ rules) -- followed by an LP whose Q stores NO entry (create accepts it): a taken Q of zero entries
gets a valid offset, and the last item's Q slice is empty at the end of the array.
usage: _fleet_matrices_device_worker.py OUT.json"""
import functools
import json
import os
import sys
import traceback

import numpy as np
import torch  # noqa: F401  (before qpdo_amd loads its library: one HIP runtime in the process)
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from qpdo_amd import solver  # noqa: E402
from _fleet_device_worker import band_problems, compare, compare_host, finite, imask, pack  # noqa: E402
from test_gpu_fleet_matrices import Twins, fleet_problems, new_A, new_Q, pick, with_stype  # noqa: E402
from test_gpu_small import assert_identical  # noqa: E402

ST = dict(max_iter=1000, verbose=0)


def lp_item():
    """min q'x over a box and one coupling row: Q = 0 with no stored entry"""
    rng = np.random.default_rng(5)
    n = 6
    A = sp.vstack([sp.eye(n), sp.csc_matrix(rng.standard_normal((1, n)))]).tocsc()
    return dict(n=n, m=n + 1, Q=sp.csc_matrix((n, n)), Qstype=-1, q=rng.standard_normal(n), A=A, l=-np.ones(n + 1), u=np.ones(n + 1), c=0.0)


@functools.lru_cache(maxsize=None)
def worker_problems():
    return tuple(fleet_problems(False)) + (lp_item(),)


def gpu(a):
    return None if a is None else torch.from_numpy(a).cuda()


def packed(D, Q, A):
    """pack_matrix_values, with NaN wherever an item has no entry"""
    qv, av, mask = D.pack_matrix_values(Q=Q, A=A)
    qoff, aoff = D.packed_matrix_layout()
    for vals, off, bit in ((qv, qoff, 1), (av, aoff, 2)):
        if vals is not None:
            for i in range(D.count):
                if not mask[i] & bit:
                    vals[off[i]:off[i + 1]] = np.nan
    return qv, av, mask


def both_matrices(H, D, Q, A):
    """the same entries to H through the host call and to D through the device call"""
    H.update_matrices(Q=Q, A=A)
    qv, av, mask = packed(D, Q, A)
    D.update_matrices_device(gpu(qv), gpu(av), mask=gpu(mask))


def values(probs, seed, idx_Q, idx_A):
    Q = pick([new_Q(p, seed + 10 * i) for i, p in enumerate(probs)], idx_Q) if idx_Q is not None else None
    A = pick([new_A(p, seed + 10 * i + 1) for i, p in enumerate(probs)], idx_A) if idx_A is not None else None
    return Q, A


def bit_parity_with_the_host_path(scaling):
    probs = list(worker_problems())
    N = len(probs)
    H, D = solver.Fleet(probs, matrix_updates=True, scaling=scaling, **ST), solver.Fleet(probs, matrix_updates=True, scaling=scaling, **ST)
    rng = np.random.default_rng(11)
    all_items, even, odd = set(range(N)), set(range(0, N, 2)), set(range(1, N, 2))

    def solve(what, fetch=False):
        rh = H.solve()
        out = D.solve_device()
        compare(D, out, rh, what)
        if fetch:
            compare_host(D.fetch_last(), rh, "fetch_last after " + what)
        return rh

    try:
        qoff, aoff = D.packed_matrix_layout()
        nq, na = [sp.csc_matrix(p["Q"]).nnz for p in probs], [sp.csc_matrix(p["A"]).nnz for p in probs]
        assert qoff.tolist() == [0] + np.cumsum(nq).tolist() and aoff.tolist() == [0] + np.cumsum(na).tolist()
        # the shapes the gather can go wrong at are all here
        assert max(na) > 256 and max(na) % 256 and min(x for x in nq + na if x) <= 4 and 0 in na[1:-1] and nq[-1] == 0, (nq, na)
        rh = solve("1 cold", fetch=True)
        sts = [r["info"]["status_val"] for r in rh]
        assert sts[0] == -3 and sts[1] == -4 and sts.count(1) >= 4, sts
        q, l, u = [1.5 * p["q"] + 0.1 for p in probs], [p["l"] - 0.1 for p in probs], [p["u"] + 0.05 for p in probs]
        H.update(q, l, u); D.update_device(pack(q), pack(l), pack(u))
        both_matrices(H, D, *values(probs, 100, even, even))
        rh = solve("2 update q, l, u; new Q and A on the even items; from zero", fetch=True)
        both_matrices(H, D, *values(probs, 200, {i for i in all_items if i % 3 == 1}, {i for i in all_items if i % 3 == 0}))
        H.warm_start_last(); D.warm_start_last_device()
        rh = solve("3 A only / Q only / neither; warm_start_last")
        xw = [finite(r["x"]) + 1e-3 * rng.standard_normal(p["n"]) for r, p in zip(rh, probs)]
        yw = [finite(r["y"]) + 1e-3 * rng.standard_normal(p["m"]) for r, p in zip(rh, probs)]
        H.warm_start(xw, yw); D.warm_start_device(pack(xw), pack(yw))
        both_matrices(H, D, *values(probs, 300, odd, odd))       # the warm start of the odd items is discarded, the even items keep theirs
        solve("4 warm start, then new Q and A on the odd items", fetch=True)
        some = {0, 3, N - 1}
        both_matrices(H, D, *values(probs, 400, some, some))
        q = [p["q"] * 0.7 - 0.2 for p in probs]
        H.update(q=q); D.update_device(q=pack(q))
        solve("5 new Q and A on some items, then update q")
        both_matrices(H, D, *values(probs, 500, even, even))
        both_matrices(H, D, *values(probs, 600, even | {1}, even | {1}))
        rh = solve("6 two matrix calls in a row")
        # a NULL mask with both arrays: every item takes both
        Q, A = values(probs, 700, all_items, all_items)
        H.update_matrices(Q=Q, A=A)
        qv, av, mask = packed(D, Q, A)
        assert mask.tolist() == [3] * N and not np.isnan(qv).any() and not np.isnan(av).any()
        D.update_matrices_device(gpu(qv), gpu(av))
        H.warm_start_last(); D.warm_start_last_device()
        solve("7 NULL mask, both arrays", fetch=True)
        # Q_values alone under a mask that also has bit 1 set: no array, no A -- A stays what step 7 gave on every item
        Q, _ = values(probs, 800, all_items, None)
        H.update_matrices(Q=Q)
        qv, _, _ = packed(D, Q, None)
        D.update_matrices_device(Q_values=gpu(qv), mask=imask([3] * N))
        H.warm_start_last(); D.warm_start_last_device()
        solve("8 Q_values only, mask bits 0 and 1", fetch=True)
    finally:
        H.close(); D.close()


def parity_with_fresh_oracles():
    """the device path against a NEW oracle per updated item (Twins of tests/test_gpu_fleet_matrices.py, that file's assertions)"""
    probs = list(worker_problems())
    N = len(probs)
    st = dict(scaling=10, max_iter=1000, verbose=0)
    T = Twins(probs, st)
    D = solver.Fleet(probs, matrix_updates=True, **st)
    even = set(range(0, N, 2))

    def solve(what):
        D.solve_device()
        rd, ro = D.fetch_last(), T.solve()
        for i, (g, o) in enumerate(zip(rd, ro)):
            assert_identical(g, o, what="%s, item %d" % (what, i))
        return ro

    def matrices(Q, A):
        T.update_matrices(Q=Q, A=A)
        qv, av, mask = packed(D, Q, A)
        D.update_matrices_device(gpu(qv), gpu(av), mask=gpu(mask))

    try:
        solve("1 cold")
        q, l, u = [1.5 * p["q"] + 0.1 for p in probs], [p["l"] - 0.1 for p in probs], [p["u"] + 0.05 for p in probs]
        T.update(q, l, u); D.update_device(pack(q), pack(l), pack(u))
        matrices(*values(probs, 100, even, even))
        ro = solve("2 update q, l, u; new Q and A on the even items; from zero")
        matrices(*values(probs, 200, {i for i in range(N) if i % 3 == 1}, {i for i in range(N) if i % 3 == 0}))
        D.warm_start_last_device(); T.warm_start_last(ro)
        solve("3 A only / Q only / neither; warm_start_last")
    finally:
        D.close(); T.close()


def unpack(templates, vals, off):
    """per-item matrices in the templates' (sorted CSC) pattern from a packed value array"""
    out = []
    for i, M in enumerate(templates):
        M = sp.csc_matrix(M, copy=True)
        M.sort_indices()
        M.data = np.array(vals[off[i]:off[i + 1]])
        out.append(M)
    return out


def mixed_calls_and_streams():
    probs = list(worker_problems())
    N = len(probs)
    H, D = solver.Fleet(probs, matrix_updates=True, scaling=10, **ST), solver.Fleet(probs, matrix_updates=True, scaling=10, **ST)
    try:
        H.solve(); D.solve_device()
        # device matrices + host update + device solve
        Q, A = values(probs, 100, {0, 2, 3, N - 1}, {1, 2, 5})
        q = [1.2 * p["q"] - 0.05 for p in probs]
        H.update_matrices(Q=Q, A=A); H.update(q=q); H.warm_start_last(); rh = H.solve()
        qv, av, mask = packed(D, Q, A)
        D.update_matrices_device(gpu(qv), gpu(av), mask=gpu(mask)); D.update(q=q); D.warm_start_last_device(); out = D.solve_device()
        compare(D, out, rh, "device matrices, host update, device solve")
        # host matrices + device update + host solve
        Q, A = values(probs, 200, {1, 4, 5}, {0, 3, N - 1})
        q = [0.9 * p["q"] + 0.02 for p in probs]
        H.update_matrices(Q=Q, A=A); H.update(q=q); H.warm_start_last(); rh = H.solve()
        D.update_matrices(Q=Q, A=A); D.update_device(q=pack(q)); D.warm_start_last(); rd = D.solve()
        compare_host(rd, rh, "host matrices, device update, host solve")
        # a full real-time-iteration step on a stream of the caller's: the values made by torch ops on it right before, x read by one
        # right after, no wait between
        Q, A = [p["Q"] for p in probs], [p["A"] for p in probs]      # (the create-time values as the base: most items stay solvable)
        qv, av, _ = packed(D, Q, A)
        baseQ, baseA, baseq = gpu(qv), gpu(av), pack([p["q"] for p in probs])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        own = {k: torch.empty_like(v) for k, v in out.items()}
        with torch.cuda.stream(s):
            Qt, At, qt = baseQ * 1.25, baseA * 0.5, baseq * 1.25 + 0.01
            D.update_matrices_device(Qt, At); D.update_device(q=qt); D.warm_start_last_device(); out = D.solve_device(out=own)
            twice = out["x"] * 2.0
        s.synchronize()
        assert all(out[k] is own[k] for k in own)
        no, _ = D.packed_layout()
        qoff, aoff = D.packed_matrix_layout()
        qh = qt.cpu().numpy()
        H.update_matrices(Q=unpack(Q, Qt.cpu().numpy(), qoff), A=unpack(A, At.cpu().numpy(), aoff))
        H.update(q=[qh[no[i]:no[i + 1]] for i in range(N)]); H.warm_start_last(); rh = H.solve()
        compare(D, out, rh, "on a side stream")
        assert np.array_equal(twice.cpu().numpy(), 2.0 * np.concatenate([r["x"] for r in rh]), equal_nan=True)
        assert sum(r["info"]["status_val"] == 1 for r in rh) >= 3, [r["info"]["status_val"] for r in rh]
    finally:
        H.close(); D.close()


def host_side_refusals_launch_nothing():
    probs = list(worker_problems())
    st = dict(scaling=10, **ST)
    H, D, plain = solver.Fleet(probs, matrix_updates=True, **st), solver.Fleet(probs, matrix_updates=True, **st), solver.Fleet(probs, **st)
    L = solver.lib()
    err = lambda: (L.qpdo_amd_last_error() or b"").decode()
    name = "qpdo_amd_fleet_update_matrices_dev: "
    try:
        H.solve(); D.solve()
        qoff, aoff = D.packed_matrix_layout()
        NQ, NA = int(qoff[-1]), int(aoff[-1])
        Q, A = values(probs, 100, set(range(len(probs))), set(range(len(probs))))
        qv, av, mask = packed(D, Q, A)
        dq, da, dm = gpu(qv), gpu(av), gpu(mask)
        before, stats_before = D.matrix_stats(), D.stats()
        call = L.qpdo_amd_fleet_update_matrices_dev
        assert call(D._h, dq.data_ptr(), da.data_ptr(), dm.data_ptr(), NQ + 1, NA, None) != 0
        assert err().startswith(name + "q_len") and str(NQ + 1) in err() and str(NQ) in err(), err()
        assert call(D._h, dq.data_ptr(), da.data_ptr(), dm.data_ptr(), NQ, NA - 1, None) != 0
        assert err().startswith(name + "a_len") and str(NA - 1) in err() and str(NA) in err(), err()
        assert call(D._h, qv.ctypes.data, da.data_ptr(), dm.data_ptr(), NQ, NA, None) != 0 and err().startswith(name + "Qx is not device memory"), err()
        assert call(D._h, dq.data_ptr(), av.ctypes.data, dm.data_ptr(), NQ, NA, None) != 0 and err().startswith(name + "Ax is not device memory"), err()
        assert call(D._h, dq.data_ptr(), da.data_ptr(), mask.ctypes.data, NQ, NA, None) != 0 and err().startswith(name + "item_mask is not device memory"), err()
        assert call(plain._h, dq.data_ptr(), da.data_ptr(), dm.data_ptr(), NQ, NA, None) != 0
        assert err().startswith(name) and "created without QPDO_AMD_FLEET_MATRIX_UPDATES" in err(), err()
        try:
            plain.packed_matrix_layout()
            raise AssertionError("the layout of a fleet without the flag was delivered")
        except RuntimeError as e:
            assert "qpdo_amd_fleet_get_packed_matrix_layout: the fleet was created without QPDO_AMD_FLEET_MATRIX_UPDATES" in str(e), e
        try:
            D.update_matrices_device(Q_values=qv)
            raise AssertionError("a numpy array passed the tensor validator")
        except ValueError as e:
            assert str(e).startswith("Q_values: "), e
        assert D.matrix_stats() == before and D.stats() == stats_before and plain.matrix_stats()["calls"] == 0
        q1 = [1.1 * p["q"] for p in probs]
        H.update(q=q1); H.warm_start_last(); rh = H.solve()
        D.update(q=q1); D.warm_start_last(); rd = D.solve()
        compare_host(rd, rh, "after the refused calls")
    finally:
        H.close(); D.close(); plain.close()


def accounting():
    probs = list(worker_problems())
    N = len(probs)
    st = dict(scaling=10, **ST)
    F, plain = solver.Fleet(probs, matrix_updates=True, **st), solver.Fleet(probs, **st)
    try:
        nq, na = [sp.csc_matrix(p["Q"]).nnz for p in probs], [sp.csc_matrix(p["A"]).nnz for p in probs]
        # what the flag cost before the offset table existed (tests/test_gpu_fleet_matrices.py::test_stats), plus the table
        grown = F.stats()["matrix_bytes_uploaded"] - plain.stats()["matrix_bytes_uploaded"]
        assert F.matrix_stats()["resident_extra_bytes"] >= grown + 8 * (sum(na) + sum(nq)) + 4 * 2 * (N + 1)
        F.solve()
        s0 = F.stats()
        Q, A = values(probs, 100, {0, 2}, {2, 3})
        F.update_matrices(Q=Q, A=A)
        ms = F.matrix_stats()
        assert ms["calls"] == 1 and ms["items_last_call"] == 3 and ms["value_bytes_uploaded_last_call"] > 0 and ms["last_kernel_seconds"] > 0
        host_kernel_s = ms["last_kernel_seconds"]
        qv, av, mask = packed(F, Q, A)
        F.update_matrices_device(gpu(qv), gpu(av), mask=gpu(mask))
        ms = F.matrix_stats()
        assert (ms["calls"], ms["items_last_call"], ms["value_bytes_uploaded_last_call"]) == (2, -1, 0), ms
        assert ms["last_kernel_seconds"] == host_kernel_s            # the last HOST call's figure
        F.update_matrices_device()                                   # both None: returns, launches nothing
        F.update_matrices_device(mask=gpu(mask))
        assert F.matrix_stats()["calls"] == 2
        F.update_matrices_device(A_values=gpu(av))
        ms = F.matrix_stats()
        assert (ms["calls"], ms["items_last_call"], ms["value_bytes_uploaded_last_call"]) == (3, -1, 0), ms
        s1 = F.stats()
        for f in ("matrix_bytes_uploaded", "solve_launches", "solves"):
            assert s1[f] == s0[f], f
        d = F.sync()
        assert (d["update_calls"], d["warm_start_calls"], d["solve_calls"], d["refused_items"]) == (0, 0, 0, 0), d
    finally:
        F.close(); plain.close()


def a_band_layout_fleet(scaling):
    probs = [with_stype(p, st) for p, st in zip(band_problems(), (-1, 0))]
    H, D = solver.Fleet(probs, matrix_updates=True, scaling=scaling, **ST), solver.Fleet(probs, matrix_updates=True, scaling=scaling, **ST)
    try:
        assert H.factor_layout() == D.factor_layout() == solver.K_BAND
        rh = H.solve(); out = D.solve_device()
        compare(D, out, rh, "band fleet, cold")
        q = [1.1 * p["q"] + 0.01 for p in probs]
        both_matrices(H, D, *values(probs, 100, {0, 1}, {0, 1}))
        H.update(q=q); D.update_device(q=pack(q))
        H.warm_start_last(); D.warm_start_last_device()
        rh = H.solve(); out = D.solve_device()
        compare(D, out, rh, "band fleet, step 1")
        compare_host(D.fetch_last(), rh, "band fleet, fetch_last")
        both_matrices(H, D, *values(probs, 200, {1}, {0}))
        H.warm_start_last(); D.warm_start_last_device()
        rh = H.solve(); out = D.solve_device()
        compare(D, out, rh, "band fleet, step 2")
        assert H.factor_layout() == D.factor_layout() == solver.K_BAND      # a function of the pattern: unchanged by the calls
    finally:
        H.close(); D.close()


SCENARIOS = {
    "bit_parity_with_the_host_path[10]": functools.partial(bit_parity_with_the_host_path, 10),
    "bit_parity_with_the_host_path[0]": functools.partial(bit_parity_with_the_host_path, 0),
    "parity_with_fresh_oracles": parity_with_fresh_oracles,
    "mixed_calls_and_streams": mixed_calls_and_streams,
    "host_side_refusals_launch_nothing": host_side_refusals_launch_nothing,
    "accounting": accounting,
    "a_band_layout_fleet[10]": functools.partial(a_band_layout_fleet, 10),
    "a_band_layout_fleet[0]": functools.partial(a_band_layout_fleet, 0),
}


def main():
    out = {}
    for name, run in SCENARIOS.items():
        try:
            run()
            out[name] = "ok"
        except AssertionError:                      # a failed check: recorded, the other scenarios still run
            out[name] = traceback.format_exc()[-3000:]
        except Exception:                           # anything else may be a device error: nothing more is started on the GPU
            out[name] = traceback.format_exc()[-3000:]
            for rest in SCENARIOS:
                out.setdefault(rest, "not run: '%s' ended with an error" % name)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f)
        if len(out) == len(SCENARIOS):
            break


if __name__ == "__main__":
    main()
