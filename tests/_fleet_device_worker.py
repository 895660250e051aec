"""Child process of tests/test_gpu_fleet_device.py: the scenarios of the fleet's device entry points (qpdo_amd_fleet_*_dev, fetch_last, sync;
solver.Fleet.update_device / warm_start_device / warm_start_last_device / solve_device), each run once, their outcomes written as JSON.
A process of its own because torch comes FIRST here: a torch wheel bundles its HIP runtime, and the loader shares it with libqpdo_amd.so
only when torch was imported before the library is loaded -- the pytest process has loaded the library long before.

Every scenario drives one fleet through the host calls and a second one, built from the same problems, through the device calls on packed
GPU tensors, and compares bit patterns (int64 views: a NaN must be the same NaN in the same place).  The items are small and
heterogeneous on purpose -- n = 2 with both infeasible statuses, m = 0, equality rows, one C3 item: the offsets of the packed layout are
what can go wrong.
usage: _fleet_device_worker.py OUT.json"""
import functools
import json
import os
import sys
import traceback

import numpy as np
import torch  # noqa: F401  (before qpdo_amd loads its library: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from qpdo_amd import problems, solver  # noqa: E402

ST = dict(max_iter=1000, verbose=0)
NORMS = ("res_prim_norm", "res_dual_norm", "res_prim_in_norm", "res_dual_in_norm", "objective")


@functools.lru_cache(maxsize=None)
def fleet_problems():
    return (problems.infeasibility_kat("primal_infeasible"), problems.infeasibility_kat("dual_infeasible"),
            problems.random_qp(21, 30, 0, 0.2), problems.random_qp(23, 40, 60, 0.2, 10), problems.config_qp("C3", 0))


@functools.lru_cache(maxsize=None)
def band_problems():
    """the smallest chain item of tests/test_gpu_small_band.py (its shape A: n = 256, half-bandwidth 12) beside an m = 0 item"""
    return (problems.banded_random_qp(1, 256, 12), problems.random_qp(21, 30, 0, 0.2))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def bit_equal(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def pack(vecs):
    """list of per-item vectors -> one GPU tensor in the packed layout"""
    return torch.from_numpy(np.concatenate([np.asarray(v, np.float64) for v in vecs])).cuda()


def imask(vals):
    return torch.tensor(vals, dtype=torch.int32).cuda()


def finite(v):
    return np.nan_to_num(np.asarray(v, float), nan=0.0)


def compare(F, out, ref, what):
    """the tensors of solve_device against the per-item dicts of the host fleet's solve(): every field, bit for bit"""
    torch.cuda.synchronize()
    no, mo = F.packed_layout()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    bad = []
    for i, r in enumerate(ref):
        x, y = o["x"][no[i]:no[i + 1]], o["y"][mo[i]:mo[i + 1]]
        pc, dc = o["prim_inf_cert"][mo[i]:mo[i + 1]], o["dual_inf_cert"][no[i]:no[i + 1]]
        inf = r["info"]
        ok = (bit_equal(x, r["x"]) and bit_equal(y, r["y"]) and bit_equal(pc, r["prim_inf_cert"]) and bit_equal(dc, r["dual_inf_cert"])
              and o["status"][i].tolist() == [inf["status_val"], inf["iterations"], inf["oterations"]]
              and bit_equal(o["norms"][i], [inf[f] for f in NORMS]))
        if inf["status_val"] in (-3, -4):
            ok = ok and bool(np.isnan(x).all() and np.isnan(y).all())
        if not ok:
            bad.append((what, i, inf["status_val"], o["status"][i].tolist()))
    assert not bad, bad


def compare_host(a, b, what):
    """two lists of per-item dicts (solve() / fetch_last()): every field but the three wall-clock times"""
    assert len(a) == len(b)
    for i, (ra, rb) in enumerate(zip(a, b)):
        for f in ("status_val", "status", "iterations", "oterations"):
            assert ra["info"][f] == rb["info"][f], (what, i, f)
        for f in NORMS:
            assert bit_equal(ra["info"][f], rb["info"][f]), (what, i, f)
        for f in ("x", "y", "prim_inf_cert", "dual_inf_cert"):
            assert bit_equal(ra[f], rb[f]), (what, i, f)


def step_data(probs, k, rng):
    """q, l, u of control step k for every item (infinite bounds stay infinite: both paths clip them)"""
    q = [(1.0 + 0.1 * k) * p["q"] + 0.01 * rng.standard_normal(p["n"]) for p in probs]
    l = [p["l"] - 0.05 * k for p in probs]
    u = [p["u"] + 0.03 * k for p in probs]
    return q, l, u


def bit_parity_with_the_host_path(scaling):
    probs = list(fleet_problems())
    A, B = solver.Fleet(probs, scaling=scaling, **ST), solver.Fleet(probs, scaling=scaling, **ST)
    rng = np.random.default_rng(11)
    try:
        # 1: all of q, l, u
        q, l, u = step_data(probs, 1, rng)
        A.update(q, l, u); A.warm_start_last(); ra = A.solve()
        B.update_device(pack(q), pack(l), pack(u)); B.warm_start_last_device(); out = B.solve_device()
        compare(B, out, ra, "step 1")
        sts = [r["info"]["status_val"] for r in ra]
        assert sts[0] == -3 and sts[1] == -4 and sts[2:] == [1, 1, 1], sts          # both NaN rules and solved items are exercised
        compare_host(B.fetch_last(), ra, "fetch_last after step 1")
        # 2: masked -- odd items take only q, item 0 takes nothing, the others everything
        q, l, u = step_data(probs, 2, rng)
        hq = [None if i == 0 else v for i, v in enumerate(q)]
        hl = [None if (i == 0 or i % 2) else v for i, v in enumerate(l)]
        hu = [None if (i == 0 or i % 2) else v for i, v in enumerate(u)]
        A.update(hq, hl, hu); A.warm_start_last(); ra = A.solve()
        B.update_device(pack(q), pack(l), pack(u), mask=imask([0 if i == 0 else (1 if i % 2 else 7) for i in range(len(probs))]))
        B.warm_start_last_device(); out = B.solve_device()
        compare(B, out, ra, "step 2 (masked)")
        # 3: an explicit warm start with a y-less item, then new q
        xw = [finite(r["x"]) + 1e-3 * rng.standard_normal(p["n"]) for r, p in zip(ra, probs)]
        yw = [finite(r["y"]) + 1e-3 * rng.standard_normal(p["m"]) for r, p in zip(ra, probs)]
        q, _, _ = step_data(probs, 3, rng)
        A.warm_start(xw, [None if i == 3 else v for i, v in enumerate(yw)]); A.update(q=q); ra = A.solve()
        B.warm_start_device(pack(xw), pack(yw), mask=imask([1 if i == 3 else 3 for i in range(len(probs))]))
        B.update_device(q=pack(q)); out = B.solve_device()
        compare(B, out, ra, "step 3 (explicit warm start)")
        compare_host(B.fetch_last(), ra, "fetch_last after step 3")
    finally:
        A.close(); B.close()


def mixed_calls_and_streams():
    probs = list(fleet_problems())
    A, B = solver.Fleet(probs, scaling=10, **ST), solver.Fleet(probs, scaling=10, **ST)
    rng = np.random.default_rng(12)
    try:
        q, l, u = step_data(probs, 1, rng)                   # a device update, then a host solve
        A.update(q, l, u); ra = A.solve()
        B.update_device(pack(q), pack(l), pack(u)); rb = B.solve()
        compare_host(rb, ra, "device update, host solve")
        q, l, u = step_data(probs, 2, rng)                   # a host update, then a device solve
        A.update(q, l, u); A.warm_start_last(); ra = A.solve()
        B.update(q, l, u); B.warm_start_last_device(); out = B.solve_device()
        compare(B, out, ra, "host update, device solve")
        # the same step on a stream of the caller's: q made by a torch op on it right before, x read by one right after, no wait between
        base = pack(step_data(probs, 3, rng)[0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        own = {k: torch.empty_like(v) for k, v in out.items()}
        with torch.cuda.stream(s):
            qt = base * 1.25 + 0.01
            B.update_device(q=qt); B.warm_start_last_device(); out = B.solve_device(out=own)
            twice = out["x"] * 2.0
        s.synchronize()
        assert all(out[k] is own[k] for k in own)
        no, _ = B.packed_layout()
        qh = qt.cpu().numpy()
        A.update(q=[qh[no[i]:no[i + 1]] for i in range(len(probs))]); A.warm_start_last(); ra = A.solve()
        compare(B, out, ra, "on a side stream")
        assert np.array_equal(twice.cpu().numpy(), 2.0 * np.concatenate([r["x"] for r in ra]), equal_nan=True)
        assert np.isfinite(twice.cpu().numpy()[no[2]:]).all()
    finally:
        A.close(); B.close()


def a_refused_item():
    probs, k = list(fleet_problems()), 3
    A, B = solver.Fleet(probs, scaling=10, **ST), solver.Fleet(probs, scaling=10, **ST)
    rng = np.random.default_rng(13)
    try:
        A.solve(); B.solve_device()
        assert B.sync()["refused_items"] == 0
        q, l, u = step_data(probs, 1, rng)
        lbad = [v.copy() for v in l]
        lbad[k][5] = u[k][5] + 1.0
        B.update_device(pack(q), pack(lbad), pack(u))
        s = B.sync()
        assert (s["refused_items"], s["first_refused_item"], s["update_calls"]) == (1, k, 1), s
        drop = lambda v: [None if i == k else w for i, w in enumerate(v)]       # item k: as on a fleet that never received the update
        A.update(drop(q), drop(l), drop(u))
        A.warm_start_last(); ra = A.solve()
        B.warm_start_last_device(); out = B.solve_device()
        compare(B, out, ra, "after the refused update")
        s = B.sync()
        assert (s["refused_items"], s["first_refused_item"]) == (0, -1), s
    finally:
        A.close(); B.close()


def host_side_refusals_launch_nothing():
    probs = list(fleet_problems())
    A, B = solver.Fleet(probs, scaling=10, **ST), solver.Fleet(probs, scaling=10, **ST)
    L = solver.lib()
    err = lambda: (L.qpdo_amd_last_error() or b"").decode()
    try:
        ra = A.solve(); B.solve()
        no, mo = B.packed_layout()
        N, M = int(no[-1]), int(mo[-1])
        q = pack([p["q"] for p in probs])
        qhost = np.concatenate([p["q"] for p in probs])
        before, dev_before = B.stats(), B.sync()
        assert L.qpdo_amd_fleet_update_dev(B._h, q.data_ptr(), None, None, None, N + 1, M, None) != 0 and "n_len" in err()
        assert L.qpdo_amd_fleet_update_dev(B._h, q.data_ptr(), None, None, None, N, M - 1, None) != 0 and "m_len" in err()
        assert L.qpdo_amd_fleet_update_dev(B._h, qhost.ctypes.data, None, None, None, N, M, None) != 0
        assert "qpdo_amd_fleet_update_dev: q is not device memory" in err()
        assert L.qpdo_amd_fleet_warm_start_dev(B._h, None, qhost.ctypes.data, None, N, M, None) != 0 and "y0 is not device memory" in err()
        assert L.qpdo_amd_fleet_solve_dev(B._h, None, None, None, qhost.ctypes.data, None, None, N, M, None) != 0 and "norms is not device memory" in err()
        assert L.qpdo_amd_fleet_update_dev(B._h, None, None, None, None, N, M, None) == 0          # no array at all: nothing to do
        try:
            B.update_device(q=qhost)
            raise AssertionError("a numpy array passed the tensor validator")
        except ValueError as e:
            assert str(e).startswith("q: "), e
        assert B.stats() == before and B.sync() == dev_before
        q1 = [1.1 * p["q"] for p in probs]
        A.update(q=q1); A.warm_start_last(); ra = A.solve()
        B.update(q=q1); B.warm_start_last(); rb = B.solve()
        compare_host(rb, ra, "after the refused calls")
    finally:
        A.close(); B.close()


def accounting():
    probs = list(fleet_problems())[:4]
    F = solver.Fleet(probs, scaling=10, **ST)
    try:
        F.update(q=[p["q"] for p in probs])
        assert F.stats()["vector_bytes_uploaded_last_call"] > 0
        F.update_device(q=pack([p["q"] for p in probs]))
        assert F.stats()["vector_bytes_uploaded_last_call"] == 0
        F.warm_start([p["q"] for p in probs], None)
        assert F.stats()["vector_bytes_uploaded_last_call"] > 0
        F.warm_start_device(x=pack([p["q"] for p in probs]))
        assert F.stats()["vector_bytes_uploaded_last_call"] == 0
        s0 = F.stats()
        first = F.solve_device()
        s1 = F.stats()
        again = F.solve_device()
        s2 = F.stats()
        assert [s["solve_launches"] - s0["solve_launches"] for s in (s1, s2)] == [1, 2] and s2["solves"] - s0["solves"] == 2
        assert all(first[k] is again[k] for k in first)      # allocated once, reused
        d = F.sync()
        assert (d["update_calls"], d["warm_start_calls"], d["solve_calls"]) == (1, 1, 2), d
        assert F.stats()["last_kernel_seconds"] > 0.0
    finally:
        F.close()


def a_band_layout_fleet(scaling):
    probs = list(band_problems())
    A, B = solver.Fleet(probs, scaling=scaling, **ST), solver.Fleet(probs, scaling=scaling, **ST)
    rng = np.random.default_rng(14)
    try:
        assert A.factor_layout() == B.factor_layout() == solver.K_BAND
        A.solve(); B.solve_device()
        q, l, u = step_data(probs, 1, rng)
        A.update(q, l, u); A.warm_start_last(); ra = A.solve()
        B.update_device(pack(q), pack(l), pack(u)); B.warm_start_last_device(); out = B.solve_device()
        compare(B, out, ra, "band fleet")
        compare_host(B.fetch_last(), ra, "band fleet, fetch_last")
    finally:
        A.close(); B.close()


SCENARIOS = {
    "bit_parity_with_the_host_path[10]": functools.partial(bit_parity_with_the_host_path, 10),
    "bit_parity_with_the_host_path[0]": functools.partial(bit_parity_with_the_host_path, 0),
    "mixed_calls_and_streams": mixed_calls_and_streams,
    "a_refused_item": a_refused_item,
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
