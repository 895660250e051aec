"""New fleet matrix values from device arrays (qpdo_amd_fleet_update_matrices_dev, include/qpdo_amd_ext.h) where no device is needed: the
packed value layout is host arithmetic (the cumulative sums of the stored entry counts, either itype), the new calls on a NULL fleet are
refused by the host driver under their own names, solver.pack_matrix_values -- a function of the problems' host images -- lays the values
out in the create-time order for every stype, and Fleet.update_matrices_device validates its tensors before any library call.  The C-side
checks again from a compiled C program with the host driver under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from qpdo_amd import _build, problems, solver


def last_error():
    return (solver.lib().qpdo_amd_last_error() or b"").decode()


def stored(Qf, st):
    """the storage of the full symmetric Qf for stype st (the with_stype idea of tests/test_gpu_fleet_matrices.py)"""
    Qf = sp.csc_matrix(Qf)
    if st == 0:
        return Qf
    coo = Qf.tocoo()
    keep = coo.row >= coo.col if st < 0 else coo.row <= coo.col
    return sp.csc_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=Qf.shape)


def with_stype(p, st):
    return dict(p, Q=stored(problems.full_Q(p), st), Qstype=st)


def layout_problems():
    ps = (problems.infeasibility_kat("primal_infeasible"), problems.random_qp(21, 30, 0, 0.2), problems.random_qp(23, 40, 60, 0.2, 10))
    return [with_stype(p, (-1, 1, 0)[i % 3]) for i, p in enumerate(ps)]


def host_images(probs, index_dtype):
    """`count` QPDOData whose matrices carry the index type named, what they point into, and the matrices as the create path stores them"""
    keep, arr, mats = [], (C.POINTER(solver.QPDOData) * len(probs))(), []
    for i, p in enumerate(probs):
        A, Q = sp.csc_matrix(p["A"]), sp.csc_matrix(p["Q"])
        A.sort_indices(); Q.sort_indices()
        Qs, As = solver._sparse_view(Q, p["Qstype"], keep, index_dtype), solver._sparse_view(A, 0, keep, index_dtype)
        d = solver.QPDOData()
        d.n, d.m, d.Q, d.A = A.shape[1], A.shape[0], C.pointer(Qs), C.pointer(As)
        keep.extend([Qs, As, d])
        arr[i] = C.pointer(d)
        mats.append((Q, A))
    return arr, keep, mats


@pytest.mark.parametrize("index_dtype", [np.int32, np.int64], ids=["CHOLMOD_INT", "CHOLMOD_LONG"])
def test_packed_matrix_layout_is_the_cumulative_sums_of_the_stored_entries(index_dtype, monkeypatch):
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):      # (a call that reached a device would fail)
        monkeypatch.setenv(v, "-1")
    L = solver.lib()
    probs = layout_problems()
    count = len(probs)
    arr, keep, mats = host_images(probs, index_dtype)
    assert all(arr[i].contents.Q.contents.itype == arr[i].contents.A.contents.itype == (2 if index_dtype == np.int64 else 0) for i in range(count))
    qo, ao = (C.c_long * (count + 1))(), (C.c_long * (count + 1))()
    assert L.qpdo_amd_fleet_packed_matrix_layout(count, arr, qo, ao) == 0, last_error()
    nq, na = [Q.nnz for Q, _ in mats], [A.nnz for _, A in mats]
    assert [p["Qstype"] for p in probs] == [-1, 1, 0] and na[1] == 0 and probs[1]["m"] == 0
    assert nq[2] == problems.full_Q(probs[2]).nnz and nq[1] < problems.full_Q(probs[1]).nnz      # full storage / one triangle
    assert qo[:] == [0] + np.cumsum(nq).tolist() and ao[:] == [0] + np.cumsum(na).tolist()
    assert ao[1] == ao[2]                                    # the m = 0 item occupies nothing
    name = "qpdo_amd_fleet_packed_matrix_layout"
    assert L.qpdo_amd_fleet_packed_matrix_layout(0, arr, qo, ao) != 0 and name + ": count must be positive" in last_error()
    assert L.qpdo_amd_fleet_packed_matrix_layout(count, None, qo, ao) != 0 and name + ": NULL data array" in last_error()
    assert L.qpdo_amd_fleet_packed_matrix_layout(count, arr, None, ao) != 0 and name + ": NULL output" in last_error()
    assert L.qpdo_amd_fleet_packed_matrix_layout(count, arr, qo, None) != 0 and name + ": NULL output" in last_error()


def test_the_new_calls_on_a_null_fleet_are_refused():
    L = solver.lib()
    one = (C.c_long * 2)()
    calls = dict(
        qpdo_amd_fleet_get_packed_matrix_layout=lambda: L.qpdo_amd_fleet_get_packed_matrix_layout(None, one, one),
        qpdo_amd_fleet_update_matrices_dev=lambda: L.qpdo_amd_fleet_update_matrices_dev(None, None, None, None, 0, 0, None))
    for name, call in calls.items():
        assert call() != 0 and last_error() == name + ": NULL fleet", (name, last_error())
    assert set(calls) <= set(solver.EXT_SYMBOLS) and "qpdo_amd_fleet_packed_matrix_layout" in solver.EXT_SYMBOLS
    for name in calls:
        assert hasattr(L, name)


def new_values(M, seed):
    M = sp.csc_matrix(M, copy=True)
    M.sort_indices()
    M.data = np.random.default_rng(seed).standard_normal(len(M.data))
    return M


def test_pack_matrix_values_lays_the_values_out_in_the_create_time_order():
    probs = layout_problems()
    count = len(probs)
    dims, qstype = [(p["n"], p["m"]) for p in probs], [p["Qstype"] for p in probs]
    arr, keep, mats = host_images(probs, np.int32)
    qo, ao = (C.c_long * (count + 1))(), (C.c_long * (count + 1))()
    assert solver.lib().qpdo_amd_fleet_packed_matrix_layout(count, arr, qo, ao) == 0
    qoff, aoff = np.array(qo[:]), np.array(ao[:])
    # at the layout's offsets: the .data of the matrices as the create path stores them (sorted CSC of the caller's storage), per stype
    Qn = [new_values(Q, 10 + i) for i, (Q, _) in enumerate(mats)]
    An = [new_values(A, 20 + i) for i, (_, A) in enumerate(mats)]
    qv, av, mask = solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=Qn, A=An)
    assert qv.dtype == av.dtype == np.float64 and mask.dtype == np.int32 and len(qv) == qoff[-1] and len(av) == aoff[-1]
    for i in range(count):
        assert np.array_equal(qv[qoff[i]:qoff[i + 1]], Qn[i].data) and np.array_equal(av[aoff[i]:aoff[i + 1]], An[i].data), i
    assert mask.tolist() == [3, 3, 3]
    # unsorted input: the packed order is still the create path's (sorted row indices within a column)
    rev = Qn[2].copy()
    for j in range(rev.shape[1]):
        s, e = rev.indptr[j], rev.indptr[j + 1]
        rev.indices[s:e], rev.data[s:e] = rev.indices[s:e][::-1].copy(), rev.data[s:e][::-1].copy()
    rev.has_sorted_indices = False
    assert not np.array_equal(rev.data, Qn[2].data)
    # ... and packing a matrix whose values are their own indices gives the index map from the caller's ordering
    own, numbered = rev.data.copy(), rev.copy()
    numbered.data = np.arange(numbered.nnz, dtype=np.float64)
    numbered.has_sorted_indices = False
    imap = solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=[None, None, numbered])[0][qoff[2]:].astype(np.int64)
    assert np.array_equal(own[imap], Qn[2].data)
    qv2, _, _ = solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=[None, None, rev])
    assert np.array_equal(qv2[qoff[2]:], Qn[2].data) and not qv2[:qoff[2]].any()
    # the mask follows the None pattern; items without an entry keep zeros; a None list gives None
    qv, av, mask = solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=[Qn[0], None, None], A=[None, An[1], An[2]])
    assert mask.tolist() == [1, 2, 2]
    assert np.array_equal(qv[:qoff[1]], Qn[0].data) and not qv[qoff[1]:].any()
    assert not av[:aoff[2]].any() and np.array_equal(av[aoff[2]:], An[2].data)
    qv, av, mask = solver.pack_matrix_values(dims, qstype, qoff, aoff, A=[An[0], None, None])
    assert qv is None and mask.tolist() == [2, 0, 0] and np.array_equal(av[:aoff[1]], An[0].data)
    qv, av, mask = solver.pack_matrix_values(dims, qstype, qoff, aoff)
    assert qv is None and av is None and mask.tolist() == [0, 0, 0]
    # refusals name the argument
    with pytest.raises(ValueError, match="^Q: expected a list of 3 matrices, got 2"):
        solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=Qn[:2])
    with pytest.raises(ValueError, match="^A: expected a list of 3 matrices, got 1"):
        solver.pack_matrix_values(dims, qstype, qoff, aoff, A=An[:1])
    with pytest.raises(ValueError, match=r"^Q\[0\]: expected shape \(2, 2\)"):
        solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=[sp.csc_matrix((3, 3)), None, None])
    with pytest.raises(ValueError, match=r"^A\[2\]: expected shape \(60, 40\)"):
        solver.pack_matrix_values(dims, qstype, qoff, aoff, A=[None, None, sp.csc_matrix((60, 41))])
    fewer = Qn[2].copy()
    fewer.data[0] = 0.0
    fewer.eliminate_zeros()
    with pytest.raises(ValueError, match=r"^Q\[2\]: %d stored entries, the pattern at create has %d" % (Qn[2].nnz - 1, Qn[2].nnz)):
        solver.pack_matrix_values(dims, qstype, qoff, aoff, Q=[None, None, fewer])


def test_the_fleet_methods_go_through_the_same_function():
    """a Fleet object with no native fleet behind it: pack_matrix_values needs the cached layout alone"""
    probs = layout_problems()
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims, F._qstype = None, 3, [(p["n"], p["m"]) for p in probs], [p["Qstype"] for p in probs]
    nq = [sp.csc_matrix(p["Q"]).nnz for p in probs]
    na = [sp.csc_matrix(p["A"]).nnz for p in probs]
    F._mlayout = (np.array([0] + np.cumsum(nq).tolist()), np.array([0] + np.cumsum(na).tolist()))
    assert F.packed_matrix_layout() is F._mlayout            # cached
    Q1 = new_values(probs[1]["Q"], 3)
    qv, av, mask = F.pack_matrix_values(Q=[None, Q1, None])
    assert av is None and mask.tolist() == [0, 1, 0] and np.array_equal(qv[nq[0]:nq[0] + nq[1]], Q1.data)
    with pytest.raises(ValueError, match="^A: expected a list of 3"):
        F.pack_matrix_values(A=[])


def test_update_matrices_device_validates_before_any_library_call():
    """no GPU here: dtype and element count are checked before the device, so each refusal is reachable with CPU tensors; the (NULL)
    handle is never reached"""
    import torch
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims = None, 2, [(4, 3), (2, 0)]
    F._layout, F._device, F._dev_out = (np.array([0, 4, 6]), np.array([0, 3, 3])), 0, None
    F._mlayout = (np.array([0, 7, 9]), np.array([0, 5, 5]))
    with pytest.raises(ValueError, match="^Q_values: expected 9 elements"):
        F.update_matrices_device(Q_values=torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError, match="^Q_values: expected dtype float64, got torch.float32"):
        F.update_matrices_device(Q_values=torch.zeros(9, dtype=torch.float32))
    with pytest.raises(ValueError, match="^A_values: expected 5 elements"):
        F.update_matrices_device(A_values=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match="^A_values: expected dtype float64"):
        F.update_matrices_device(Q_values=None, A_values=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="^mask: expected dtype int32"):
        F.update_matrices_device(mask=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="^mask: expected 2 elements"):
        F.update_matrices_device(mask=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="^A_values: expected a tensor on the GPU"):
        F.update_matrices_device(A_values=torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError, match="^Q_values: expected a torch tensor"):
        F.update_matrices_device(Q_values=np.zeros(9))


def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="fleet_matrices_device_args_driver.c")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    if sanitize:
        supp = tmp_path / "lsan.supp"
        supp.write_text("leak:libhsa-runtime64\nleak:libamdhip64\nleak:librccl\n")
        env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
                   LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % supp)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    return out.returncode, out.stdout + out.stderr


def test_argument_checks_from_a_c_caller(tmp_path):
    rc, txt = run_driver(tmp_path, False)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """the host driver (qpdo_api.c) and the C caller with -fsanitize=address,undefined, as a stand-alone program on the CPU"""
    rc, txt = run_driver(tmp_path, True)
    assert rc == 0 and "all refused before any device call" in txt, txt[-3000:]
    assert "AddressSanitizer" not in txt and "runtime error" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
