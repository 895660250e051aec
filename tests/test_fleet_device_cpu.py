"""The fleet's device entry points (qpdo_amd_fleet_*_dev, include/qpdo_amd_ext.h) where no device is needed: the packed layout is host
arithmetic, every call on a NULL fleet is refused by the host driver under its own name, the Python mirror of QPDOAmdFleetDevStats has
the C layout, and solver.check_device_tensor -- the one check every tensor passes before any library call -- names what it refuses.
The C-side checks again from a compiled C program with the host driver under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from qpdo_amd import _build, problems, solver


def last_error():
    return (solver.lib().qpdo_amd_last_error() or b"").decode()


def test_packed_layout_is_the_cumulative_sums(monkeypatch):
    for v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):      # (a call that reached a device would fail)
        monkeypatch.setenv(v, "-1")
    L = solver.lib()
    probs = [problems.infeasibility_kat("primal_infeasible"), problems.random_qp(21, 30, 0, 0.2), problems.random_qp(3, 12, 20, 0.3),
             problems.random_qp(23, 40, 60, 0.2, 10)]
    img = solver.Batch(probs)
    count = len(probs)
    arr = (C.POINTER(solver.QPDOData) * count)(*[img.items[i].data for i in range(count)])
    no, mo = (C.c_long * (count + 1))(), (C.c_long * (count + 1))()
    assert L.qpdo_amd_fleet_packed_layout(count, arr, no, mo) == 0
    ns, ms = [p["n"] for p in probs], [p["m"] for p in probs]
    assert ms[1] == 0
    assert no[:] == [0] + np.cumsum(ns).tolist() and mo[:] == [0] + np.cumsum(ms).tolist()
    assert mo[1] == mo[2]                                    # the m = 0 item occupies nothing
    assert L.qpdo_amd_fleet_packed_layout(0, arr, no, mo) != 0 and "qpdo_amd_fleet_packed_layout: count must be positive" in last_error()
    assert L.qpdo_amd_fleet_packed_layout(count, None, no, mo) != 0 and "qpdo_amd_fleet_packed_layout: NULL data array" in last_error()
    assert L.qpdo_amd_fleet_packed_layout(count, arr, None, mo) != 0 and "qpdo_amd_fleet_packed_layout: NULL output" in last_error()


def test_calls_on_a_null_fleet_are_refused():
    L = solver.lib()
    one, info, s = (C.c_long * 2)(), (solver.QPDOInfo * 1)(), solver.FleetDevStats()
    calls = dict(
        qpdo_amd_fleet_get_packed_layout=lambda: L.qpdo_amd_fleet_get_packed_layout(None, one, one),
        qpdo_amd_fleet_update_dev=lambda: L.qpdo_amd_fleet_update_dev(None, None, None, None, None, 0, 0, None),
        qpdo_amd_fleet_warm_start_dev=lambda: L.qpdo_amd_fleet_warm_start_dev(None, None, None, None, 0, 0, None),
        qpdo_amd_fleet_warm_start_last_dev=lambda: L.qpdo_amd_fleet_warm_start_last_dev(None, None),
        qpdo_amd_fleet_solve_dev=lambda: L.qpdo_amd_fleet_solve_dev(None, None, None, None, None, None, None, 0, 0, None),
        qpdo_amd_fleet_fetch_last=lambda: L.qpdo_amd_fleet_fetch_last(None, None, None, info),
        qpdo_amd_fleet_sync=lambda: L.qpdo_amd_fleet_sync(None, C.byref(s)),
        qpdo_amd_fleet_device=lambda: L.qpdo_amd_fleet_device(None))
    for name, call in calls.items():
        assert call() != 0 and last_error() == name + ": NULL fleet", (name, last_error())
    assert set(calls) <= set(solver.EXT_SYMBOLS) and "qpdo_amd_fleet_packed_layout" in solver.EXT_SYMBOLS
    for name in calls:
        assert hasattr(L, name)


def test_dev_stats_mirror_has_the_c_layout():
    assert C.sizeof(solver.FleetDevStats) == 5 * 8
    assert [f for f, _ in solver.FleetDevStats._fields_] == ["update_calls", "warm_start_calls", "solve_calls", "refused_items", "first_refused_item"]


def test_the_tensor_validator_names_what_it_refuses():
    """no GPU here: dtype, contiguity and element count are checked before the device, so each refusal is reachable with CPU tensors"""
    import torch
    chk = solver.check_device_tensor
    assert chk("q", None, 0, "float64", 6) is None
    with pytest.raises(ValueError, match="^q: expected a tensor on the GPU"):
        chk("q", torch.zeros(6, dtype=torch.float64), 0, "float64", 6)
    with pytest.raises(ValueError, match="^l: expected dtype float64, got torch.float32"):
        chk("l", torch.zeros(6, dtype=torch.float32), 0, "float64", 6)
    with pytest.raises(ValueError, match="^u: the tensor is not contiguous"):
        chk("u", torch.zeros(12, dtype=torch.float64)[::2], 0, "float64", 6)
    with pytest.raises(ValueError, match="^x: expected 6 elements"):
        chk("x", torch.zeros(5, dtype=torch.float64), 0, "float64", 6)
    with pytest.raises(ValueError, match="^mask: expected dtype int32, got torch.int64"):
        chk("mask", torch.zeros(3, dtype=torch.int64), 0, "int32", 3)
    with pytest.raises(ValueError, match="^status: expected dtype int64"):
        chk("status", torch.zeros(9, dtype=torch.int32), 0, "int64", 9)
    with pytest.raises(ValueError, match="^q: expected a torch tensor"):
        chk("q", np.zeros(6), 0, "float64", 6)


def test_the_front_end_validates_before_any_library_call():
    """a Fleet object with no native fleet behind it: the methods must raise from the validator, never reach the (NULL) handle"""
    import torch
    F = solver.Fleet.__new__(solver.Fleet)
    F._h, F.count, F.dims = None, 2, [(4, 3), (2, 0)]
    F._layout, F._device, F._dev_out = (np.array([0, 4, 6]), np.array([0, 3, 3])), 0, None
    with pytest.raises(ValueError, match="^q: expected 6 elements"):
        F.update_device(q=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="^u: expected dtype float64"):
        F.update_device(u=torch.zeros(3, dtype=torch.float32))
    with pytest.raises(ValueError, match="^mask: expected dtype int32"):
        F.warm_start_device(mask=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="^y: expected a tensor on the GPU"):
        F.warm_start_device(y=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="^status: expected 6 elements"):
        F.solve_device(out=dict(status=torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="unknown keys"):
        F.solve_device(out=dict(z=None))


def run_driver(tmp_path, sanitize):
    exe = _build.build_abi_driver(str(tmp_path), sanitize=sanitize, driver="fleet_device_args_driver.c")
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
