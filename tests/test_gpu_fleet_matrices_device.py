"""New Q / A values for fleet items from device arrays on the caller's stream (qpdo_amd_fleet_update_matrices_dev,
solver.Fleet.pack_matrix_values / update_matrices_device; k_small_fleet_gather_matrices in front of the unchanged k_small_fleet_matrices).
The contract is the host call's own: an item given values from device memory is, bit for bit, the item qpdo_amd_fleet_update_matrices
leaves for the same values.

The scenarios live in tests/_fleet_matrices_device_worker.py and run ONCE, in one child process that imports torch before the library is
loaded (one HIP runtime in the process; tests/test_gpu_fleet_device.py).  Each test below reads one scenario's outcome.
  bit parity        two matrix_updates fleets from the same problems, H driven by the host calls, D by the device calls, through the call
                    pattern of tests/test_gpu_fleet_matrices.py::run_sequence plus a NULL-mask step and a Q-only step: x, y, status,
                    counts, norms, objective, NaN placement and certificates bitwise equal after every solve; fetch_last field for field
  fresh oracles     the device path against a new oracle per updated item
  mixed             device matrices + host update + device solve, host matrices + device update + host solve, a whole
                    real-time-iteration step on a side stream between two torch ops
  host refusals     wrong lengths, host pointers and a fleet without the flag are refused by name before any launch
  accounting        calls, items_last_call, value_bytes_uploaded_last_call, resident_extra_bytes, solve_launches
  band fleet        the same parity on a fleet in the K_BAND layout"""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def outcomes(out_dir):
    out = os.path.join(out_dir, "fleet_matrices_device.json")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_fleet_matrices_device_worker.py")
    p = subprocess.run([sys.executable, worker, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(out), (p.stdout + p.stderr)[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenario(gpu_required, tmp_path_factory):
    res = outcomes(str(tmp_path_factory.mktemp("fleet_matrices_device")))
    return lambda name: res.get(name, "the worker did not run this scenario")


@pytest.mark.parametrize("scaling", [10, 0])
def test_bit_parity_with_the_host_path(scaling, scenario):
    assert scenario("bit_parity_with_the_host_path[%d]" % scaling) == "ok"


def test_parity_with_fresh_oracles(scenario):
    assert scenario("parity_with_fresh_oracles") == "ok"


def test_mixed_calls_and_streams(scenario):
    assert scenario("mixed_calls_and_streams") == "ok"


def test_host_side_refusals_launch_nothing(scenario):
    assert scenario("host_side_refusals_launch_nothing") == "ok"


def test_accounting(scenario):
    assert scenario("accounting") == "ok"


@pytest.mark.parametrize("scaling", [10, 0])
def test_a_band_layout_fleet(scaling, scenario):
    assert scenario("a_band_layout_fleet[%d]" % scaling) == "ok"
