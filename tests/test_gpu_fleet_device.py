"""The fleet's device entry points (qpdo_amd_fleet_*_dev, fetch_last, sync; solver.Fleet.update_device / warm_start_device /
warm_start_last_device / solve_device): q, l, u, x0, y0 arrive as packed torch tensors on the GPU, the results leave as packed torch
tensors, everything is enqueued on torch's current stream.  The contract is the host calls' own: per item the same bits.

The scenarios live in tests/_fleet_device_worker.py and run ONCE, in one child process, because that is what they are about: a process
in which torch and libqpdo_amd.so share one HIP runtime, which needs torch imported before the library is loaded (a torch wheel bundles
its runtime) -- and this pytest process loaded the library in earlier tests.  Each test below reads one scenario's outcome.
  bit parity        two fleets from the same problems, one driven by the host calls, one by the device calls, three closed-loop steps (all
                    of q, l, u; a masked step; an explicit warm start with a y-less item): x, y, status, counts, norms, objective, NaN
                    placement and certificates bitwise equal after every solve; fetch_last equals the host solve field for field
  mixed             device update + host solve, host update + device solve, then a step on a side stream between two torch ops
  refused item      l > u on one item: counted, named, untouched; the others proceed
  host refusals     wrong lengths and host pointers are refused by name before any launch
  accounting        vector_bytes_uploaded_last_call, solve_launches, the device-call counters
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
    out = os.path.join(out_dir, "fleet_device.json")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_fleet_device_worker.py")
    p = subprocess.run([sys.executable, worker, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(out), (p.stdout + p.stderr)[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scenario(gpu_required, tmp_path_factory):
    res = outcomes(str(tmp_path_factory.mktemp("fleet_device")))
    return lambda name: res.get(name, "the worker did not run this scenario")


@pytest.mark.parametrize("scaling", [10, 0])
def test_bit_parity_with_the_host_path(scaling, scenario):
    assert scenario("bit_parity_with_the_host_path[%d]" % scaling) == "ok"


def test_mixed_calls_and_streams(scenario):
    assert scenario("mixed_calls_and_streams") == "ok"


def test_a_refused_item(scenario):
    assert scenario("a_refused_item") == "ok"


def test_host_side_refusals_launch_nothing(scenario):
    assert scenario("host_side_refusals_launch_nothing") == "ok"


def test_accounting(scenario):
    assert scenario("accounting") == "ok"


@pytest.mark.parametrize("scaling", [10, 0])
def test_a_band_layout_fleet(scaling, scenario):
    assert scenario("a_band_layout_fleet[%d]" % scaling) == "ok"
