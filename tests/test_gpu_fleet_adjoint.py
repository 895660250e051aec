"""The adjoint of a fleet's last solve on the device (qpdo_amd_fleet_adjoint_dev, solver.Fleet.adjoint_device, qpdo_amd.torch_layer.FleetQP;
k_small_fleet_adjoint).  The scenarios live in tests/_fleet_adjoint_worker.py and run ONCE, in one child process that imports torch before
the library is loaded (one HIP runtime in the process; tests/test_gpu_fleet_device.py).  Each test below reads one scenario's outcome.
  fleet P / B / G   a heterogeneous fleet in each layout of K (PACKED with both flags, BAND, GLOBAL), scaling 10 and 0: codes, flags against
                    the longdouble reference on every row with a margin, the residual and error bounds of the solve with the device's own
                    flags, placement of dl / du, dQ / dA against the formulas (P), a run with NaN in gy on the inactive rows
  not accepted      two identical active rows with gy differing on them: code 1 and NaN, the neighbours accepted; accepted with gy = None
  no bit moves      solve -> update -> warm_start_last -> solve -> update_matrices -> solve on three fleets, one with adjoint calls, in each
                    layout of K (GLOBAL: the adjoint overwrites the items' global work vectors and K buffer)
  refusals          before a solve, after an update, without the flags, wrong lengths, host pointers: nothing launched, no counter moved
  streams           the call on a side stream behind a solve on another, ordered by the fleet's event
  FleetQP           backward equals the direct call bit for bit; which inputs get gradients; "zero"; the stale backward
  parent bits       every output of the call on fleets P / B / G (both scalings, gy None and given, matrices off and on) hashes to what the
                    call delivered at the commit before this test (tests/golden/fleet_adjoint_parent_bits.json, recorded with
                    _fleet_adjoint_worker.py --record PATH on an MI355X): the anchor for any change to the kernel behind the call, or to which
                    kernel that is; a moved x or y of the SOLVE is reported as a stale recording, not as a changed adjoint"""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def outcomes(out_dir):
    out = os.path.join(out_dir, "fleet_adjoint.json")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_fleet_adjoint_worker.py")
    p = subprocess.run([sys.executable, worker, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(out), (p.stdout + p.stderr)[-3000:]
    with open(out) as f:
        res = json.load(f)
    print("fleet adjoint worker notes:", json.dumps(res.get("notes", {})))
    return res


@pytest.fixture(scope="module")
def scenario(gpu_required, tmp_path_factory):
    res = outcomes(str(tmp_path_factory.mktemp("fleet_adjoint")))
    return lambda name: res.get(name, "the worker did not run this scenario")


@pytest.mark.parametrize("scaling", [10, 0])
@pytest.mark.parametrize("name", ["P", "B", "G"], ids=["PACKED", "BAND", "GLOBAL"])
def test_adjoint_of_a_fleet(name, scaling, scenario):
    assert scenario("fleet_%s[%d]" % (name, scaling)) == "ok"


def test_an_inconsistent_system_is_not_accepted(scenario):
    assert scenario("not_accepted") == "ok"


@pytest.mark.parametrize("name", ["P", "B", "G"], ids=["PACKED", "BAND", "GLOBAL"])
def test_no_bit_of_any_solve_moves(name, scenario):
    assert scenario("no_bit_moves[%s]" % name) == "ok"


def test_refusals_launch_nothing(scenario):
    assert scenario("refusals_launch_nothing") == "ok"


def test_the_call_on_a_side_stream(scenario):
    assert scenario("streams") == "ok"


def test_fleet_qp_layer(scenario):
    assert scenario("fleet_qp_layer") == "ok"


def test_the_single_call_keeps_its_recorded_bits(scenario):
    assert scenario("parent_bits") == "ok"
