"""Many right-hand sides per factorization on a fleet's last solve (qpdo_amd_fleet_adjoint_multi_dev, qpdo_amd_fleet_tangent_dev;
solver.Fleet.adjoint_many_device / tangent_device; FleetQP.tangent / vjp_many; k_small_fleet_sens).  The scenarios live in
tests/_fleet_sensitivity_worker.py and run ONCE, in one child process that imports torch before the library is loaded
(tests/test_gpu_fleet_device.py).  Each test below reads one scenario's outcome.  nrhs takes 1, 2, G, G + 1 and 2G + 3 with G = rhs_group().
  adjoint bits      per fleet (PACKED, BAND, GLOBAL), scaling 10 and 0, with and without gy, with and without matrices: every output slab of
                    adjoint_many_device, status and residual included, equals adjoint_device with that slab as a bit pattern
  refused alone     right-hand sides alternating between a consistent and an inconsistent gy on an item with a duplicated row: codes 0 / 1
  tangent           against the longdouble reference with the device's flags: residual and error bounds, dy off S, NaN on unused rows
  duality           <g, d> = <v, r> between the adjoint's and the tangent's results within the bound their own residuals give
  no bit moves      three fleets through solve, update, warm start, matrix update; one with a tangent and a multi-adjoint after every solve
  refusals          nothing launched, no counter moved
  streams           the calls on a side stream behind a solve on another
  FleetQP           tangent / vjp_many equal the Fleet calls bit for bit; "zero"; stale calls raise"""
import functools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def outcomes(out_dir):
    out = os.path.join(out_dir, "fleet_sensitivity.json")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_fleet_sensitivity_worker.py")
    p = subprocess.run([sys.executable, worker, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(out), (p.stdout + p.stderr)[-3000:]
    with open(out) as f:
        res = json.load(f)
    print("fleet sensitivity worker notes:", json.dumps(res.get("notes", {})))
    return res


@pytest.fixture(scope="module")
def scenario(gpu_required, tmp_path_factory):
    res = outcomes(str(tmp_path_factory.mktemp("fleet_sensitivity")))
    return lambda name: res.get(name, "the worker did not run this scenario")


LAYOUTS = pytest.mark.parametrize("name", ["P", "B", "G"], ids=["PACKED", "BAND", "GLOBAL"])


@pytest.mark.parametrize("scaling", [10, 0])
@LAYOUTS
def test_adjoint_slabs_carry_the_single_calls_bits(name, scaling, scenario):
    assert scenario("adjoint_bits_%s[%d]" % (name, scaling)) == "ok"


def test_a_refused_right_hand_side_stays_alone(scenario):
    assert scenario("refused_alone") == "ok"


@pytest.mark.parametrize("scaling", [10, 0])
@LAYOUTS
def test_tangent_against_the_longdouble_reference(name, scaling, scenario):
    assert scenario("tangent_%s[%d]" % (name, scaling)) == "ok"


@LAYOUTS
def test_duality_of_adjoint_and_tangent(name, scenario):
    assert scenario("duality[%s]" % name) == "ok"


@LAYOUTS
def test_no_bit_of_any_solve_moves(name, scenario):
    assert scenario("no_bit_moves[%s]" % name) == "ok"


def test_refusals_launch_nothing(scenario):
    assert scenario("refusals_launch_nothing") == "ok"


def test_the_calls_on_a_side_stream(scenario):
    assert scenario("streams") == "ok"


def test_fleet_qp_layer(scenario):
    assert scenario("fleet_qp_layer") == "ok"
