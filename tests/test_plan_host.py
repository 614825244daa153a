"""The search planner without a GPU (tls_amd/csrc/tls_plan.hip.h): tls_period_costs against pins recorded before the plan
became one value that tls_prepare, enqueue, tls_plan_info and the cost model share (tools/period_costs_pins.py wrote
tests/golden/period_costs_pins.npz), and the planner's own invariants over a sweep of inputs, in a stand-alone host
program built with the address and undefined-behaviour sanitizers (tests/host/plan_sweep.hip)."""
import importlib.util
import os
import shutil
import subprocess

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pins_tool():
    spec = importlib.util.spec_from_file_location("period_costs_pins", os.path.join(ROOT, "tools", "period_costs_pins.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_period_costs_are_the_recorded_ones():
    """Trial cells and workgroups in flight exactly, expected taps and modelled times to a relative 1e-12 (erfc, exp and
    sqrt are the machine's libm; the wrong kernel family changes a time by percent) -- on either side of every
    uniform-weight edge of the plan, two slab plans, four noise levels (one between the two pruning thresholds, where the
    cost model and the launch disagree on purpose: DESIGN.md section 8) and seven switch sets."""
    tool = _pins_tool()
    pins = numpy.load(tool.FIXTURE)
    cases = tool.cases()
    assert [name for name, _ in cases] == [str(name) for name in pins["names"]]
    for i, (name, inp) in enumerate(cases):
        sigmas = tool.sigmas_of(inp)
        numpy.testing.assert_allclose(sigmas, pins["sigmas"][i], rtol=1e-9, err_msg=name)
        cells, taps, time, slots = tool.compute(inp, list(pins["sigmas"][i]))
        numpy.testing.assert_array_equal(cells, pins["cells_%d" % i], err_msg=name)
        numpy.testing.assert_array_equal(slots, pins["slots_%d" % i], err_msg=name)
        numpy.testing.assert_allclose(taps, pins["taps_%d" % i], rtol=1e-12, atol=0, err_msg=name)
        numpy.testing.assert_allclose(time, pins["time_%d" % i], rtol=1e-12, atol=0, err_msg=name)


def test_planner_sweep_under_sanitizers(tmp_path):
    """plan_search and pick_kernel over series of 100 to 200 000 points, both weight structures, three width tables, four
    period counts and the switch sets of the pins: every plan within the LDS, its tiles and lists sized as the kernels
    index them, the four-slot kernel picked only where the plan fits it.  Host code only: no device, nothing preloaded."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the planner sweep is part of the suite")
    exe = str(tmp_path / "plan_sweep")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host", "plan_sweep.hip")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "plans checked" in run.stdout
