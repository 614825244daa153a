"""The four-slot kernel's dot products with the template taps broadcast from lanes ("Where the taps
live"; slim_dot_windows in tls_kernels.hip.h).

The change moved the taps of phase 3b from SGPRs (scalar loads) into one VGPR pair per 16 taps, read by the FMAs through
DPP row broadcasts; the FMAs, their operands and their order per accumulator are the parent's, so every bit of
(chi2, row, depth) and the counters of the work done, `evaluated_cells` and `inner_steps`, must be the parent's.  tests/golden/slim_tap_broadcast_parent.npz holds them as
the PARENT commit's kernel computed them on an MI355X for the cases below (tools/record_slim_tap_broadcast.py ran this
module's CASES against the parent's library); every comparison is byte equality.

`issued_fma` is recorded too but cannot be compared for equality: it counts the lane-FMAs of the batches as they were FORMED,
and which units of a row fall into its partly filled last batch -- re-listed window by window when it is short -- follows the
order in which the waves pushed their live units (push_live: "order inside a list is irrelevant").  Two recordings with the
parent's own library differ in it (PERF_LOG.md, "template taps broadcast from lanes": 5 of the 9 counting cases, by up to
0.16 %), so it is checked for what does hold in every run: whole waves of whole steps, and no less than `inner_steps`.

Cases, uniform weights, 24-64 periods each:
  default rows at N = 720 and 1459 (rows of one step and of >= 3 steps: the tap pairs rotate);
  T0_fit_margin raised so that rows run at strides 2, 3, 4, 5 (compile-time tap offsets, two pairs from 3 on) and above 5
    (the run-time form) -- asserted on the table's widths;
  noise levels at which some rows keep <= 20 live units and others > 64 (re-listed one-window batches, a partly filled
    last batch) -- asserted on the kernel's own row statistics;
  5200 points (the 512-thread shape) and 4800 (three slots a CU);
  a survey group of 3 curves through search_batch;
  one period that notes band windows (the outlier construction of test_perm_table.py)."""
import importlib.util
import os

import numpy
import pytest

from search_spec import stride
from tls_amd import synthetic

FORCE_SLIM = dict(slim=1, prune=0, screen32=0)   # the four-slot kernel where the host would take a classic variant
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slim_tap_broadcast_parent.npz")
COUNTERS = ("evaluated_cells", "inner_steps", "issued_fma")
_CACHE = {}


def _series(n, sigma=60e-6, seed=0):
    """n points at 30-minute cadence with a planet of 2.345 d."""
    t, flux = synthetic.light_curve((n + 0.5) / 48.0, 48, sigma, seed=seed, per=2.345, rp=0.03, a=9)
    assert len(t) == n
    return t, flux


def _inputs(n, sigma=60e-6, seed=0, **kw):
    key = (n, sigma, seed, tuple(sorted(kw.items())))
    if key not in _CACHE:
        t, flux = _series(n, sigma, seed)
        _CACHE[key] = synthetic.search_inputs(t, flux, **kw)
    return _CACHE[key]


def _periods(inp, count):
    grid = inp["periods"]
    return numpy.ascontiguousarray(numpy.linspace(grid[0], grid[-1], count))


def _strides(inp):
    return sorted({stride(int(w), inp["params"]["T0_fit_margin"]) for w in inp["table"].width})


def _search(gpu, inp, periods, kernel="slim"):
    gpu.set_options(**FORCE_SLIM)
    got = gpu.search(inp["t"], inp["y"], inp["dy"], periods, inp["table"], inp["params"], count_work=True)
    assert gpu.last_kernel() == kernel, gpu.last_kernel()
    plain = gpu.search(inp["t"], inp["y"], inp["dy"], periods, inp["table"], inp["params"])
    assert gpu.last_kernel() == kernel
    for a, b in zip(plain[:3], got[:3]):
        assert a.tobytes() == b.tobytes(), "the plain instantiation against the counting one"
    return got[0], got[1], got[2], numpy.asarray([got[3][k] for k in COUNTERS], dtype=numpy.int64)


def case_default_rows(gpu, n):
    inp = _inputs(n)
    assert _strides(inp) == [1]
    return _search(gpu, inp, _periods(inp, 48))


# (n, T0_fit_margin): stride int(width * margin) of the table's widths
MARGINS = {"720": (720, 0.08), "1459": (1459, 0.05)}


def case_strides(gpu, which):
    n, margin = MARGINS[which]
    inp = _inputs(n, T0_fit_margin=margin)
    have = _strides(inp)
    assert set(have) >= {1, 2, 3, 4, 5} and max(have) > 5, have        # every compile-time stride and the run-time form
    assert 8 * max(have) <= max(int(w) for w in inp["table"].width)   # (which is still tiled: kR windows a lane)
    return _search(gpu, inp, _periods(inp, 32))


def case_live_units(gpu, n, sigma, want):
    """A noise level at which the depth predicate leaves rows a handful of live units (re-listed, one window a lane: `singles`)
    or more than a wave's (several batches a row, the last partly filled: `waves`)."""
    inp = _inputs(n, sigma=sigma)
    periods = _periods(inp, 24)
    out = _search(gpu, inp, periods)
    gpu.execute(phase_clock=True)
    stats = gpu.phase_cycles()
    rows = len(periods) * len(inp["table"].width)             # (at most: a period searches a range of the table's rows)
    print("sigma %g: %d kept units, %d re-listed positions, %d batches on at most %d rows"
          % (sigma, stats["stat_kept_units"], stats["stat_singles"], stats["stat_batches"], rows))
    if want == "singles":
        assert stats["stat_singles"] > 0, stats
    else:
        assert stats["stat_kept_units"] > 64 * rows and stats["stat_kept_units"] % 64 != 0, stats   # some row holds more than a wave
    return out


def case_shape(gpu, n, kernel):
    inp = _inputs(n)
    return _search(gpu, inp, _periods(inp, 24), kernel=kernel)


def case_survey_group(gpu):
    inputs = [_inputs(1459, seed=s) for s in range(3)]
    periods = _periods(inputs[0], 32)
    gpu.set_options(**FORCE_SLIM)
    ys, dys = numpy.stack([i["y"] for i in inputs]), numpy.stack([i["dy"] for i in inputs])
    chi2, row, depth = gpu.search_batch(inputs[0]["t"], ys, dys, periods, inputs[0]["table"], inputs[0]["params"])
    assert gpu.last_kernel() == "slim"
    return chi2, row, depth, numpy.zeros(len(COUNTERS), dtype=numpy.int64)   # (a group launch counts no work)


def case_band_windows(gpu):
    """One wild flux value widens the undecided band until windows fall inside: noted, then decided on the exact prefix sum."""
    base = _inputs(1459)
    y = base["y"].copy()
    y[137] = 3.0e4
    key = "band"
    if key not in _CACHE:
        _CACHE[key] = synthetic.search_inputs(base["t"], y)
    inp = _CACHE[key]
    periods = _periods(inp, 24)
    out = _search(gpu, inp, periods)
    gpu.execute(phase_clock=True)
    assert gpu.phase_cycles()["stat_exact_retries"] > 0, gpu.phase_cycles()
    return out


CASES = {
    "default_rows_720": lambda gpu: case_default_rows(gpu, 720),
    "default_rows_1459": lambda gpu: case_default_rows(gpu, 1459),
    "strides_720": lambda gpu: case_strides(gpu, "720"),
    "strides_1459": lambda gpu: case_strides(gpu, "1459"),
    "live_units_1459_quiet": lambda gpu: case_live_units(gpu, 1459, 20e-6, "singles"),
    "live_units_1459_noisy": lambda gpu: case_live_units(gpu, 1459, 400e-6, "waves"),
    "threads512_5200": lambda gpu: case_shape(gpu, 5200, "slim512"),
    "three_slots_4800": lambda gpu: case_shape(gpu, 4800, "slim"),
    "survey_group_of_3": case_survey_group,
    "band_windows": case_band_windows,
}


def run_case(gpu, name):
    """(chi2, row, depth, counters) of a case, the context's switches put back."""
    try:
        return CASES[name](gpu)
    finally:
        gpu.set_options(**{k: None for k in FORCE_SLIM})


def test_the_asm_header_is_the_generators_output():
    """tls_slim_dot_asm.inc.h holds the loops' asm text; tools/gen_slim_dot_asm.py computes the tap indices in it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_slim_dot_asm", os.path.join(root, "tools", "gen_slim_dot_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(root, "tls_amd", "csrc", "tls_slim_dot_asm.inc.h")) as f:
        assert f.read() == gen.render()


@pytest.fixture(scope="module")
def golden():
    with numpy.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_parent(gpu, golden, name):
    got = run_case(gpu, name)
    for value, part in zip(got, ("chi2", "row", "depth", "counters")):
        want = golden["%s/%s" % (name, part)]
        value = numpy.ascontiguousarray(value)
        assert value.dtype == want.dtype and value.shape == want.shape, (name, part, value.dtype, want.dtype, value.shape, want.shape)
        if part == "counters":
            have, recorded = dict(zip(COUNTERS, value.tolist())), dict(zip(COUNTERS, want.tolist()))
            print("%s: counters %s, recorded at the parent %s" % (name, have, recorded))
            for key in ("evaluated_cells", "inner_steps"):
                assert have[key] == recorded[key], (name, key, have, recorded)
            assert have["issued_fma"] % (64 * 8) == 0 and have["issued_fma"] >= have["inner_steps"], (name, have)
        else:
            assert value.tobytes() == want.tobytes(), "%s: %s differs from the parent's bytes in %d of %d entries" % (
                name, part, int((value.view(numpy.int64) != want.view(numpy.int64)).sum()) if value.itemsize == 8 else -1, value.size)
