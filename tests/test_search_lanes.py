"""Launch lanes ("Launch lanes"; switch `lanes`): back-to-back plain searches of a four-slot plan whose
table of folded orders is filled alternate between two streams with a buffer set each, so that search i+1 starts on the
compute units search i has already left.  The lanes change where a launch runs and never what it computes: every comparison
here is byte equality of (chi2, row, depth) with the same search alone on a fresh context, and the host-side lane counters
(`Context.lanes()`) say which lane the launches took.  Nothing here asserts a time except the bookkeeping of kernel_timing.

Shapes: the 720-point series (256 threads a workgroup) and the 5200-point one (512 threads) of test_slim_tap_broadcast.py.
Period counts: 4096 at 720 points and 1024 at 5200, a few rounds of the 1024 (512) resident workgroups, so that a launch
lasts several host enqueue times and lane B's launch is enqueued while lane A's still runs.  Checked once with
`rocprofv3 --kernel-trace` on an MI355X (tools/gpu_lane_trace.py 720:4096 and 5200:1024, tools/lane_trace_overlap.py): a
search takes 247 us at 720 points and 539 us at 5200 against 25 us a host enqueue under the profiler (10 us without it), and
19 of 19 launches of a run began before the one before it ended, by 221-269 us and 428-805 us (PERF_LOG.md, "two launch
lanes")."""
import contextlib
import time

import numpy
import pytest

from test_slim_tap_broadcast import FORCE_SLIM, _inputs, _periods
from tls_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

SHAPES = {"slim": (720, 4096), "slim512": (5200, 1024)}   # kernel: (points, periods)
_WANT = {}


@contextlib.contextmanager
def fresh_context(**switches):
    ctx = _lib.Context(0)
    try:
        ctx.set_options(**dict(FORCE_SLIM, **switches))
        yield ctx
        checked, counts = ctx.check_counts()   # (a checked build counts every violated device-side bound: none on either lane)
        assert not checked or not any(counts.values()), counts
    finally:
        ctx.close()


def _args(inp, periods):
    return (inp["t"], inp["y"], inp["dy"], periods, inp["table"], inp["params"])


def _case(kernel, seed=0):
    n, count = SHAPES[kernel]
    inp = _inputs(n, seed=seed)
    return inp, _periods(inp, count)


def _bytes(result):
    return tuple(numpy.ascontiguousarray(a).tobytes() for a in result[:3])


def _standalone(key, args, count_work=False):
    """One search alone on a fresh context: computed once per key, shared and left unchanged."""
    if key not in _WANT:
        with fresh_context() as ctx:
            got = ctx.search(*args, count_work=count_work)
            _WANT[key] = (_bytes(got), got[3] if count_work else None, ctx.last_kernel())
    return _WANT[key]


def _warm(ctx, args, kernel):
    """The filling launch and one reading launch: the next plain execute may overlap."""
    ctx.prepare(*args)
    ctx.execute()
    ctx.execute()
    assert ctx.last_kernel() == kernel and ctx.perm_table()["filled"]
    return ctx.lanes()


def _run(ctx, count):
    for _ in range(count):
        ctx.execute()


@pytest.mark.parametrize("lanes", [None, 0], ids=["lanes_on", "lanes_off"])
@pytest.mark.parametrize("kernel", list(SHAPES))
def test_repeated_searches(kernel, lanes):
    """After two warming executes, six executes in a row and a fetch equal one execute and a fetch; three of the six took
    lane B (none with lanes = 0)."""
    inp, periods = _case(kernel)
    args = _args(inp, periods)
    want = _standalone((kernel, 0), args)
    assert want[2] == kernel
    with fresh_context(lanes=lanes) as ctx:
        before = _warm(ctx, args, kernel)
        assert before["b"] == 0 and before["on"] == (lanes is None)
        _run(ctx, 6)
        assert _bytes(ctx.fetch()) == want[0]
        after = ctx.lanes()
        assert after["b"] - before["b"] == (3 if lanes is None else 0), (before, after)
        assert after["a"] - before["a"] == (3 if lanes is None else 6), (before, after)
        # an odd count leaves the latest result on lane A, an even one on lane B
        for count in (1, 2, 3):
            _run(ctx, count)
            assert _bytes(ctx.fetch()) == want[0], count


@pytest.mark.parametrize("kernel", list(SHAPES))
def test_streaming(kernel):
    """Three fluxes whose results differ, update_flux and execute alternating: a fetch after each search, a fetch only at the
    end, and u(A) e u(B) e with no fetch between, each returns the LAST flux's standalone bytes.  Ten times over, so that an
    older launch has the chance to finish last."""
    cases = [_case(kernel, seed) for seed in (0, 1, 2)]
    wants = [_standalone((kernel, seed), _args(*cases[seed]))[0] for seed in (0, 1, 2)]
    assert len(set(wants)) == 3
    with fresh_context() as ctx:
        _warm(ctx, _args(*cases[0]), kernel)
        for rep in range(10):
            for (inp, _), want in zip(cases, wants):
                ctx.update_flux(inp["y"], inp["dy"])
                ctx.execute()
                assert _bytes(ctx.fetch()) == want, rep
            before = ctx.lanes()
            for inp, _ in cases:
                ctx.update_flux(inp["y"], inp["dy"])
                ctx.execute()
            assert _bytes(ctx.fetch()) == wants[2], rep
            for which in (0, 1):
                ctx.update_flux(cases[which][0]["y"], cases[which][0]["dy"])
                ctx.execute()
            assert _bytes(ctx.fetch()) == wants[1], rep
            after = ctx.lanes()
            # (the first search behind a fetch takes lane A; then B, A | A, B)
            assert after["b"] - before["b"] == 2 and after["a"] - before["a"] == 3, (before, after)
        # searches with and without a new flux between them, in one run
        ctx.update_flux(cases[2][0]["y"], cases[2][0]["dy"])
        _run(ctx, 2)
        ctx.update_flux(cases[0][0]["y"], cases[0][0]["dy"])
        _run(ctx, 3)
        ctx.update_flux(cases[1][0]["y"], cases[1][0]["dy"])
        _run(ctx, 2)
        assert _bytes(ctx.fetch()) == wants[1]


def test_band_resolution_on_both_lanes():
    """The outlier flux of test_perm_table.py notes band windows on a reading launch: the period's order is stashed per
    workgroup and its windows listed in the band list, both of them per lane."""
    from test_gpu_parity import _inputs as config_inputs
    inp = config_inputs("k2_90d")
    y = inp["y"].copy()
    y[137] = 3.0e4
    inp = synthetic.search_inputs(inp["t"], y, None, **synthetic.config("k2_90d")[2])
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::7]))
    want = _standalone(("band", 0), args)
    assert want[2] == "slim"
    with fresh_context() as ctx:
        before = _warm(ctx, args, "slim")
        for count in (3, 4):   # the latest launch on lane A, on lane B
            _run(ctx, count)
            assert _bytes(ctx.fetch()) == want[0], count
        after = ctx.lanes()
        assert after["b"] - before["b"] == 3, (before, after)
        ctx.execute(phase_clock=True)
        assert ctx.phase_cycles()["stat_exact_retries"] > 0
        assert _bytes(ctx.fetch()) == want[0]
        assert ctx.lanes()["b"] == after["b"]


def test_ineligible_launches_join():
    """A counting execute, execute_timed, a prepare with another period grid (the table refills) and power() behind an
    overlapped run: each equals the same call on a fresh context, and none of them goes to lane B."""
    import tls_amd
    inp, periods = _case("slim")
    args = _args(inp, periods)
    want = _standalone(("slim", 0), args)
    counted = _standalone(("slim", 0, "counting"), args, count_work=True)
    other = _args(inp, numpy.ascontiguousarray(periods[::3]))
    want_other = _standalone(("slim", 0, "other grid"), other)
    t, flux, kw = synthetic.config("k2_90d", seed=0)
    model = tls_amd.transitleastsquares(t, flux, verbose=False)
    with fresh_context() as ref:
        want_power = model.power(verbose=False, show_progress_bar=False, context=ref, **kw)
    with fresh_context() as ctx:
        _warm(ctx, args, "slim")

        def overlapped_run():
            before = ctx.lanes()
            _run(ctx, 4)
            after = ctx.lanes()
            assert after["b"] - before["b"] == 2, (before, after)
            return after["b"]

        lane_b = overlapped_run()
        ctx.execute(count_work=True)
        got = ctx.fetch(with_counters=True)
        assert _bytes(got) == counted[0] == want[0]
        for key, value in counted[1].items():
            if key != "issued_fma":   # (follows the order in which the waves pushed their units: PERF_LOG.md)
                assert got[3][key] == value, key
        assert ctx.lanes()["b"] == lane_b

        lane_b = overlapped_run()
        assert ctx.execute_timed(3) > 0
        assert _bytes(ctx.fetch()) == want[0]
        assert ctx.lanes()["b"] == lane_b

        lane_b = overlapped_run()
        ctx.prepare(*other)
        assert not ctx.perm_table()["filled"]
        for k in range(3):   # filling, reading, reading: the third may overlap but starts on lane A
            ctx.execute()
            assert _bytes(ctx.fetch()) == want_other[0], k
        assert ctx.lanes()["b"] == lane_b

        _warm(ctx, args, "slim")
        lane_b = overlapped_run()
        got_power = model.power(verbose=False, show_progress_bar=False, context=ctx, **kw)
        for key in ("chi2", "power", "SDE", "period", "T0", "depth", "duration", "chi2_min"):
            assert numpy.asarray(got_power[key]).tobytes() == numpy.asarray(want_power[key]).tobytes(), key
        assert ctx.lanes()["b"] == lane_b


@pytest.mark.parametrize("kernel", list(SHAPES))
def test_poisoned_lds_and_smeared_scratch(kernel):
    """LDS full of NaNs and both lanes' scratch smeared before an overlapped run: no launch reads what it has not written."""
    inp, periods = _case(kernel)
    args = _args(inp, periods)
    want = _standalone((kernel, 0), args)
    with fresh_context() as ctx:
        _warm(ctx, args, kernel)
        _run(ctx, 2)   # (lane B's buffers exist from here on)
        for count in (3, 4):
            ctx.poison_lds()
            before = ctx.lanes()
            _run(ctx, count)
            assert _bytes(ctx.fetch()) == want[0], count
            assert ctx.lanes()["b"] - before["b"] == count // 2


def test_kernel_timing_of_an_overlapped_run():
    """Six overlapped executes are six launches, every one charged more than nothing, and together no more than the run took
    (1.2: slack for the two synchronizations the wall clock includes, not a measured quantity)."""
    inp, periods = _case("slim512")
    args = _args(inp, periods)
    with fresh_context() as ctx:
        _warm(ctx, args, "slim512")
        _run(ctx, 4)
        ctx.kernel_timing(reset=True)
        ctx.synchronize()
        before = ctx.lanes()
        t0 = time.perf_counter()
        _run(ctx, 6)
        ctx.synchronize()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        assert ctx.lanes()["b"] - before["b"] == 3
        terms = ctx.launch_ms()
        total, launches = ctx.kernel_timing(reset=True)
        print("wall %.4f ms, kernel_timing %.4f ms over %d launches: %s" % (wall_ms, total, launches, terms))
        assert launches == 6 and len(terms) == 6
        assert all(ms > 0 for ms in terms), terms
        assert abs(float(numpy.sum(terms)) - total) <= 1e-9 * total
        assert total <= 1.2 * wall_ms, (total, wall_ms)


def test_switching_the_lanes_between_runs():
    """Changing `lanes` joins; the bytes do not change, and lane B gets launches only while the lanes are on."""
    inp, periods = _case("slim")
    args = _args(inp, periods)
    want = _standalone(("slim", 0), args)
    with fresh_context() as ctx:
        _warm(ctx, args, "slim")
        assert ctx.lanes()["on"]
        for lanes in (0, None, 0, None):
            before = ctx.lanes()
            _run(ctx, 3)                      # (left in flight: the switch below has to join them)
            ctx.set_options(lanes=lanes)
            assert ctx.perm_table()["filled"]  # (no planning switch: the plan and its table stay)
            _run(ctx, 4)
            assert _bytes(ctx.fetch()) == want[0], lanes
            after = ctx.lanes()
            assert after["on"] == (lanes is None)
            # three searches A, B, A with the lanes on, then four on lane A | three on lane A, then A, B, A, B
            assert after["b"] - before["b"] == (1 if lanes == 0 else 2), (lanes, before, after)
            assert after["a"] + after["b"] - before["a"] - before["b"] == 7
