"""The four-slot kernel's per-plan table of folded orders (switch `perm_table`).

The folded order of a period is numpy's stable argsort of fold_phase(t, period): a function of the time stamps and the period
alone.  The first four-slot launch of a plan stores every period's order, every later launch of the plan reads it and sorts
nothing.  The table holds the permutation the kernel would have computed, so nothing may move: every comparison here is
numpy.array_equal on (chi2, row, depth) -- and equal work counters where a launch counts -- against the same search with
`perm_table = 0`, which sorts in every launch."""
import contextlib

import numpy
import pytest

from test_gpu_parity import _inputs
from tls_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

ROW_ENTRIES = {"slim": 256 * 20, "slim512": 512 * 20}     # a table row: threads x samples a thread keeps, 2 bytes each


@contextlib.contextmanager
def fresh_context(**switches):
    ctx = _lib.Context(0)
    try:
        if switches:
            ctx.set_options(**switches)
        yield ctx
    finally:
        ctx.close()


def _args(inp, periods=None):
    return (inp["t"], inp["y"], inp["dy"], inp["periods"] if periods is None else periods, inp["table"], inp["params"])


def _same(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("chi2", "row", "depth")):
        assert numpy.array_equal(a, b), "%s: %s differs" % (what, name)


def _same_counters(got, want, what):
    for key in ("grid_cells", "evaluated_cells", "inner_steps"):
        assert got[3][key] == want[3][key], (what, key, got[3][key], want[3][key])


def _without_table(gpu, args):
    """(plain, counting) of the search that sorts in every launch; the plan holds no table."""
    gpu.set_options(perm_table=0)
    plain = gpu.search(*args)
    counting = gpu.search(*args, count_work=True)
    assert gpu.perm_table()["bytes"] == 0 and not gpu.perm_table()["filled"]
    gpu.set_options(perm_table=None)
    return plain, counting


def _fill_then_read(gpu, args, kernel, want_plain, want_counting, counting_first, launches=3):
    """A filling launch and `launches - 1` reading ones of a plan the context does not hold yet, plain and counting in turn."""
    gpu.prepare(*args)
    state = gpu.perm_table()
    assert state["bytes"] == 2 * ROW_ENTRIES[kernel] * len(args[3]) and not state["filled"], state
    for k in range(launches):
        counting = (k % 2 == 0) == counting_first
        got = gpu.search(*args, count_work=counting)
        assert gpu.last_kernel() == kernel
        assert gpu.perm_table()["filled"]
        what = "launch %d (%s, %s)" % (k, "counting" if counting else "plain", "filling" if k == 0 else "reading")
        _same(got, want_counting if counting else want_plain, what)
        if counting:
            _same_counters(got, want_counting, what)


@pytest.mark.parametrize("counting_first", [False, True], ids=["plain_first", "counting_first"])
@pytest.mark.parametrize("name,kernel,stride", [("k2_90d", "slim", 1), ("tutorial01", "slim", 3), ("lc_150d", "slim512", 5)])
def test_filling_launch_then_reading_launches(gpu, name, kernel, stride, counting_first):
    """n = 4320 (256 threads, four slots a CU), 4800 (three slots) and 7200 (the 512-thread shape): the launch that fills
    the table and two that read it, plain and counting in both orders."""
    inp = _inputs(name)
    assert len(inp["t"]) == {"k2_90d": 4320, "tutorial01": 4800, "lc_150d": 7200}[name]
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::stride]))
    want_plain, want_counting = _without_table(gpu, args)
    assert gpu.last_kernel() == kernel
    _same(want_counting, want_plain, "counting against plain without a table")
    _fill_then_read(gpu, args, kernel, want_plain, want_counting, counting_first)


@pytest.mark.parametrize("n,kernel", [(4320, "slim"), (7200, "slim512")])
def test_commensurate_periods_and_tied_flux(gpu, n, kernel):
    """The period list of the commensurate-period test: multiples of the cadence pile the phases up (piles of 144 points at
    4320, of 240 at 7200: the pile path fills those rows), on a flux quantised so that many values tie exactly."""
    commensurate = [30 / 48.0, 1.0, 2.5, 2.0, 10.0, 45.0]
    t = 3.0 + numpy.arange(n) / 48.0
    y = 1 + numpy.round(numpy.random.RandomState(5).normal(0, 5e-5, n) * 4e4) / 4e4
    assert len(numpy.unique(y)) < n // 50
    inp = synthetic.search_inputs(t, y)
    ordinary = inp["periods"][:: max(1, len(inp["periods"]) // 300)]
    periods = numpy.sort(numpy.concatenate([ordinary, commensurate]))
    args = _args(inp, periods)
    want_plain, want_counting = _without_table(gpu, args)
    _fill_then_read(gpu, args, kernel, want_plain, want_counting, counting_first=False)


@pytest.mark.parametrize("outlier", [3.0e4, 2.0e6])
def test_band_resolution_reads_the_order_from_the_table(gpu, outlier):
    """One wild flux value widens the undecided band until windows fall inside (the outlier flux of the band tests): a few
    dozen a period at 3e4 -- noted and decided on the exact prefix sum, flux gathered through the stashed order --, more than
    the list holds at 2e6 -- the period is searched again in exact mode.  On a READING launch the order comes from the table;
    stat_exact_retries > 0 says the path ran."""
    inp = _inputs("k2_90d")
    y = inp["y"].copy()
    y[137] = outlier
    kw = synthetic.config("k2_90d")[2]
    inp = synthetic.search_inputs(inp["t"], y, None, **kw)
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::7]))
    gpu.set_options(slim=1, prune=0, screen32=0)          # (the outlier is scatter to the host, which would take the classic kernel)
    want_plain, want_counting = _without_table(gpu, args)
    _fill_then_read(gpu, args, "slim", want_plain, want_counting, counting_first=True, launches=4)
    assert gpu.perm_table()["filled"]
    gpu.execute(phase_clock=True)                         # (a reading launch)
    stats = gpu.phase_cycles()
    assert stats["stat_exact_retries"] > 0, stats
    for slot in ("fold_count", "scan", "scatter", "rank", "e_convert"):      # slots 0-3 and 8: nothing was sorted
        assert stats[slot] == 0, (slot, stats[slot])
    _same(gpu.fetch(), want_plain, "the phase-clock launch")


def _two_launches_like_a_fresh_context(gpu, args, what):
    with fresh_context() as other:
        want = other.search(*args)
    gpu.prepare(*args)
    assert not gpu.perm_table()["filled"], what                # the plan was made from scratch: its table is empty
    for k in range(2):
        _same(gpu.search(*args), want, "%s, launch %d" % (what, k))
    assert gpu.last_kernel() != "slim" or gpu.perm_table()["filled"]


def test_invalidation_and_reuse(gpu):
    """The table lives as long as the plan key: other periods of the same count, other time stamps of the same length, a
    switch, and the change to per-point dy and back each plan from scratch -- two launches each, against a context that has
    never held another plan.  The same plan with a new flux keeps the table."""
    inp = _inputs("k2_90d")
    periods = numpy.ascontiguousarray(inp["periods"][::9])
    args = _args(inp, periods)
    gpu.search(*args)
    size = gpu.perm_table()["bytes"]
    assert gpu.last_kernel() == "slim" and gpu.perm_table()["filled"] and size == 2 * ROW_ENTRIES["slim"] * len(periods)
    # same n and n_periods, other periods
    other_periods = periods * (1.0 + 1.0 / 1024)
    _two_launches_like_a_fresh_context(gpu, _args(inp, other_periods), "other periods")
    assert gpu.perm_table()["bytes"] == size
    # same periods, other time stamps of equal length
    shifted_t = inp["t"] + 0.013 * numpy.sin(numpy.arange(len(inp["t"])))
    shifted_args = (shifted_t, inp["y"], inp["dy"], other_periods, inp["table"], inp["params"])
    _two_launches_like_a_fresh_context(gpu, shifted_args, "other time stamps")
    # a switch
    gpu.set_options(blocks=96)
    with fresh_context(blocks=96) as other:
        want = other.search(*args)
    gpu.prepare(*args)
    assert not gpu.perm_table()["filled"]
    for k in range(2):
        _same(gpu.search(*args), want, "switch blocks, launch %d" % k)
    gpu.set_options(blocks=None)
    # uniform dy -> per-point dy -> uniform dy
    dy = numpy.random.RandomState(5).uniform(0.7, 1.5, len(inp["y"])) * 50e-6
    weighted = (inp["t"], inp["y"], dy, periods, inp["table"], inp["params"])
    gpu.search(*args)
    assert gpu.perm_table()["filled"]
    _two_launches_like_a_fresh_context(gpu, weighted, "per-point dy")
    assert gpu.last_kernel() == "resident"
    _two_launches_like_a_fresh_context(gpu, args, "uniform dy again")
    assert gpu.last_kernel() == "slim"
    # the same plan, new flux: answered from the held plan, the table with it
    before = gpu.perm_table()
    assert before["filled"]
    inp2 = _inputs("k2_90d", seed=3)
    assert numpy.array_equal(inp2["t"], inp["t"]) and not numpy.array_equal(inp2["y"], inp["y"])
    args2 = _args(inp2, periods)
    with fresh_context(perm_table=0) as other:
        want2 = other.search(*args2)
    gpu.prepare(*args2)
    after = gpu.perm_table()
    assert after["plan_reuses"] == before["plan_reuses"] + 1 and after["filled"] and after["bytes"] == before["bytes"], (before, after)
    gpu.execute()
    _same(gpu.fetch(), want2, "new flux through the held plan")


@pytest.mark.parametrize("n_curves,stride", [(5, 1), (40, 4)])
@pytest.mark.parametrize("batch_first", [True, False], ids=["batch_fills", "single_fills"])
def test_survey_groups_share_the_table(n_curves, stride, batch_first):
    """search_batch of 5 curves (one group) and of 40 (two groups: the second reads what the first stored) equals the single
    searches, whichever fills the table."""
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    fluxes = numpy.stack([synthetic.config("k2_90d", seed=s)[1] for s in range(n_curves)])
    inputs = [synthetic.search_inputs(t, fluxes[k], **kw) for k in range(n_curves)]
    periods = numpy.ascontiguousarray(inputs[0]["periods"][::stride])
    ys = numpy.stack([inp["y"] for inp in inputs])
    dys = numpy.stack([inp["dy"] for inp in inputs])
    with fresh_context(perm_table=0) as plain_ctx:
        want = [plain_ctx.search(*_args(inp, periods)) for inp in inputs]
        assert plain_ctx.last_kernel() == "slim" and plain_ctx.perm_table()["bytes"] == 0
    with fresh_context() as ctx:
        if not batch_first:
            _same(ctx.search(*_args(inputs[0], periods)), want[0], "the single search that fills")
            assert ctx.perm_table()["filled"]
        chi2, row, depth = ctx.search_batch(inputs[0]["t"], ys, dys, periods, inputs[0]["table"], inputs[0]["params"])
        assert ctx.last_kernel() == "slim" and ctx.perm_table()["filled"]
        for k in range(n_curves):
            _same((chi2[k], row[k], depth[k]), want[k], "curve %d of the batch" % k)
        for k in (0, n_curves - 1):
            _same(ctx.search(*_args(inputs[k], periods)), want[k], "single search %d behind the batch" % k)


def test_power_batch_and_shards(gpu):
    """power_batch summaries with and without the table; a sharded plan (periods[r::8]) returns the full grid's bits on its
    share, on a filling and on a reading launch."""
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    fluxes = numpy.stack([synthetic.config("k2_90d", seed=s)[1] for s in range(5)])
    inputs = [synthetic.search_inputs(t, fluxes[k], **kw) for k in range(5)]
    inp = inputs[0]
    ys, dys = numpy.stack([i["y"] for i in inputs]), numpy.stack([i["dy"] for i in inputs])
    with fresh_context(perm_table=0) as plain_ctx:
        want = plain_ctx.power_batch(inp["t"], ys, dys, inp["periods"], inp["table"], inp["params"], 30)[0]
    for k in range(2):                                      # (the second call reads the table throughout)
        got = gpu.power_batch(inp["t"], ys, dys, inp["periods"], inp["table"], inp["params"], 30)[0]
        assert gpu.perm_table()["filled"]
        assert got.tobytes() == want.tobytes(), "power_batch summaries, call %d" % k
    full = gpu.search(*_args(inp))
    for r in range(8):
        share = numpy.ascontiguousarray(inp["periods"][r::8])
        for k in range(2):
            got = gpu.search(*_args(inp, share))
            _same(got, tuple(a[r::8] for a in full[:3]), "shard %d of 8, launch %d" % (r, k))
        assert gpu.perm_table()["filled"] and gpu.perm_table()["bytes"] == 2 * ROW_ENTRIES["slim"] * len(share)


def test_budget(gpu):
    """A cap below the table's size: no table, the same results.  perm_table = 0 allocates nothing.  With a table the
    context's device memory grows by exactly its size."""
    inp = _inputs("k2_90d")
    periods = numpy.ascontiguousarray(inp["periods"][::4])
    args = _args(inp, periods)
    need = 2 * ROW_ENTRIES["slim"] * len(periods)
    assert need > (1 << 20)
    with fresh_context(perm_table=0) as ctx:
        want = ctx.search(*args)
        assert ctx.perm_table()["bytes"] == 0 and not ctx.perm_table()["filled"]
        without = ctx.device_bytes()[0]
    with fresh_context(perm_table=1) as ctx:                # 1 MiB
        for k in range(2):
            _same(ctx.search(*args), want, "capped at 1 MiB, launch %d" % k)
        assert ctx.perm_table()["bytes"] == 0 and not ctx.perm_table()["filled"]
        assert ctx.device_bytes()[0] == without
    with fresh_context(perm_table=(need >> 20) + 1) as ctx:  # a cap that just holds it
        for k in range(2):
            _same(ctx.search(*args), want, "capped above the need, launch %d" % k)
        assert ctx.perm_table()["bytes"] == need and ctx.perm_table()["filled"]
        assert ctx.device_bytes()[0] == without + need
    with fresh_context() as ctx:
        _same(ctx.search(*args), want, "library's cap")
        assert ctx.perm_table()["bytes"] == need
        assert ctx.device_bytes()[0] == without + need


@pytest.mark.parametrize("n", [4320, 7200])
def test_pile_path_cost_where_a_launch_sorts(gpu, n):
    """The commensurate-period cost bound on launches that SORT: a plan without a table (`perm_table = 0`) and the filling
    launch of a plan with one.  (test_commensurate_periods_cost_no_more_than_their_neighbours times the launch behind a
    search of the same plan, which reads the table and ranks no pile.)  The four-slot kernel ranks a pile on 64-bit keys
    formed once per member: the costliest commensurate period within 4 x the median period of the same launch, as there."""
    commensurate = [30 / 48.0, 1.0, 2.5, 2.0, 10.0, 45.0]
    t = 3.0 + numpy.arange(n) / 48.0
    y = 1 + numpy.random.RandomState(5).normal(0, 5e-5, n)
    inp = synthetic.search_inputs(t, y)
    ordinary = inp["periods"][:: max(1, len(inp["periods"]) // 300)]
    periods = numpy.sort(numpy.concatenate([ordinary, commensurate]))
    special = numpy.isin(periods, commensurate)
    args = _args(inp, periods)

    def check(cycles, what):
        cycles = cycles.astype(float)
        median, worst = numpy.median(cycles[~special]), cycles[special].max()
        print("%s, n %d: worst pile period %.0f cycles = %.2f x the median %.0f" % (what, n, worst, worst / median, median))
        assert gpu.last_kernel().startswith("slim")
        assert worst <= 4.0 * median, (what, worst, median, periods[special][numpy.argmax(cycles[special])])
        return median

    gpu.set_options(perm_table=0)
    gpu.search(*args)
    assert gpu.perm_table()["bytes"] == 0
    sorting = check(gpu.period_cycles(), "no table")
    gpu.set_options(perm_table=None)
    gpu.prepare(*args)
    assert gpu.perm_table()["bytes"] > 0 and not gpu.perm_table()["filled"]
    check(gpu.period_cycles(), "filling launch")
    assert gpu.perm_table()["filled"]
    reading = numpy.median(gpu.period_cycles().astype(float)[~special])
    print("median period: %.0f cycles sorting, %.0f reading" % (sorting, reading))
    assert reading < sorting                                  # (a reading launch skips the sort: it cannot cost more)


@pytest.mark.parametrize("name,kernel,stride", [("k2_90d", "slim", 5), ("lc_150d", "slim512", 9)])
def test_reading_launch_after_poisoned_lds(gpu, name, kernel, stride):
    """A reading launch skips the phase that was the first writer of a period's LDS region and of the sort's counters: NaN
    words into every CU's LDS (and all-ones into the per-workgroup scratch) between the filling launch and the reading
    ones must not move a bit, plain or counting, single curve or group."""
    inp = _inputs(name)
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::stride]))
    want_plain, want_counting = _without_table(gpu, args)
    filling = gpu.search(*args)
    assert gpu.last_kernel() == kernel and gpu.perm_table()["filled"]
    _same(filling, want_plain, "filling launch")
    for k, counting in enumerate((False, True, False)):
        gpu.poison_lds(0x7ff80000)
        got = gpu.search(*args, count_work=counting)
        assert gpu.last_kernel() == kernel and gpu.perm_table()["filled"]
        _same(got, want_counting if counting else want_plain, "reading launch %d behind poisoned LDS" % k)
        if counting:
            _same_counters(got, want_counting, "reading launch %d behind poisoned LDS" % k)
    ys = numpy.stack([inp["y"], inp["y"][::-1].copy()])
    dys = numpy.stack([inp["dy"], inp["dy"]])
    gpu.poison_lds(0x7ff80000)
    chi2, row, depth = gpu.search_batch(inp["t"], ys, dys, args[3], inp["table"], inp["params"])
    _same((chi2[0], row[0], depth[0]), want_plain, "group of two behind poisoned LDS")
