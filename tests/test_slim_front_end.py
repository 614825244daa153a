"""The four-slot kernel's phase 2 from the table: gather, patch and scan in registers (switch `reg_scan`).

A plan whose fast-mode scan stretch per = ceil(M / threads), made odd, fits the 20 entries a thread keeps stores its folded
orders STRETCH-MAJOR: slot tid * 20 + j of a row holds the original index of patched position tid * per + j (position k >= n:
the index of position k - n).  A reading launch in fast mode then forms X in registers, with the operations of the in-place
scan in their order -- so nothing may move: every GPU comparison here is numpy.array_equal on (chi2, row, depth), and equal work
counters where a launch counts, between `reg_scan = 0` (thread-major rows, the in-place scan) and the default in one process.
Which path ran is asked of the device: `stat_register_scans` counts the prefix sums formed in registers.
"Off" is `reg_scan = 0`, "on" the value the session started with ("the library decides": on), so a run of the suite under
TLS_REG_SCAN=0 keeps its choice."""
import numpy
import pytest

import plan_edges as pe
from tls_amd import _lib, synthetic

PER_THREAD = pe.SLIM_PER_THREAD     # entries of a row a thread keeps
ROW_ENTRIES = {"slim": 256 * PER_THREAD, "slim512": 512 * PER_THREAD}
THREADS = {"slim": 256, "slim512": 512}
# the series of plan_edges' default set on either side of the `per` edge: M = 4864 | 4865 at 256 threads, 9728 | 9729 at 512
PER_EDGE = {4342: ("slim", 4864, 19), 4343: ("slim", 4865, 21), 8686: ("slim512", 9728, 19), 8687: ("slim512", 9729, 21)}


# ---- the layout, restated (CPU) ---------------------------------------------------------------------------------------

def scan_per(threads, M):
    """The fast-mode scan's stretch: ceil(M / threads), made odd."""
    per = -(-M // threads)
    return per if per % 2 else per + 1


def stretch_major_row(order, n, M, threads, per):
    """A row of the table: the thread's patched positions side by side, unused slots zero."""
    row = numpy.zeros(threads * PER_THREAD, dtype=numpy.int64)
    used = numpy.zeros(threads * PER_THREAD, dtype=bool)
    for k in range(M):
        slot = (k // per) * PER_THREAD + k % per
        assert k % per < PER_THREAD and slot < len(row) and not used[slot], (k, slot)
        used[slot] = True
        row[slot] = order[k if k < n else k - n]
    return row, used


def perm_slot(threads, per, k):
    """slim_perm_slot: where folded position k < n is kept (per == 0: thread-major)."""
    return (k // per) * PER_THREAD + k % per if per > 0 else (k % threads) * PER_THREAD + k // threads


def _edge_shapes():
    """(n, W, threads) of every four-slot plan the edges of tests/plan_edges.py visit, and of the `per` edge's series."""
    shapes = set()
    lengths = set(PER_EDGE)
    for edge in pe.PLAN_EDGES:
        if not any(k.startswith("slim") for k in edge.kernels):
            continue
        at = edge.model_edge()
        lengths.update((edge.set_name, n) for n in (at, at + 1))
    for item in sorted(lengths, key=str):
        set_name, n = item if isinstance(item, tuple) else ("default", item)
        nn, M, n_widths, pad = pe.shape(pe.inputs(set_name, n))
        kernel = pe.expected_plan(nn, M, n_widths, pad)[0]
        if kernel in THREADS:
            shapes.add((nn, M - nn, THREADS[kernel]))
    return sorted(shapes)


def test_stretch_major_slot_map_and_its_inverse():
    shapes = _edge_shapes()
    assert len(shapes) >= 8 and {s[2] for s in shapes} == {256, 512}
    seen_fit, seen_unfit = False, False
    for n, W, threads in shapes:
        M = n + W
        per = scan_per(threads, M)
        assert per % 2 == 1 and threads * per >= M and W <= n
        if per > PER_THREAD:                       # the plan keeps thread-major rows
            seen_unfit = True
            assert M > threads * (PER_THREAD - 1)
            slots = [perm_slot(threads, 0, k) for k in range(n)]
            assert len(set(slots)) == n and max(slots) < threads * PER_THREAD
            continue
        seen_fit = True
        order = numpy.random.RandomState(n).permutation(n)
        row, used = stretch_major_row(order, n, M, threads, per)
        assert int(used.sum()) == M and len(row) == threads * PER_THREAD          # every patched position has one slot
        for k in range(n):                                                         # slim_perm_slot inverts it
            assert row[perm_slot(threads, per, k)] == order[k]
        # a thread's entries are its scan stretch of the patched series
        patched = numpy.concatenate([order, order[:W]])
        for tid in (0, 1, threads // 2, (M - 1) // per, threads - 1):
            lo, hi = min(tid * per, M), min(tid * per + per, M)
            assert numpy.array_equal(row[tid * PER_THREAD: tid * PER_THREAD + hi - lo], patched[lo:hi])
            assert not used[tid * PER_THREAD + hi - lo: (tid + 1) * PER_THREAD].any()
    assert seen_fit and seen_unfit


def test_the_per_edge_is_where_the_issue_puts_it():
    for n, (kernel, M, per) in PER_EDGE.items():
        nn, MM, n_widths, pad = pe.shape(pe.inputs("default", n))
        assert (nn, MM) == (n, M) and pe.expected_plan(nn, MM, n_widths, pad)[0] == kernel
        assert scan_per(THREADS[kernel], M) == per
    assert scan_per(256, 4838) == 19               # config 2


# ---- the device ------------------------------------------------------------------------------------------------------

SWITCHES = ("reg_scan",)
FORCE_SLIM = dict(slim=1, prune=0, screen32=0)   # the four-slot kernel where the host would take a classic variant


def _args(inp, periods=None):
    return (inp["t"], inp["y"], inp["dy"], inp["periods"] if periods is None else periods, inp["table"], inp["params"])


def _config_inputs(name, **over):
    t, f, kw = synthetic.config(name, **over)
    return synthetic.search_inputs(t, f, **kw)


def _same(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("chi2", "row", "depth")):
        assert a.tobytes() == b.tobytes(), "%s: %s differs" % (what, name)


def _same_counters(got, want, what):
    for key in ("evaluated_cells", "inner_steps"):
        assert got[3][key] == want[3][key], (what, key, got[3][key], want[3][key])


def _session_value(ctx, switch):
    """(the value the context started with, whether that means on): a run of the suite under TLS_<SWITCH>=0 keeps its choice."""
    value = ctx.get_options()[switch] if not hasattr(ctx, "initial_options") else ctx.initial_options[switch]
    return value, value != 0


def _fits(args, kernel):
    """The layout rule: the scan stretch of the plan (M from the template table) is at most the entries a thread keeps."""
    M = pe.shape({"t": args[0], "table": args[4], "params": args[5]})[1]
    return scan_per(THREADS[kernel], M) <= PER_THREAD


def _launches(gpu, args, kernel, poison=False):
    """A filling launch and three reading ones (plain, counting, plain, counting) of a plan made from scratch, then a
    reading launch that keeps the statistics."""
    gpu.prepare(*args)
    assert not gpu.perm_table()["filled"]
    out = []
    for k in range(4):
        if poison and k > 0:
            gpu.poison_lds(0x7ff80000)
        out.append(gpu.search(*args, count_work=bool(k % 2)))
        assert gpu.last_kernel() == kernel and gpu.perm_table()["filled"]
    assert gpu.perm_table()["bytes"] == 2 * ROW_ENTRIES[kernel] * len(args[3])      # a row keeps its size
    gpu.execute(phase_clock=True)
    stats = gpu.phase_cycles()
    for slot in ("fold_count", "scan", "scatter", "rank", "e_convert"):              # a reading launch sorts nothing
        assert stats[slot] == 0, (slot, stats[slot])
    out.append(gpu.fetch())
    return out, stats


def _off_against_on(gpu, switch, args, kernel, poison=False, options=None):
    """`switch = 0` against the session's value: five launches each, every result and the counters 0 and 1 equal; which
    path ran is asked of the device.  Returns the statistics of the two reading launches (off, on)."""
    session, is_on = _session_value(gpu, switch)
    reg_scan_on = _session_value(gpu, "reg_scan")[1]
    gpu.set_options(**dict(options or {}, **{switch: 0}))
    off, stats_off = _launches(gpu, args, kernel, poison)
    gpu.set_options(**{switch: session})
    on, stats_on = _launches(gpu, args, kernel, poison)
    for k, (a, b) in enumerate(zip(on, off)):
        what = "%s, launch %d (%s, %s)" % (switch, k, "counting" if k % 2 else "plain", "reading" if k else "filling")
        _same(a, b, what)
        if k % 2:
            _same_counters(a, b, what)
    _same(on[1], on[0], "counting against plain")
    _same(on[4], on[0], "the statistics launch against the filling launch")
    # phase 2: fast mode forms one prefix sum a period; what goes through exact mode afterwards takes the in-place path
    fits = _fits(args, kernel)
    scans = {False: 0, True: len(args[3]) if fits else 0}
    assert stats_off["stat_register_scans"] == scans[reg_scan_on and switch != "reg_scan"], stats_off
    assert stats_on["stat_register_scans"] == scans[reg_scan_on], stats_on
    return stats_off, stats_on


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("n", sorted(PER_EDGE))
def test_either_side_of_the_per_edge(gpu, n, switch):
    """M = 4864 | 4865 at 256 threads and 9728 | 9729 at 512: the last plan whose stretch fits a thread's entries and the
    first that keeps thread-major rows and the in-place scan."""
    kernel, M, per = PER_EDGE[n]
    inp = pe.inputs("default", n)
    args = _args(inp, inp["selected"])
    assert pe.shape(inp)[1] == M and _fits(args, kernel) == (per <= PER_THREAD)
    _off_against_on(gpu, switch, args, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name,kernel,stride", [("k2_90d", "slim", 3), ("tutorial01", "slim", 5), ("lc_150d", "slim512", 7)])
def test_filling_then_reading_launches_behind_poisoned_lds(gpu, name, kernel, stride, switch):
    """Both shapes, plain and counting, four and three slots a CU, low noise (most rows of a period are sparse or hold no
    live unit); NaN words into every CU's LDS between the launches: the register path has no barrier in front of its first
    LDS store and reads nothing it has not written."""
    inp = _config_inputs(name)
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::stride]))
    assert _fits(args, kernel) == (name != "tutorial01")      # 4800 points: M = 5376, a stretch of 21 at 256 threads
    _off_against_on(gpu, switch, args, kernel, poison=True)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
def test_plan_without_a_table(gpu, switch):
    """`perm_table = 0`: every launch sorts, single searches take the in-place phase 2 under either layout."""
    inp = _config_inputs("k2_90d")
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::6]))
    want = gpu.search(*args, count_work=True)
    for value in (0, _session_value(gpu, switch)[0]):
        gpu.set_options(**{"perm_table": 0, switch: value})
        for counting in (False, True):
            got = gpu.search(*args, count_work=counting)
            assert gpu.last_kernel() == "slim" and gpu.perm_table()["bytes"] == 0
            _same(got, want, "no table, %s %r" % (switch, value))
            if counting:
                _same_counters(got, want, "no table, %s %r" % (switch, value))
        gpu.execute(phase_clock=True)
        assert gpu.phase_cycles()["stat_register_scans"] == 0
        _same(gpu.fetch(), want, "no table, %s %r, the statistics launch" % (switch, value))


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("outlier", [3.0e4, 2.0e6])
def test_band_windows(gpu, outlier, switch):
    """One wild flux value puts windows inside the undecided band: a few dozen a period are noted and decided on the exact
    prefix sum -- the resolution reads the flux through
    slim_perm_slot, the exact-mode gather reads the row entry by entry --, more than the list holds and the period is
    searched again in exact mode.  On reading launches."""
    t, y, kw = synthetic.config("k2_90d")
    y = y.copy()
    y[137] = outlier
    inp = synthetic.search_inputs(t, y, None, **kw)
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::7]))
    off, on = _off_against_on(gpu, switch, args, "slim", options=FORCE_SLIM)
    assert on["stat_exact_retries"] > 0 and on["stat_exact_retries"] == off["stat_exact_retries"], (on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("n,kernel", [(4320, "slim"), (7200, "slim512")])
def test_commensurate_periods(gpu, n, kernel, switch):
    """Multiples of the cadence pile the phases up (the pile path fills those rows) on a flux whose values tie."""
    commensurate = [30 / 48.0, 1.0, 2.5, 2.0, 10.0, 45.0]
    t = 3.0 + numpy.arange(n) / 48.0
    y = 1 + numpy.round(numpy.random.RandomState(5).normal(0, 5e-5, n) * 4e4) / 4e4
    inp = synthetic.search_inputs(t, y)
    ordinary = inp["periods"][:: max(1, len(inp["periods"]) // 300)]
    periods = numpy.sort(numpy.concatenate([ordinary, commensurate]))
    _off_against_on(gpu, switch, _args(inp, periods), kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("batch_first", [True, False], ids=["batch_fills", "single_fills"])
def test_survey_group_of_32_against_single_searches(batch_first, switch):
    """search_batch of 32 curves equals the single searches with the switch off and on, whichever fills the table (a group
    that fills reads its own stash, which has the plan's layout)."""
    n_curves = 32
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    inputs = [synthetic.search_inputs(t, synthetic.config("k2_90d", seed=s)[1], **kw) for s in range(n_curves)]
    periods = numpy.ascontiguousarray(inputs[0]["periods"][::16])
    ys = numpy.stack([inp["y"] for inp in inputs])
    dys = numpy.stack([inp["dy"] for inp in inputs])
    results = []
    for leg in ("off", "session"):
        ctx = _lib.Context(0)
        try:
            if leg == "off":
                ctx.set_options(**{switch: 0})
            singles = []
            if not batch_first:
                singles.append(ctx.search(*_args(inputs[0], periods)))
            batch = ctx.search_batch(inputs[0]["t"], ys, dys, periods, inputs[0]["table"], inputs[0]["params"])
            assert ctx.last_kernel() == "slim" and ctx.perm_table()["filled"]
            again = ctx.search_batch(inputs[0]["t"], ys, dys, periods, inputs[0]["table"], inputs[0]["params"])
            for a, b in zip(batch, again):
                assert a.tobytes() == b.tobytes()
            singles += [ctx.search(*_args(inputs[k], periods)) for k in range(n_curves)]
            results.append((batch, singles))
        finally:
            ctx.close()
    for leg, (batch, singles) in zip(("off", "session"), results):
        for k in range(n_curves):
            _same((batch[0][k], batch[1][k], batch[2][k]), singles[k + (0 if batch_first else 1)], "curve %d, %s %s" % (k, switch, leg))
    for a, b in zip(results[0][0], results[1][0]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("sigma", [150e-6, 600e-6])
def test_noisy_series(gpu, sigma, switch):
    """Noise well above transit_depth_min: full rows, sparse rows and re-listed tails behind a prefix sum formed in registers."""
    inp = _config_inputs("k2_90d", sigma=sigma)
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::20]))
    _off_against_on(gpu, switch, args, "slim", options=FORCE_SLIM)
