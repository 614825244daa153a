"""The four-slot kernel's dense depth predicate in fast mode (phase 3a; switch `dense_hoist`,
tls_slim_kernel.hip.h: slim_dense_tile).

The switch changes how the rows of a tile are walked -- one loop per case, the band test per step, no mask for lanes without
a unit, a repeated last row instead of a branch per row -- and not one operation of a cell's decision.  So nothing may move:
every GPU comparison here is tobytes() equality on (chi2, row, depth) and equal `evaluated_cells` and `inner_steps` of a
counting launch, between the switch at 0 (the kernel instantiations with the former loop) and the value the session started
with ("the library decides": on), on one plan launched three times each way: a filling launch and two reading ones.  (The
cases ran in the same form over the other half of the proposal, `dense_rows4`, before it was dropped: PERF_LOG.md.)

The shapes are the smallest at which the loop can go wrong: the plan's edges, a last tile that is full, nearly empty and
nearly full, dense row counts on both sides of the two-row step (and of a four-row one), more rows than the 64 lanes that
take their masks, windows inside the undecided band (noted, and so many that the period goes through exact mode, which keeps
the former loop), a survey group, and poisoned LDS between the launches.

Dense row counts: config 2's default grid (256 threads) holds periods of 4 to 32 dense rows; the 150-day series (512
threads) those of 0 to 32 -- its shortest periods start at rows that are strided already --, so the counts below four,
and the period without a dense row, are searched there (test_row_counts_either_side_of_the_steps).

The duration grid of step 1.02 holds 110 distinct widths at 1458 points and more from 1459 on (plan_edges.width_table_edge):
1458 is the last length the four-slot kernel takes with it, and the one searched here."""
import numpy
import pytest

import plan_edges as pe
from tls_amd import _lib, grid, synthetic

K_R = 5          # windows of a unit (kR)
WAVE = 64
BAND_CAP = 256   # noted windows a period (kBandCap)
PARTS = (("dense_hoist",),)
PART_IDS = ["hoist"]
FORCE_SLIM = dict(slim=1, prune=0, screen32=0)   # the four-slot kernel where the host would take a classic variant


# ---- the plan's rows, restated (CPU) ------------------------------------------------------------------------------------

def width_rows(inp):
    """(distinct widths ascending, their T0 strides, M): core.py:50-55 and 113-116 as the plan has them."""
    width = numpy.unique(numpy.asarray(inp["table"].width)).astype(numpy.int64)
    margin = inp["params"]["T0_fit_margin"]
    xth = numpy.ones(len(width), dtype=numpy.int64)
    if margin > 0:
        inv = 1 / margin
        for k, w in enumerate(width):
            if w > margin:
                xth[k] = max(1, int(float(w) / inv))
    M = len(inp["t"]) + int(width[-1]) + int(width[-1]) % 2
    return width, xth, M


def period_rows(inp, periods):
    """(k_lo, k_hi, k_x) of every period: the in-range rows of the ascending width table (core.py:143-156) and the end of
    the dense ones (stride 1), as plan_periods forms them."""
    width, xth, _ = width_rows(inp)
    p = inp["params"]
    n = len(inp["t"])
    length = float(numpy.max(inp["t"]) - numpy.min(inp["t"]))
    strided = numpy.nonzero(xth != 1)[0]
    first_strided = int(strided[0]) if len(strided) else len(width)
    assert (xth[first_strided:] != 1).all()
    out = []
    for P in periods:
        duration_max = grid.T14(p["R_star_max"], p["M_star_max"], float(P), small=False)
        duration_min = grid.T14(p["R_star_min"], p["M_star_min"], float(P), small=True)
        naive = length / float(P)
        correction = (naive + 1) / naive
        lo, hi = int(numpy.floor(duration_min * n)), int(numpy.ceil(duration_max * n * correction))
        k_lo = int(numpy.searchsorted(width, lo, side="left"))
        k_hi = max(k_lo, int(numpy.searchsorted(width, hi, side="right")))
        out.append((k_lo, k_hi, min(k_hi, max(k_lo, first_strided))))
    return out


def units_of_row(inp, k):
    """Units of a dense row: n_pos = M - width + 1 trial positions, kR to a unit."""
    width, xth, M = width_rows(inp)
    assert xth[k] == 1
    n_pos = M - int(width[k]) + 1
    return -(-n_pos // K_R)


def dense_counts(inp, periods):
    return numpy.array([k_x - k_lo for k_lo, _, k_x in period_rows(inp, periods)])


# lengths of the default set (plan_edges.light_curve) whose first dense row has 0, 1 and 63 units in its last tile, for
# every period searched here; found by a scan of the restatement above, re-derived and asserted by the test
LAST_TILE = {0: 2289, 1: 2292, 63: 2284}


def _with_residue(inp, residue):
    rows = period_rows(inp, inp["selected"])
    keep = [i for i, (k_lo, _, k_x) in enumerate(rows) if k_x > k_lo and units_of_row(inp, k_lo) % WAVE == residue]
    return numpy.ascontiguousarray(inp["selected"][keep])


def test_last_tile_lengths_have_their_residues():
    for residue, n in LAST_TILE.items():
        inp = pe.inputs("default", n)
        periods = _with_residue(inp, residue)
        assert len(periods) >= 6, (residue, n, len(periods))
        nn, M, n_widths, pad = pe.shape(inp)
        assert pe.expected_plan(nn, M, n_widths, pad)[0] == "slim"


ROW_COUNTS = {"k2_90d": ("slim", (4, 5, 8)), "lc_150d": ("slim512", (0, 1, 2, 3, 4, 5, 8))}


def test_row_counts_either_side_of_the_steps():
    for name, (_, wanted) in ROW_COUNTS.items():
        inp, periods, counts = _row_count_periods(name)
        assert tuple(sorted(set(counts))) == wanted and len(periods) == len(counts) == 3 * len(wanted)
    assert dense_counts(_config_inputs("k2_90d"), _config_inputs("k2_90d")["periods"]).min() == 4


# ---- the device ---------------------------------------------------------------------------------------------------------

def _args(inp, periods=None):
    return (inp["t"], inp["y"], inp["dy"], inp["periods"] if periods is None else periods, inp["table"], inp["params"])


def _config_inputs(name, **over):
    t, f, kw = synthetic.config(name, **over)
    return synthetic.search_inputs(t, f, **kw)


def _row_count_periods(name):
    """Periods of a configuration's default grid with the dense row counts wanted of it (ROW_COUNTS), three of each."""
    inp = _config_inputs(name)
    counts = dense_counts(inp, inp["periods"])
    keep = []
    for want in ROW_COUNTS[name][1]:
        at = numpy.nonzero(counts == want)[0]
        assert len(at) >= 3, (name, want, len(at))
        keep.extend(at[numpy.linspace(0, len(at) - 1, 3).astype(int)])
    keep = numpy.array(sorted(keep), dtype=int)
    return inp, numpy.ascontiguousarray(inp["periods"][keep]), [int(c) for c in counts[keep]]


def _same(got, want, what):
    for a, b, name in zip(got[:3], want[:3], ("chi2", "row", "depth")):
        assert a.tobytes() == b.tobytes(), "%s: %s differs" % (what, name)


def _same_counters(got, want, what):
    for key in ("evaluated_cells", "inner_steps"):
        assert got[3][key] == want[3][key], (what, key, got[3][key], want[3][key])


def _session(ctx, part):
    """The values the context started with: a run of the suite under TLS_DENSE_HOIST=0 keeps its choice."""
    initial = ctx.initial_options if hasattr(ctx, "initial_options") else ctx.get_options()
    return {name: initial[name] for name in part}


def _launches(ctx, args, kernel, poison=False):
    """A filling launch and two reading ones (plain, counting) of a plan made from scratch, then a reading launch that keeps
    the statistics."""
    ctx.prepare(*args)
    out = []
    for k in range(3):
        if poison and k > 0:
            ctx.poison_lds(0x7ff80000)
        out.append(ctx.search(*args, count_work=(k == 2)))
        assert ctx.last_kernel() == kernel and ctx.perm_table()["filled"]
    ctx.execute(phase_clock=True)
    stats = ctx.phase_cycles()
    out.append(ctx.fetch())
    return out, stats


def _off_against_on(ctx, part, args, kernel, poison=False, options=None):
    """The part's switches at 0 against the session's values: four launches each, every result and the work counters equal.
    Returns the statistics of the two statistics launches (off, on)."""
    ctx.set_options(**dict(options or {}, **{name: 0 for name in part}))
    off, stats_off = _launches(ctx, args, kernel, poison)
    ctx.set_options(**_session(ctx, part))
    on, stats_on = _launches(ctx, args, kernel, poison)
    for k, (a, b) in enumerate(zip(on, off)):
        what = "%s, launch %d (%s)" % ("+".join(part), k, ("filling", "reading", "reading, counting", "statistics")[k])
        _same(a, b, what)
        if k == 2:
            _same_counters(a, b, what)
            assert a[3]["evaluated_cells"] > 0
    for k in (1, 2, 3):
        _same(on[k], on[0], "launch %d against the filling launch" % k)
    assert stats_on["stat_exact_retries"] == stats_off["stat_exact_retries"], (stats_on, stats_off)
    return stats_off, stats_on


def _bucket_room_edge():
    edge = [e for e in pe.PLAN_EDGES if e.name == "bucket-room"][0]
    return edge, edge.model_edge() + 1


def test_the_shortest_four_slot_series_is_where_the_issue_puts_it():
    edge, n = _bucket_room_edge()
    assert n == 675 and edge.plan(n)[0] == "slim" and edge.plan(n - 1)[0] == "resident"


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
@pytest.mark.parametrize("n,kernel", [(675, "slim"), (5120, "slim"), (5121, "slim512")])
def test_plan_edges(gpu, n, kernel, part):
    """The shortest series the four-slot kernel takes (the bucket-room edge, 10 ppm), the last 256-thread length and the first
    512-thread one."""
    inp = _bucket_room_edge()[0].inputs(n) if n == 675 else pe.inputs("default", n)
    _off_against_on(gpu, part, _args(inp, inp["selected"]), kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
@pytest.mark.parametrize("residue", sorted(LAST_TILE))
def test_last_tile_full_nearly_empty_nearly_full(gpu, residue, part):
    """Row k_lo's unit count is 0, 1 and 63 mod 64 for every period searched: the lanes of the last tile without a unit."""
    inp = pe.inputs("default", LAST_TILE[residue])
    periods = _with_residue(inp, residue)
    for k_lo, _, k_x in period_rows(inp, periods):
        assert k_x > k_lo and units_of_row(inp, k_lo) % WAVE == residue
    _off_against_on(gpu, part, _args(inp, periods), "slim", options=FORCE_SLIM)   # (50 ppm at this length: the host would screen)


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
@pytest.mark.parametrize("name", sorted(ROW_COUNTS))
def test_dense_row_counts_around_the_step(gpu, name, part):
    """0, 1, 2, 3, 4, 5 and 8 dense rows: no dense pass at all, and both sides of the four-row and of the two-row step."""
    inp, periods, counts = _row_count_periods(name)
    assert tuple(sorted(set(counts))) == ROW_COUNTS[name][1]
    _off_against_on(gpu, part, _args(inp, periods), ROW_COUNTS[name][0])


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
def test_more_dense_rows_than_lanes(gpu, part):
    """The duration grid of step 1.02 at 1458 points, its 110 widths: periods with more than 64 dense rows take push_live row
    by row."""
    n = pe.width_table_edge()[0]
    assert n == 1458
    inp = pe.inputs("fine", n, 10e-6)
    assert pe.shape(inp)[2] == 110
    counts = dense_counts(inp, inp["selected"])
    assert counts.min() > WAVE and counts.max() > WAVE + 32, (int(counts.min()), int(counts.max()))
    _off_against_on(gpu, part, _args(inp, inp["selected"]), "slim")


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
@pytest.mark.parametrize("outlier", [3.0e4, 2.0e6])
def test_band_windows_noted(gpu, outlier, part):
    """One wild flux value puts windows inside the undecided band: a few dozen a period are noted, k, window and dX, and
    decided on the exact prefix sum."""
    t, y, kw = synthetic.config("k2_90d")
    y = y.copy()
    y[137] = outlier
    inp = synthetic.search_inputs(t, y, None, **kw)
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::7]))
    off, on = _off_against_on(gpu, part, args, "slim", options=FORCE_SLIM)
    assert on["stat_exact_retries"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
def test_band_list_overflows_into_exact_mode(gpu, part):
    """Long stretches of flux exactly 1 - transit_depth_min: every window inside one has the threshold's depth, more than
    the list's 256 land in the band and the period is searched again in exact mode, by the loop without the switches."""
    t, y, kw = synthetic.config("k2_90d")
    inp = synthetic.search_inputs(t, y, None, **kw)
    y = inp["y"].copy()
    level = 1.0 - inp["params"]["transit_depth_min"]
    y[:2000] = level                       # (two stretches with 20 noisy points between them: whatever the period interleaves,
    y[2020:] = level                       # most windows of the folded series hold nothing else)
    inp = synthetic.search_inputs(t, y, None, **kw)
    assert int((inp["y"] == level).sum()) == len(y) - 20 > BAND_CAP
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::400]))
    off, on = _off_against_on(gpu, part, args, "slim", options=FORCE_SLIM)
    assert on["stat_exact_retries"] >= len(args[3]) // 2, on["stat_exact_retries"]


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
def test_poisoned_lds_between_launches(gpu, part):
    """NaN words into every CU's LDS between the launches: the loops read nothing of a previous launch."""
    inp = _config_inputs("k2_90d")
    args = _args(inp, numpy.ascontiguousarray(inp["periods"][::9]))
    _off_against_on(gpu, part, args, "slim", poison=True)


@pytest.mark.gpu
@pytest.mark.parametrize("part", PARTS, ids=PART_IDS)
def test_survey_group_of_three_against_single_searches(part):
    """n_curves = 3: the curve loop enters the pass again on the same order; against the three single searches, switches
    off and on."""
    n_curves = 3
    t, _, kw = synthetic.config("k2_90d", seed=0)
    inputs = [synthetic.search_inputs(t, synthetic.config("k2_90d", seed=s)[1], **kw) for s in range(n_curves)]
    periods = numpy.ascontiguousarray(inputs[0]["periods"][::16])
    ys = numpy.stack([inp["y"] for inp in inputs])
    dys = numpy.stack([inp["dy"] for inp in inputs])
    results = []
    for leg in ("off", "session"):
        ctx = _lib.Context(0)
        try:
            if leg == "off":
                ctx.set_options(**{name: 0 for name in part})
            batch = ctx.search_batch(inputs[0]["t"], ys, dys, periods, inputs[0]["table"], inputs[0]["params"])
            assert ctx.last_kernel() == "slim"
            singles = [ctx.search(*_args(inputs[k], periods)) for k in range(n_curves)]
            results.append((batch, singles))
        finally:
            ctx.close()
    for leg, (batch, singles) in zip(("off", "session"), results):
        for k in range(n_curves):
            _same((batch[0][k], batch[1][k], batch[2][k]), singles[k], "curve %d, %s %s" % (k, "+".join(part), leg))
    for a, b in zip(results[0][0], results[1][0]):
        assert a.tobytes() == b.tobytes()
