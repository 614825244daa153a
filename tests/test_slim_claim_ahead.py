"""The four-slot kernel's period queue on the device ("The period queue's tickets"; switch `claim_ahead`).

Bit 0: a workgroup's first ticket is its own index and the queue word hands out the later ones.  Which workgroup searches
which period may change -- nothing a period computes does: every comparison is numpy.array_equal on (chi2, row, depth),
and equal counters where a launch counts, between `claim_ahead = 0` (every ticket from the queue word) and the bit, in
one process.  (The second part that was built, the next period's ticket drawn during the dot products, was measured and
removed with its code: PERF_LOG.md; the cases it asked for stay, a retried period keeps its ticket either way.)

The series is 720 points at 30-minute cadence, just above the four-slot kernel's bucket-room edge (PERF_LOG.md, "Open
items"); the 512-thread shape runs at its smallest series, 5121 points.  Every GPU step runs under a time limit of its own:
a launch that does not end (a ticket lost, a workgroup that never leaves) ends the process instead of waiting."""
import contextlib
import faulthandler

import numpy
import pytest

from tls_amd import _lib, synthetic

FORCE_SLIM = dict(slim=1, prune=0, screen32=0)   # the four-slot kernel where the host would take a classic variant
BITS = (1,)                                       # against 0
STEP_SECONDS = 60


@contextlib.contextmanager
def _limit(seconds=STEP_SECONDS):
    """The step's own time limit: the process exits (with every thread's traceback) when it runs out."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _series(n=720, sigma=60e-6, seed=0):
    t, flux = synthetic.light_curve((n + 0.5) / 48.0, 48, sigma, seed=seed, per=2.345, rp=0.03, a=9)
    assert len(t) == n
    return t, flux


_CACHE = {}


def _inputs(n=720):
    if n not in _CACHE:
        t, flux = _series(n)
        _CACHE[n] = synthetic.search_inputs(t, flux)
    return _CACHE[n]


def _periods(inp, count):
    """`count` periods from the default grid's range."""
    grid = inp["periods"]
    if count == 1:
        return numpy.asarray([grid[len(grid) // 2]])
    return numpy.ascontiguousarray(numpy.linspace(grid[0], grid[-1], count))


def _args(inp, periods, y=None):
    return (inp["t"], inp["y"] if y is None else y, inp["dy"], periods, inp["table"], inp["params"])


def _same(got, want, what, counters=False):
    for a, b, name in zip(got[:3], want[:3], ("chi2", "row", "depth")):
        assert numpy.array_equal(a, b), "%s: %s differs in %d of %d periods" % (what, name, int((a != b).sum()), a.size)
    if counters:
        for key in ("evaluated_cells", "inner_steps"):
            assert got[3][key] == want[3][key], (what, key, got[3][key], want[3][key])


def _set(gpu, bits, **more):
    gpu.set_options(**dict(FORCE_SLIM, claim_ahead=bits, **more))


def _three_launches(gpu, args, kernel="slim"):
    """A filling launch, a reading one and a counting one on a plan made from scratch."""
    out = []
    with _limit():
        gpu.prepare(*args)
        assert not gpu.perm_table()["filled"]
        for counting in (False, False, True):
            out.append(gpu.search(*args, count_work=counting))
            assert gpu.last_kernel() == kernel
        assert gpu.perm_table()["filled"]
    _same(out[1], out[0], "reading against filling")
    _same(out[2], out[0], "counting against plain")
    return out


def _blocks(gpu, inp):
    """Workgroups of a launch that has more periods than the device has slots."""
    with _limit():
        _set(gpu, 0)
        gpu.prepare(*_args(inp, _periods(inp, 4099)))
        blocks = gpu.plan_info()["n_blocks"]
    assert 1 <= blocks <= 2048
    return blocks


COUNTS = {"1": lambda b: 1, "3": lambda b: 3, "blocks-1": lambda b: max(b - 1, 1), "blocks": lambda b: b,
          "blocks+1": lambda b: b + 1, "2*blocks+3": lambda b: 2 * b + 3}


@pytest.mark.gpu
@pytest.mark.parametrize("count", list(COUNTS))
def test_period_counts_around_the_workgroups(gpu, count):
    """Launches of 1, 3, blocks - 1, blocks, blocks + 1 and 2 * blocks + 3 periods: with at most `blocks` periods every
    ticket drawn from the queue word is one a workgroup leaves on; one period more and exactly one workgroup searches twice."""
    inp = _inputs()
    n_periods = COUNTS[count](_blocks(gpu, inp))
    args = _args(inp, _periods(inp, n_periods))
    _set(gpu, 0)
    want = _three_launches(gpu, args)
    assert len(want[0][0]) == n_periods and numpy.isfinite(want[0][0]).all()
    for bits in BITS:
        _set(gpu, bits)
        got = _three_launches(gpu, args)
        for k, (a, b) in enumerate(zip(got, want)):
            _same(a, b, "claim_ahead %d, %d periods, launch %d" % (bits, n_periods, k), counters=k == 2)


@pytest.mark.gpu
def test_five_launches_in_a_row_behind_poisoned_lds_and_stale_results(gpu):
    """The context has searched another flux on as many periods: a period nobody searches shows as that search's value.
    NaN words into every CU's LDS between the launches: the ticket is written before it is read."""
    inp = _inputs()
    blocks = _blocks(gpu, inp)
    periods = _periods(inp, 2 * blocks + 3)
    other_y = numpy.ascontiguousarray(inp["y"][::-1])
    results = {}
    for bits in (0,) + BITS:
        _set(gpu, bits)
        with _limit():
            stale = gpu.search(*_args(inp, periods * (1.0 + 1e-9), y=other_y))
            gpu.prepare(*_args(inp, periods))
            assert not gpu.perm_table()["filled"]        # another plan: the first of the five fills its table
        out = []
        for k in range(5):
            with _limit():
                gpu.poison_lds(0x7ff80000)
                out.append(gpu.search(*_args(inp, periods), count_work=k == 3))
                assert gpu.last_kernel() == "slim" and gpu.perm_table()["filled"]
        assert not numpy.array_equal(stale[0], out[0][0])
        for k in range(1, 5):
            _same(out[k], out[0], "claim_ahead %d, launch %d against the filling launch" % (bits, k))
        results[bits] = out
    for bits in BITS:
        for k in range(5):
            _same(results[bits][k], results[0][k], "claim_ahead %d, launch %d" % (bits, k), counters=k == 3)


def _band_fluxes(inp):
    """Fluxes whose window means meet the undecided band around transit_depth_min: every window of a constant flux at
    1 - transit_depth_min sits on it (more windows than the list holds: the period's exact retry); one wild value widens
    the band of a quiet flux until a few windows a period are noted (band resolution)."""
    flat = numpy.full(len(inp["y"]), 1.0 - inp["params"]["transit_depth_min"])
    wild = inp["y"].copy()
    wild[137] = 3.0e4
    return {"on_depth_min": flat, "one_wild_value": wild}


@pytest.mark.gpu
@pytest.mark.parametrize("flux", ["on_depth_min", "one_wild_value"])
def test_retried_periods_keep_their_ticket(gpu, flux):
    """Band resolution and the exact retry enter the period loop again on the ticket they hold: they must not draw another
    (a lost ticket is a period nobody searches)."""
    inp = _inputs()
    y = _band_fluxes(inp)[flux]
    periods = _periods(inp, 2 * _blocks(gpu, inp) + 3)
    args = _args(inp, periods, y=y)
    out, retries = {}, {}
    for bits in (0,) + BITS:
        _set(gpu, bits)
        out[bits] = _three_launches(gpu, args)
        with _limit():
            gpu.execute(phase_clock=True)
            retries[bits] = gpu.phase_cycles()["stat_exact_retries"]      # slot 37
            _same(gpu.fetch(), out[bits][0], "the statistics launch")
    print("exact retries (slot 37) per claim_ahead:", retries)
    assert retries[1] > 0 and all(retries[bits] == retries[0] for bits in BITS), retries
    for bits in BITS:
        for k in range(3):
            _same(out[bits][k], out[0][k], "%s, claim_ahead %d, launch %d" % (flux, bits, k), counters=k == 2)


@pytest.mark.gpu
def test_survey_group_of_three_with_a_retrying_curve(gpu):
    """A group draws one ticket per period, not one per light curve; one curve goes through `curve_exact`."""
    inp = _inputs()
    periods = _periods(inp, 2 * _blocks(gpu, inp) + 3)
    ys = numpy.stack([inp["y"], _band_fluxes(inp)["one_wild_value"], _inputs()["y"][::-1]])
    dys = numpy.stack([inp["dy"]] * 3)
    groups = {}
    for bits in (0,) + BITS:
        _set(gpu, bits)
        with _limit():
            groups[bits] = [gpu.search_batch(inp["t"], ys, dys, periods, inp["table"], inp["params"]) for _ in range(2)]
            assert gpu.last_kernel() == "slim"
        _same(groups[bits][1], groups[bits][0], "the reading group against the filling one")
    for bits in BITS:
        _same(groups[bits][0], groups[0][0], "group, claim_ahead %d" % bits)
    _set(gpu, 1)
    for c in range(3):
        with _limit():
            single = gpu.search(*_args(inp, periods, y=ys[c]))
        _same(tuple(a[c] for a in groups[1][0]), single, "curve %d of the group against its single search" % c)


@pytest.mark.gpu
def test_the_512_thread_shape(gpu):
    """5121 points: the smallest series that takes two 512-thread workgroups a CU."""
    inp = _inputs(5121)
    args = _args(inp, _periods(inp, 37))
    _set(gpu, 0)
    want = _three_launches(gpu, args, "slim512")
    for bits in BITS:
        _set(gpu, bits)
        got = _three_launches(gpu, args, "slim512")
        for k in range(3):
            _same(got[k], want[k], "slim512, claim_ahead %d, launch %d" % (bits, k), counters=k == 2)


@pytest.mark.gpu
def test_the_whole_grid_against_every_period_alone(gpu):
    """A launch of one period never draws a second valid ticket; the grid's launch draws one per period."""
    inp = _inputs()
    grid = inp["periods"]
    _set(gpu, 1)
    with _limit():
        whole = gpu.search(*_args(inp, grid))
        assert gpu.last_kernel() == "slim"
    assert numpy.isfinite(whole[0]).all()
    alone = [[], [], []]
    with _limit(120):
        for p in grid:
            one = gpu.search(*_args(inp, numpy.asarray([p])))
            for dst, a in zip(alone, one[:3]):
                dst.append(a[0])
    _same(tuple(numpy.asarray(a) for a in alone), whole, "every period alone against the whole grid")
    _set(gpu, 0)
    with _limit():
        _same(gpu.search(*_args(inp, grid)), whole, "the whole grid, claim_ahead 0")


@pytest.mark.gpu
def test_a_classic_launch_between_two_four_slot_launches(gpu):
    """The classic kernel counts from zero on the same two queue words: every launch must leave them rewound."""
    inp = _inputs()
    args = _args(inp, _periods(inp, 2 * _blocks(gpu, inp) + 3))
    runs = {}
    for bits in (0, 1):
        out = []
        for slim in (1, 0, 1, 0, 1):
            with _limit():
                gpu.set_options(slim=slim, prune=0, screen32=0, claim_ahead=bits)
                out.append(gpu.search(*args, count_work=True))
                assert gpu.last_kernel() == ("slim" if slim else "resident")
        _same(out[2], out[0], "four-slot launches around a classic one", counters=True)
        _same(out[4], out[0], "four-slot launches around a classic one", counters=True)
        _same(out[3], out[1], "classic launches around a four-slot one", counters=True)
        runs[bits] = out
    for k in range(5):
        _same(runs[1][k], runs[0][k], "launch %d of the alternating context" % k, counters=True)
