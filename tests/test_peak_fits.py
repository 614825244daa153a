"""The peak-fit stage on the device (power_batch(peaks=K, peak_fits=True), tls_debug_peak_fits): every peak's final T0 fit
and statistics record against tests/peak_fits_spec.py bit for bit, the first peak against the main chain, the main chain's
own results untouched, at the group and slab edges (launch groups of 32 curves, slabs of 128 fits), at the T0 fit's series
sizes, and on injected records that reach every status.

The CPU oracle's T0 fit is compared as tests/test_power_batch_chain.py compares it: equal, or a near-tie within T0_TIE_RTOL
(the rotation path sums a fit's residuals in another order), near-ties at most 1 in 50 fits over the module; every fitted
candidate of every test goes to the oracle."""
import warnings

import numpy
import pytest

import count_lattice
import peak_fits_spec as spec
from tls_amd import _lib, survey, transit_model
from tls_amd.planning import search_inputs
from tls_amd.stats import calculate_fill_factor

pytestmark = pytest.mark.gpu

T0_TIE_RTOL = 1e-12
T = numpy.linspace(3.0, 43.0, 1920)          # 40 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))          # period [d], a / R_star


class Tally(object):
    fits = 0
    ties = 0


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _report_ties():
    yield
    print("\nT0 near-ties: %d of %d peak fits compared with the oracle" % (Tally.ties, Tally.fits))
    assert Tally.ties * 50 <= Tally.fits, (Tally.ties, Tally.fits)


def curve(s):
    """Light curve s (the same in every batch): both planets, epochs and radii its own, white noise."""
    rng = numpy.random.RandomState(1000 + s)
    f = numpy.ones(len(T))
    epochs = []
    for per, a in PLANETS:
        tp = T[0] + rng.uniform(0.1, 0.9) * per
        epochs.append(tp)
        f += transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3], "quadratic") - 1
    return f + rng.normal(0, 4e-4, len(T)), epochs


def batch(n_curves):
    return numpy.array([curve(s)[0] for s in range(n_curves)])


@pytest.fixture(scope="module")
def shared():
    """The plan every batch of this module gets (the first curve's) and the flux rows as the device sees them."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, _ = survey._batch_inputs(T, batch(33), None, dict(KW))
    return dict(inp=inp, y=y_rows, cache={})


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check_oracle(oracle_lib, inp, y, peak, T0, where):
    """T0 against the oracle's final T0 fit of the candidate: equal, or a near-tie."""
    o_T0, epochs, res = oracle_lib.final_t0_fit(inp["rows"][int(peak["row"])], float(peak["depth"]), inp["t"], y,
                                                float(peak["period"]), inp["params"]["T0_fit_margin"])
    Tally.fits += 1
    if T0 == o_T0:
        return
    j = numpy.flatnonzero(epochs == T0)
    assert len(j), (where, "T0 is not a trial epoch", T0, o_T0)
    assert res[j[0]] <= numpy.min(res) * (1 + T0_TIE_RTOL), (where, T0, o_T0, res[j[0]], numpy.min(res))
    Tally.ties += 1


def check_fits(ctx, oracle_lib, inp, y_rows, peaks, n_peaks, powers, got, label, cache=None):
    """Every entry of `got` ([n_curves, k] with T0, status and the statistics fields) equals the spec of its peak record."""
    fitted = 0
    for c in range(len(peaks)):
        for r in range(peaks.shape[1]):
            p = peaks[c, r]
            key = (c, int(p["index"]), int(p["row"]), r >= n_peaks[c])
            if cache is not None and key in cache:
                want = cache[key]
            else:
                want = spec.expected(ctx, inp, y_rows[c], p, r, int(n_peaks[c]), powers[c])
                if cache is not None:
                    cache[key] = want
            for k, v in want.items():
                expect_equal(got[k][c, r], v, (label, c, r, k))
            if want["status"] == spec.FITTED:
                check_oracle(oracle_lib, inp, y_rows[c], p, float(got["T0"][c, r]), (label, c, r))
                fitted += 1
    return fitted


def run(ctx, n_curves, k, **more):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return survey.power_batch(T, batch(n_curves), context=ctx, peaks=k, peak_fits=True, with_arrays=True, **more, **KW)


def test_two_planets(ctx, oracle_lib, shared):
    """Both injected planets are the first two candidates of every curve, each with its own epoch, duration and statistics."""
    summary, periods, chi2, row, depth, power, pk = run(ctx, 3, 8)
    peaks, n_peaks = pk["peaks"], pk["n_peaks"]
    assert len(periods) < 1000 and peaks.shape == (3, 8)
    assert peaks.dtype.names[-len(survey.peak_fit_fields()):] == survey.peak_fit_fields()
    for c in range(3):
        assert n_peaks[c] >= 2 and (peaks["status"][c, :2] == 0).all()
        found = set()
        for r in range(2):
            p = peaks[c, r]
            i = int(numpy.argmin([abs(p["period"] / per - 1) for per, _ in PLANETS]))
            per, tp = PLANETS[i][0], curve(c)[1][i]
            assert abs(p["period"] / per - 1) < 0.01, (c, r, p["period"])
            found.add(i)
            off = (p["T0"] - tp + 0.5 * p["period"]) % p["period"] - 0.5 * p["period"]
            assert abs(off) <= 0.5 * p["duration_days"], (c, r, p["T0"], tp, p["duration_days"])
            assert p["snr"] > 10 and p["transit_count"] >= 40.0 / per - 1 and 0.02 < p["rp_rs"] < 0.15
        assert found == {0, 1}
    fitted = check_fits(ctx, oracle_lib, shared["inp"], shared["y"], peaks, n_peaks, power, peaks, "two planets", shared["cache"])
    assert fitted >= 6


def test_rank_0_against_the_main_chain(ctx, shared):
    """Where the pick's two indices agree the first candidate IS the pick; and asking for the fits moves nothing else."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = batch(33)
        with_fits = survey.power_batch(T, f, context=ctx, peaks=4, statistics=True, peak_fits=True, **KW)
        without = survey.power_batch(T, f, context=ctx, peaks=4, statistics=True, **KW)
    summary, peaks = with_fits[0], with_fits[2]["peaks"]
    same = numpy.flatnonzero((summary["index_best"] == summary["index_power"]) & (summary["no_fit"] == 0))
    assert len(same)
    for c in same:
        assert peaks["index"][c, 0] == summary["index_power"][c] and peaks["status"][c, 0] == 0
        for k in ("T0", "rp_rs") + _lib.TRANSIT_STATS_FIELDS:
            expect_equal(peaks[k][c, 0], summary[k][c], (c, k))
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(with_fits[1], without[1], "periods")
    assert (with_fits[2]["n_peaks"] == without[2]["n_peaks"]).all()
    for k in without[2]["peaks"].dtype.names:
        expect_equal(peaks[k], without[2]["peaks"][k], k)
    # ... and neither do the fits need the statistics of the best pick
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alone = survey.power_batch(T, f[:5], context=ctx, peaks=4, peak_fits=True, **KW)
    assert "snr" not in alone[0].dtype.names
    for k in peaks.dtype.names:
        expect_equal(alone[2]["peaks"][k], peaks[k][:5], k)


@pytest.mark.parametrize("n_curves,k", [(1, 3), (32, 3), (33, 3), (16, 8), (17, 8), (2, 1), (2, 32)])
def test_group_and_slab_edges(ctx, oracle_lib, shared, n_curves, k):
    """One curve, a whole group and a group and one; 128 fits (one whole slab) and 136 (the slab's end inside curve 16's
    candidates); one candidate a curve and the most."""
    summary, periods, chi2, row, depth, power, pk = run(ctx, n_curves, k)
    peaks, n_peaks = pk["peaks"], pk["n_peaks"]
    assert peaks.shape == (n_curves, k)
    fitted = check_fits(ctx, oracle_lib, shared["inp"], shared["y"], peaks, n_peaks, power, peaks, (n_curves, k),
                        shared["cache"])
    assert fitted >= n_curves * min(k, 2)
    past = numpy.arange(k)[None, :] >= n_peaks[:, None]
    assert (peaks["status"][past] == 1).all() and numpy.isnan(peaks["T0"][past]).all() and numpy.isnan(peaks["snr"][past]).all()


def reported_rows(table):
    first = {}
    for r, w in enumerate(table.width):
        first.setdefault(int(w), r)
    return sorted(first.values())


def records(inp, rng, n_curves, k, rows=None):
    """Peak records nobody searched for: indices spread over the grid, a template row of some duration each."""
    good = reported_rows(inp["table"]) if rows is None else rows
    n_p = len(inp["periods"])
    rec = numpy.zeros((n_curves, k), dtype=_lib.PEAK_DTYPE)
    rec["index"] = rng.randint(1, n_p - 1, (n_curves, k))
    rec["period"] = inp["periods"][rec["index"]]
    rec["row"] = rng.choice(good, (n_curves, k))
    rec["depth"] = 1 - rng.uniform(5e-4, 4e-3, (n_curves, k))
    rec["chi2"] = rng.uniform(900, 1000, (n_curves, k))
    power = numpy.array([numpy.convolve(rng.normal(0, 1, n_p + 8), numpy.ones(9) / 9, mode="valid") for _ in range(n_curves)])
    rec["power"] = numpy.take_along_axis(power, rec["index"], axis=1)
    return rec, power


def debug_fits(ctx, inp, y, rec, n_peaks, power, max_epochs=None, **kw):
    t = inp["t"]
    # (the two tables from the scalar expressions of power() themselves, not from stats.count_roots)
    root = numpy.array([float(k) ** 0.5 for k in range(len(t) + 1)])
    root_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(len(t) + 1)])
    if max_epochs is None:
        max_epochs = survey._max_epochs(t, inp["periods"])
    return ctx.debug_peak_fits(y, rec, n_peaks, power, inp["table"].duration, calculate_fill_factor(t), root, max_epochs,
                               root_count=root_count, **kw)


def with_a_repeated_width(inp):
    """The plan inputs with a table whose row 1 has row 0's width: row 1 is no width's first row."""
    from tls_amd.template import TemplateTable
    tab = inp["table"]
    overview = numpy.zeros(tab.n_rows, dtype=[("duration", "f8"), ("width_in_samples", "i8"), ("overshoot", "f8")])
    overview["duration"], overview["width_in_samples"], overview["overshoot"] = tab.duration, tab.width, tab.overshoot
    overview["width_in_samples"][1] = overview["width_in_samples"][0]
    rows = list(inp["rows"])
    rows[1] = rows[0]
    return dict(inp, table=TemplateTable(overview, rows), rows=rows)


def tiny_plan(n):
    """A plan on n points (the planner's template cache needs more): five rows of widths 2 to 6, a dozen periods."""
    from tls_amd.template import TemplateTable
    t = numpy.linspace(3.0, 33.0, n)
    widths = numpy.arange(2, 7)
    rows = [1 - 0.5 * numpy.sin(numpy.pi * (numpy.arange(w) + 0.5) / w) ** 0.5 for w in widths]
    overview = numpy.zeros(len(rows), dtype=[("duration", "f8"), ("width_in_samples", "i8"), ("overshoot", "f8")])
    overview["duration"] = widths / float(n)
    overview["width_in_samples"] = widths
    overview["overshoot"] = [1 / (2 - numpy.mean(r) / numpy.min(r)) for r in rows]
    params = dict(transit_depth_min=1e-5, R_star_min=0.13, R_star_max=3.5, M_star_min=0.1, M_star_max=1.0, T0_fit_margin=0.01)
    return dict(t=t, periods=numpy.linspace(4.0, 9.0, 12), table=TemplateTable(overview, rows), rows=rows, params=params)


@pytest.mark.parametrize("n", [10223, 10224, 15, 17])
def test_t0_fit_shapes(ctx, oracle_lib, n):
    """Both sides of the T0 fit's LDS boundary (10 223 points are the most it keeps resident) and of kT0RotMinPoints = 16,
    below which no fit takes the rotation path: two curves, two candidates each."""
    rng = numpy.random.RandomState(n)
    if n > 100:
        t = numpy.linspace(3.0, 33.0, n)
        y = numpy.array([transit_model.light_curve(t, 3.4 + s, 4.1 + s, 0.06, 12, 89.8, 0, 90, [0.4, 0.3], "quadratic")
                         + rng.normal(0, 4e-4, n) for s in range(2)])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            inp = search_inputs(t, y[0], period_min=2.5, period_max=7.0, oversampling_factor=1, T0_fit_margin=0.05)
        y[0] = inp["y"]
    else:
        inp = tiny_plan(n)
        y = 1 + rng.normal(0, 1e-3, (2, n))
    ctx.prepare(inp["t"], y[0], numpy.full(n, numpy.std(y[0])), inp["periods"], inp["table"], inp["params"])
    rec, power = records(inp, rng, 2, 2)
    n_peaks = numpy.array([2, 2])
    got, epochs, residuals, n_epochs = debug_fits(ctx, inp, y, rec, n_peaks, power, with_fits=True)
    assert (got["status"] == 0).all() and (n_epochs >= 1).all()
    assert check_fits(ctx, oracle_lib, inp, y, rec, n_peaks, power, got, ("n", n)) == 4
    # the trial grid of every fit is numpy.linspace from min(t) over one period
    for c in range(2):
        for r in range(2):
            m = int(n_epochs[c, r])
            expect_equal(epochs[c, r, :m], numpy.linspace(inp["t"].min(), inp["t"].min() + rec["period"][c, r], m), (c, r))
            assert got["T0"][c, r] == epochs[c, r, int(numpy.argmin(residuals[c, r, :m]))]


def test_injected_records(ctx, oracle_lib, shared):
    inp, k = shared["inp"], 4
    rng = numpy.random.RandomState(77)
    y = numpy.array([shared["y"][0], shared["y"][1], shared["y"][2], 1 + rng.normal(0, 4e-4, len(T))])   # (the last: noise only)
    ctx.prepare(inp["t"], y[0], numpy.full(len(T), numpy.std(y[0])), inp["periods"], inp["table"], inp["params"])
    rec, power = records(inp, rng, 4, k)
    n_peaks = numpy.array([0, 2, 4, 4])
    rec["row"][2, 1] = -1                      # the search fitted nothing at this index
    rec[2, 3] = rec[2, 2]                      # two candidates at one index
    got = debug_fits(ctx, inp, y, rec, n_peaks, power)
    assert (got["status"][0] == 1).all() and (got["status"][1] == [0, 0, 1, 1]).all() and (got["status"][2] == [0, 2, 0, 0]).all()
    for k_ in got.dtype.names:
        if k_ != "status":
            assert numpy.isnan(got[k_][0]).all() and numpy.isnan(got[k_][1, 2:]).all() and numpy.isnan(got[k_][2, 1]), k_
    assert got[2, 2].tobytes() == got[2, 3].tobytes()
    assert (got["status"][3] == 0).all() and numpy.isfinite(got["T0"][3]).all()
    assert check_fits(ctx, oracle_lib, inp, y, rec, n_peaks, power, got, "injected") == 9
    worse = rec.copy()
    worse["row"][3, 3] = inp["table"].n_rows
    with pytest.raises(RuntimeError, match="row out of range"):
        debug_fits(ctx, inp, y, worse, n_peaks, power)
    debug_fits(ctx, inp, y, worse, numpy.array([0, 2, 4, 3]), power)        # (a record past n_peaks is never read)
    # either k ** 0.5 table missing or short: an error
    tables = (numpy.array([float(i) ** 0.5 for i in range(len(T) + 1)]),
              numpy.array([float(numpy.sum(i) ** 0.5) for i in range(len(T) + 1)]))
    common = (y, rec, n_peaks, power, inp["table"].duration, calculate_fill_factor(inp["t"]))
    cap = survey._max_epochs(inp["t"], inp["periods"])
    for a, b in ((tables[0], tables[1][:-1]), (tables[0][:-1], tables[1])):
        with pytest.raises(RuntimeError, match="must cover"):
            ctx.debug_peak_fits(*common, a, cap, root_count=b)
    assert ctx.debug_peak_fits(*common, tables[0], cap, root_count=tables[1]).tobytes() == got.tobytes()
    assert ctx.debug_peak_fits(*common, tables[0], cap).tobytes() == got.tobytes()     # (the binding's own second table)
    # ... and NULL at the C entry: TLS_E_ARG, the fits untouched
    import ctypes
    raw_rec = numpy.zeros(rec.shape, dtype=_lib.PEAK_DTYPE)
    for name in _lib.PEAK_DTYPE.names:
        raw_rec[name] = rec[name]
    dur, yy, pw = (numpy.ascontiguousarray(v, dtype=float) for v in (inp["table"].duration, y, power))
    for root_p, count_p in ((_lib._dp(tables[0]), None), (None, _lib._dp(tables[1]))):
        fits = numpy.zeros(rec.shape, dtype=_lib.PEAK_FIT_DTYPE)
        fits.view(numpy.float64)[:] = -7.0
        rc = ctx._lib.tls_debug_peak_fits(ctx._h, _lib._dp(yy), len(yy), raw_rec.ctypes.data_as(ctypes.c_void_p),
                                          _lib._ip(numpy.ascontiguousarray(n_peaks, dtype=numpy.int64)), k, _lib._dp(pw),
                                          _lib._dp(dur), len(dur), calculate_fill_factor(inp["t"]), root_p, count_p,
                                          len(tables[0]), cap, fits.ctypes.data_as(ctypes.c_void_p), None, None, None)
        assert rc == -1 and (fits.view(numpy.float64) == -7.0).all()
    # more epochs than max_epochs: an error, not a truncated record
    short = float(inp["periods"].min())
    assert 40.0 / short > 30
    worse = rec.copy()
    worse["index"][1, 1] = int(numpy.argmin(inp["periods"]))
    worse["period"][1, 1] = short
    with pytest.raises(RuntimeError, match="max_epochs"):
        debug_fits(ctx, inp, y, worse, n_peaks, power, max_epochs=30)
    # a row that starts no template duration (this plan's widths are all distinct: a table whose second row repeats the
    # first row's width): an error, as in the main chain
    again = with_a_repeated_width(inp)
    assert reported_rows(again["table"])[:2] == [0, 2]
    ctx.prepare(inp["t"], y[0], numpy.full(len(T), numpy.std(y[0])), inp["periods"], again["table"], inp["params"])
    worse = rec.copy()
    worse["row"] = numpy.where(rec["row"] == 1, 2, rec["row"])
    debug_fits(ctx, again, y, worse, n_peaks, power)
    worse["row"][3, 3] = 1
    with pytest.raises(RuntimeError, match="not the first row"):
        debug_fits(ctx, again, y, worse, n_peaks, power)


def lattice_candidates(inp, n_curves, k, seed):
    """Peak records from tests/count_lattice.py: the lattice picks whose odd or even in-transit count, at the lattice's own
    T0, is one where the two forms of k ** 0.5 differ (or one of the fixed list), thinned evenly to n_curves * k, as
    candidates of period and duration -- the T0 is the fit's to find.  The plan has fewer rows than the lattice has
    durations: duration j stands in the row_duration table at the j-th row that starts a template width, j < that many."""
    t = inp["t"]
    good = reported_rows(inp["table"])
    targets = sorted(set(count_lattice.disagreeing_counts(len(t))) | set(count_lattice.FIXED))
    table = count_lattice.lattice_counts(t)
    lattice = count_lattice.lattice()
    at = [i for i in numpy.flatnonzero(numpy.isin(table, targets).any(axis=1)) if lattice[i][2] < len(good)]
    assert len(at) >= n_curves * k
    at = [at[i] for i in numpy.linspace(0, len(at) - 1, n_curves * k).astype(int)]
    row_duration = numpy.full(inp["table"].n_rows, count_lattice.DURATIONS[0])
    row_duration[good] = count_lattice.DURATIONS[:len(good)]
    rng = numpy.random.RandomState(seed)
    rec, power = records(inp, rng, n_curves, k)
    rec["period"] = numpy.array([lattice[i][0] for i in at]).reshape(n_curves, k)
    rec["row"] = numpy.array([good[lattice[i][2]] for i in at]).reshape(n_curves, k)
    return rec, power, row_duration, targets


def test_candidates_at_counts_where_the_two_roots_differ(ctx):
    """Candidates on four noisy curves of count_lattice.TIME, 32 ranks each, steered to the in-transit counts at which
    numpy.sum(k) ** 0.5 (the odd and even depth errors) is not float(k) ** 0.5 (snr, pink noise): every fit equals the spec,
    whose errors are stats.intransit_stats' own, and rank 0 of every curve -- and every fit that reached such a count --
    equals the main chain's record for the same pick (tls_debug_transit_stats at the fitted T0).

    A fit puts its T0 wherever the noise has its minimum, so a candidate's counts scatter around the lattice's; the test
    asks that 3 distinct members of the targets are reached by the fits, as an odd or an even count.  (128 candidates with
    two counts each between about 10 and 110, 7 targets or more among those values: a dozen hits are expected, and a test
    that reached fewer than 3 would say little.)"""
    n_curves, k = 4, 32
    t = count_lattice.TIME
    rng = numpy.random.RandomState(41)
    y = 1 + rng.normal(0, 4e-4, (n_curves, len(t)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp = search_inputs(t, y[0], period_min=1.5, period_max=9.0, oversampling_factor=1)
    y[0] = inp["y"]
    ctx.prepare(inp["t"], y[0], numpy.full(len(t), numpy.std(y[0])), inp["periods"], inp["table"], inp["params"])
    rec, power, row_duration, targets = lattice_candidates(inp, n_curves, k, 43)
    n_peaks = numpy.full(n_curves, k)
    root = numpy.array([float(i) ** 0.5 for i in range(len(t) + 1)])
    root_count = numpy.array([float(numpy.sum(i) ** 0.5) for i in range(len(t) + 1)])
    fill = calculate_fill_factor(t)
    got = ctx.debug_peak_fits(y, rec, n_peaks, power, row_duration, fill, root, 32, root_count=root_count)
    assert (got["status"] == 0).all()
    reached, again, hits = set(), [], 0
    for c in range(n_curves):
        for r in range(k):
            p = rec[c, r]
            T0 = spec.candidate_T0(ctx, inp, y[c], float(p["period"]), float(p["depth"]), int(p["row"]))
            duration = row_duration[int(p["row"])]
            want = spec.candidate_stats(t, y[c], float(p["period"]), T0, duration, inp["periods"], power[c], int(p["index"]))
            odd, even, _ = count_lattice.counts(t, float(p["period"]), T0, duration)
            expect_equal(got["T0"][c, r], T0, (c, r, "T0"))
            for name, v in want.items():
                expect_equal(got[name][c, r], v, (c, r, name, "odd %d even %d" % (odd, even)))
            hit = {odd, even} & set(targets)
            reached |= hit
            hits += bool(hit)
            if hit or r == 0:
                again.append((c, r))
    print("\n%d of %d fits have an odd or even count among the targets; distinct members reached: %s"
          % (hits, n_curves * k, sorted(reached)))
    assert len(reached) >= 3
    # the main chain on the same picks: one record, whichever stage formed it
    for c in range(n_curves):
        mine = [r for cc, r in again if cc == c]
        stats, _, _ = ctx.debug_transit_stats(
            numpy.repeat(y[c][None, :], len(mine), axis=0), rec["period"][c, mine], got["T0"][c, mine], rec["row"][c, mine],
            rec["depth"][c, mine], 0, rec["index"][c, mine], numpy.repeat(power[c][None, :], len(mine), axis=0), row_duration,
            fill, root, 32, root_count=root_count)
        for name in _lib.TRANSIT_STATS_FIELDS:
            expect_equal(stats[name], got[name][c, mine], (c, name, "main chain"))


def test_two_contexts_equal_the_one_device_call():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = batch(33)
        one = survey.power_batch(T, f, device=0, peaks=3, statistics=True, peak_fits=True, **KW)
        two = survey.power_batch(T, f, devices=[0, 0], peaks=3, statistics=True, peak_fits=True, **KW)
    for k in one[0].dtype.names:
        expect_equal(two[0][k], one[0][k], k)
    assert sorted(one[2]) == sorted(two[2]) == ["n_peaks", "peaks"]
    expect_equal(two[2]["n_peaks"], one[2]["n_peaks"], "n_peaks")
    assert one[2]["peaks"].dtype == two[2]["peaks"].dtype
    for k in one[2]["peaks"].dtype.names:
        expect_equal(two[2]["peaks"][k], one[2]["peaks"][k], k)
