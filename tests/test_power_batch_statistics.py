"""Survey-mode power()'s per-transit vetting statistics on the device (tls_power_batch_stats, tls_debug_transit_stats): every
field bit-equal to what power() reports for the same light curve, and to the host sequence of api.py:175-241 on injected
picks that reach the edge branches -- among them the in-transit counts at which the two forms of k ** 0.5 that power()
takes of a count differ (tests/count_lattice.py)."""
import time
import warnings

import numpy
import pytest

import count_lattice
import tls_amd
from tls_amd import _lib, survey, synthetic, transit_model
from tls_amd.helpers import transit_mask
from tls_amd.stats import (FAP, _intransit_fluxes, all_transit_times, calculate_fill_factor,
                           calculate_transit_duration_in_days, count_stats, intransit_stats, period_uncertainty, snr_stats)

pytestmark = pytest.mark.gpu

# summary field -> (results key, index into a tuple-valued key or None)
RESULT_OF = {
    "period_uncertainty": ("period_uncertainty", None), "duration_days": ("duration", None),
    "depth_mean": ("depth_mean", 0), "depth_mean_std": ("depth_mean", 1),
    "depth_mean_even": ("depth_mean_even", 0), "depth_mean_even_std": ("depth_mean_even", 1),
    "depth_mean_odd": ("depth_mean_odd", 0), "depth_mean_odd_std": ("depth_mean_odd", 1),
    "snr": ("snr", None), "odd_even_mismatch": ("odd_even_mismatch", None), "transit_count": ("transit_count", None),
    "distinct_transit_count": ("distinct_transit_count", None), "empty_transit_count": ("empty_transit_count", None),
    "in_transit_count": ("in_transit_count", None), "after_transit_count": ("after_transit_count", None),
    "before_transit_count": ("before_transit_count", None), "rp_rs": ("rp_rs", None), "FAP": ("FAP", None),
    "chi2red_min": ("chi2red_min", None),
}
PER_TRANSIT = ("transit_times", "per_transit_count", "transit_depths", "transit_depths_uncertainties", "snr_per_transit",
               "snr_pink_per_transit")


def gapped_time():
    t = numpy.linspace(3.0, 33.0, 720)
    return t[(t < 14.0) | (t > 18.5)]   # a data gap: some epochs hold no point


def batch(t, n_curves, seed):
    rng = numpy.random.RandomState(seed)
    fluxes, dys = [], []
    for s in range(n_curves):
        per = float(rng.uniform(1.6, 6.0))
        f = transit_model.light_curve(t, 3.2 + rng.uniform(0, 1), per, float(rng.uniform(0.03, 0.08)), 12, 89.8, 0, 90,
                                      [0.4, 0.3], "quadratic") + rng.normal(0, 4e-4, len(t))
        if s == 5:
            f = numpy.ones(len(t))     # flat: nothing passes transit_depth_min
            f[::7] += 1e-7
        fluxes.append(f)
        dys.append(rng.uniform(0.8, 1.3, len(t)) * 4e-4)
    return numpy.array(fluxes), numpy.array(dys)


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=what)


@pytest.mark.parametrize("weights", [False, True])
def test_statistics_equal_power_per_curve(weights):
    """70 light curves in three launch groups: every statistics field and every per-transit array equals the results of
    transitleastsquares(t, y_k[, dy_k]).power(same kwargs), NaN for NaN, for curves spread over the groups."""
    ctx = _lib.Context(0)
    t = gapped_time()
    fluxes, dys = batch(t, 70, 11)
    dy_batch = dys if weights else None
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        summary, periods, pt = survey.power_batch(t, fluxes, dy_batch, context=ctx, statistics=True, per_transit=True, **kw)
        assert len(summary) == 70 and summary["no_fit"][5] == 1
        empties = 0
        for s in (0, 1, 5, 17, 31, 32, 33, 47, 63, 64, 65, 69):
            one = tls_amd.transitleastsquares(t, fluxes[s], None if dy_batch is None else dy_batch[s], verbose=False).power(
                context=ctx, verbose=False, show_progress_bar=False, **kw)
            rec = summary[s]
            expect_equal([rec["T0"], rec["period"]], [one.T0, one.period], "curve %d: T0, period" % s)
            for field, (key, i) in RESULT_OF.items():
                want = one[key] if i is None else one[key][i]
                expect_equal(rec[field], want, "curve %d: %s" % (s, field))
            if rec["no_fit"]:
                assert pt["n_epochs"][s] == 0 and numpy.all(numpy.isnan(pt["transit_times"][s]))
                continue
            e = int(pt["n_epochs"][s])
            assert e == len(one.transit_times) == rec["transit_count"]
            for key in PER_TRANSIT:
                expect_equal(pt[key][s, :e], one[key], "curve %d: %s" % (s, key))
                assert numpy.all(numpy.isnan(pt[key][s, e:])), (s, key)
            empties += int(one.empty_transit_count)
        assert empties > 0   # the gap emptied some epochs
    ctx.close()


def host_stats(t, y, period, T0, duration, periods, power):
    """api.py:175-241 on the host (stats.py), the pink noise in its numpy form: the statistics record and the rows."""
    with warnings.catch_warnings(), numpy.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        transit_times = all_transit_times(T0, t, period)
        fill = calculate_fill_factor(t)
        d = calculate_transit_duration_in_days(t, period, transit_times, duration, fill_factor=fill)
        chunks = _intransit_fluxes(t, y, transit_times, d)
        flux_ootr = y[~transit_mask(t, period, 2 * duration, T0)]
        (mo, me, mos, mes, fo, fe, ptc, td, tdu) = intransit_stats(t, y, transit_times, d, chunks=chunks)
        all_flux = numpy.concatenate([fo, fe])
        std_ootr = numpy.std(flux_ootr)
        spt, sppt = snr_stats(t=t, y=y, period=period, duration=duration, T0=T0, transit_times=transit_times,
                              transit_duration_in_days=d, per_transit_count=ptc, chunks=chunks, flux_ootr=flux_ootr,
                              mean_flux=td, std_ootr=std_ootr)
        dm = numpy.mean(all_flux)
        dms = numpy.std(all_flux) / numpy.sum(ptc) ** (0.5)
        snr = ((1 - dm) / std_ootr) * len(all_flux) ** (0.5)
        n_in, n_after, n_before = count_stats(t, y, transit_times, d)
        mismatch = abs(mo - me) / (mos + mes)
        E = len(transit_times)
        empty = numpy.count_nonzero(ptc == 0)
        rec = dict(period_uncertainty=period_uncertainty(periods, power), duration_days=d, depth_mean=dm, depth_mean_std=dms,
                   depth_mean_even=me, depth_mean_even_std=mes, depth_mean_odd=mo, depth_mean_odd_std=mos, snr=snr,
                   odd_even_mismatch=mismatch, transit_count=E, distinct_transit_count=E - empty, empty_transit_count=empty,
                   in_transit_count=n_in, after_transit_count=n_after, before_transit_count=n_before)
        rows = (transit_times, ptc, td, tdu, spt, sppt)
        width = int(numpy.mean(ptc))
    return rec, rows, dict(width=width, n_ootr=len(flux_ootr), filled=E - empty, odd=len(fo), even=len(fe))


def prepared(ctx, t, flux, **kw):
    inp = synthetic.search_inputs(t, flux, **kw)
    ctx.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    return inp


def run_injected(ctx, inp, y, picks, row_duration, powers, max_epochs=4000):
    """picks: (period, T0, best_row) per curve; every curve's statistics from the device and from the host."""
    t = inp["t"]
    n_c = len(picks)
    # (the two tables from the scalar expressions of power() themselves, not from stats.count_roots)
    root = numpy.array([float(k) ** 0.5 for k in range(len(t) + 1)])
    root_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(len(t) + 1)])
    index_power = [int(numpy.argmax(p)) for p in powers]
    stats, rows, n_ep = ctx.debug_transit_stats(
        numpy.repeat(y[None, :], n_c, axis=0), [p[0] for p in picks], [p[1] for p in picks], [p[2] for p in picks],
        0.999, 0, index_power, numpy.array(powers), row_duration, calculate_fill_factor(t), root, max_epochs,
        root_count=root_count)
    infos = []
    for c, (period, T0, best_row) in enumerate(picks):
        rec, want_rows, info = host_stats(t, y, period, T0, row_duration[best_row], inp["periods"], powers[c])
        where = "pick %d (period %r, T0 %r, duration %r; %d odd and %d even points in transit)" % (
            c, period, T0, float(row_duration[best_row]), info["odd"], info["even"])
        for k, v in rec.items():
            expect_equal(stats[k][c], v, "%s: %s" % (where, k))
        e = int(n_ep[c])
        assert e == rec["transit_count"]
        for i, v in enumerate(want_rows):
            expect_equal(rows[c, i, :e], v, "%s: %s" % (where, PER_TRANSIT[i]))
            assert numpy.all(numpy.isnan(rows[c, i, e:]))
        infos.append(info)
    return stats, infos


def test_injected_picks_reach_every_branch():
    ctx = _lib.Context(0)
    t = gapped_time()
    _, f = synthetic.light_curve(30.0, 24, 2e-4, per=4.321, rp=0.05, a=12)
    f = numpy.interp(t, numpy.linspace(3.0, 33.0, len(f)), f)
    inp = prepared(ctx, t, f, period_min=1.5, period_max=9.0, oversampling_factor=2)
    y, n_p = inp["y"], len(inp["periods"])
    rng = numpy.random.RandomState(3)
    smooth = numpy.exp(-0.5 * ((numpy.arange(n_p) - n_p / 2) / 40.0) ** 2) + rng.uniform(0, 0.05, n_p)
    first_peak = smooth[::-1].copy()
    first_peak[0] = 10.0
    first_peak[-1] = 6.0                    # the lower walk wraps to the end of the grid and stops one further
    last_peak = smooth.copy()
    last_peak[-1] = 10.0                    # the upper walk runs past the end: inf
    flat_power = numpy.ones(n_p)            # both walks run off: inf
    wide = numpy.full(inp["table"].n_rows, 0.499)   # a fractional duration that masks nearly all of every period
    dur = inp["table"].duration
    picks = [
        (4.321, 3.0 + 1.1, 3, smooth),                   # an ordinary pick
        (4.321, 3.0 - 1.3, 3, first_peak),              # T0 before min(t): the first epoch moves one period on
        (20.0, 19.5, 3, last_peak),                      # a single transit: no odd epoch, mismatch NaN
        (25.0, 16.0, 0, flat_power),                     # its one epoch inside the gap: all epochs empty, width 0
    ]
    stats, infos = run_injected(ctx, inp, y, [p[:3] for p in picks], dur, [p[3] for p in picks])
    assert stats["transit_count"][2] == 1 and infos[2]["odd"] == 0
    assert numpy.isnan(stats["odd_even_mismatch"][2])
    assert stats["distinct_transit_count"][3] == 0 and infos[3]["width"] == 0
    assert numpy.isinf(stats["period_uncertainty"][2]) and numpy.isinf(stats["period_uncertainty"][3])
    assert numpy.isfinite(stats["period_uncertainty"][1]) and stats["period_uncertainty"][1] < 0
    # pink-noise window longer than the out-of-transit flux
    stats, infos = run_injected(ctx, inp, y, [(1.0, 3.4, 2)], wide, [smooth])
    assert infos[0]["width"] > infos[0]["n_ootr"] >= 0
    # more epochs than max_epochs: an error, not a truncated record
    with pytest.raises(RuntimeError, match="max_epochs"):
        run_injected(ctx, inp, y, [(1.0, 3.4, 2)], dur, [smooth], max_epochs=20)
    ctx.close()


def test_more_than_512_filled_epochs_follow_the_segmented_form():
    ctx = _lib.Context(0)
    t = numpy.linspace(3.0, 63.0, 8640)
    rng = numpy.random.RandomState(5)
    y = 1 + rng.normal(0, 3e-4, len(t))
    inp = prepared(ctx, t, y, period_min=2.0, period_max=12.0, oversampling_factor=1)
    n_p = len(inp["periods"])
    power = numpy.exp(-0.5 * ((numpy.arange(n_p) - n_p / 3) / 30.0) ** 2)
    wide = numpy.full(inp["table"].n_rows, 0.4)
    stats, infos = run_injected(ctx, inp, inp["y"], [(0.1, 3.05, 0), (0.23, 3.1, 0)], wide, [power, power])
    assert infos[0]["filled"] > 512 and infos[1]["filled"] <= 512
    ctx.close()


@pytest.fixture(scope="module")
def lattice_table():
    """Odd and even in-transit count of every pick of count_lattice.lattice(): host work alone."""
    return count_lattice.lattice_counts()


def run_lattice(ctx, inp, y, picks, power):
    """run_injected on picks (period, T0, index into count_lattice.DURATIONS): the plan has fewer template rows than the
    lattice has durations, so the picks go by the row_duration table that holds theirs, in slabs of 256; the info of every
    pick, in the order of `picks`."""
    tables, table_of, row_of = count_lattice.duration_tables(inp["table"].n_rows)
    infos = [None] * len(picks)
    for i, table in enumerate(tables):
        mine = [c for c, p in enumerate(picks) if table_of[p[2]] == i]
        for lo in range(0, len(mine), 256):
            slab = mine[lo:lo + 256]
            injected = [(picks[c][0], picks[c][1], int(row_of[picks[c][2]])) for c in slab]
            _, got = run_injected(ctx, inp, y, injected, table, [power] * len(slab), max_epochs=32)
            for c, info in zip(slab, got):
                infos[c] = info
    return infos


def lattice_inputs(ctx):
    t = count_lattice.TIME
    rng = numpy.random.RandomState(19)
    inp = prepared(ctx, t, 1 + rng.normal(0, 4e-4, len(t)), period_min=1.5, period_max=9.0, oversampling_factor=1)
    n_p = len(inp["periods"])
    power = numpy.exp(-0.5 * ((numpy.arange(n_p) - n_p / 3) / 30.0) ** 2) + rng.uniform(0, 0.05, n_p)
    return inp, power


def test_odd_and_even_counts_where_the_two_roots_differ(lattice_table):
    """power() divides the odd and the even depth error by numpy.sum(len(x)) ** 0.5, the power of a numpy integer scalar, and
    forms snr and the pink noise with float(k) ** 0.5; at the counts D the two differ by one ulp.  Picks chosen on the host,
    before any device call, so that their odd or even count is a member of D (formed with the running numpy) or of the fixed
    list 19, 51, 63, 75, 76, 78, 107: every field and every per-transit row equals the host's.  A kernel that read one table
    for both fails here in depth_mean_odd_std or depth_mean_even_std wherever D is not empty; where it is empty the test
    runs on the fixed list and cannot tell the two roots apart."""
    t = count_lattice.TIME
    lattice = count_lattice.lattice()
    D = count_lattice.disagreeing_counts(len(t))
    print("\nnumpy %s: numpy.sum(k) ** 0.5 != float(k) ** 0.5 at len(D) = %d counts k <= %d: %s ..."
          % (numpy.__version__, len(D), len(t), D[:12]))
    targets = sorted(set(D) | set(count_lattice.FIXED))
    keep, odd_reached, even_reached = count_lattice.covering(targets, lattice_table)
    print("distinct members reached: %d as odd counts %s, %d as even counts %s, by %d picks"
          % (len(odd_reached), sorted(odd_reached), len(even_reached), sorted(even_reached), len(keep)))
    assert len(odd_reached) >= 5 and len(even_reached) >= 5
    assert len(keep) <= 64
    picks = [lattice[i] for i in keep]
    # ... a pick without an odd epoch, and one whose epochs hold 0, 1 and 2 points
    single = (20.0, 19.5, 3)
    assert count_lattice.counts(t, single[0], single[1], count_lattice.DURATIONS[3])[0] == 0
    sparse = next(p for p in lattice if p[2] < 8 and
                  set(count_lattice.counts(t, p[0], p[1], count_lattice.DURATIONS[p[2]])[2].tolist()) == {0, 1, 2})
    picks += [single, sparse]
    ctx = _lib.Context(0)
    inp, power = lattice_inputs(ctx)
    t0 = time.perf_counter()
    infos = run_lattice(ctx, inp, inp["y"], picks, power)
    print("%d picks compared in %.2f s" % (len(picks), time.perf_counter() - t0))
    for i, info in zip(keep, infos):
        assert (info["odd"], info["even"]) == tuple(lattice_table[i])     # (the counts the picks were chosen for)
    assert {info["odd"] for info in infos} >= odd_reached and {info["even"] for info in infos} >= even_reached
    assert infos[-2]["odd"] == 0 and infos[-2]["even"] > 0
    ctx.close()


def test_a_sweep_of_counts_up_to_146(lattice_table):
    """Every 6th pick of the lattice (882 picks: 133 distinct odd and even counts from 0 to 146, empty epochs and the gap
    included) through the same comparison, whatever their counts are: no choice of examples decides what is seen.  Stride 6:
    the host side (host_stats of every pick) takes about 0.8 s, the whole test about 2 s."""
    lattice = count_lattice.lattice()
    chosen = list(range(0, len(lattice), 6))
    assert len(chosen) == 882
    seen = set(lattice_table[chosen].ravel().tolist())
    assert min(seen) == 0 and max(seen) >= 140 and len(seen) >= 120
    ctx = _lib.Context(0)
    inp, power = lattice_inputs(ctx)
    t0 = time.perf_counter()
    infos = run_lattice(ctx, inp, inp["y"], [lattice[i] for i in chosen], power)
    print("\n%d picks compared in %.2f s" % (len(chosen), time.perf_counter() - t0))
    for i, info in zip(chosen, infos):
        assert (info["odd"], info["even"]) == tuple(lattice_table[i])
    empty = [0 in count_lattice.counts(count_lattice.TIME, p, T0, count_lattice.DURATIONS[j])[2]
             for p, T0, j in (lattice[i] for i in chosen)]
    assert 100 < sum(empty) < len(chosen)      # (epochs inside the gap, and picks without one)
    ctx.close()


PLANTED_SEED = 9      # (of seeds 0 to 29 one that puts 6 curves on a count of D under numpy 2.2.6; worked out on the host,
                      # with the CPU oracle's search in power())
PLANTED_KW = dict(period_min=3.0, period_max=6.0, oversampling_factor=1)


def planted_batch(n_curves=24, seed=PLANTED_SEED):
    """Light curves on count_lattice.TIME with one planet each: durations spread evenly from 0.1 d to 0.5 d (a / R_star from
    the period), so that the odd and even in-transit counts of the picks spread from about 12 to 80."""
    t = count_lattice.TIME
    rng = numpy.random.RandomState(seed)
    fluxes = []
    for s in range(n_curves):
        per = float(rng.uniform(3.3, 5.7))
        days = 0.1 + 0.4 * s / (n_curves - 1)
        f = transit_model.light_curve(t, 3.2 + float(rng.uniform(0, 1)) * per, per, float(rng.uniform(0.05, 0.08)),
                                      per / (numpy.pi * days), 90.0, 0, 90, [0.4, 0.3], "quadratic")
        fluxes.append(f + rng.normal(0, 4e-4, len(t)))
    return numpy.array(fluxes)


def test_end_to_end_at_counts_where_the_two_roots_differ():
    """survey.power_batch(statistics=True, per_transit=True) and survey.power_results against transitleastsquares(t,
    y_k).power() for 24 light curves whose planets' durations spread from 0.1 d to 0.5 d: every statistics field, every
    per-transit array and every one of the 41 keys.  At least 3 curves have, in the pick the device made, an odd or an even
    in-transit count in D (the counts at which numpy.sum(k) ** 0.5 is not float(k) ** 0.5 under the running numpy), read
    from power()'s own per_transit_count -- unless D is empty, which is printed."""
    from test_power_batch_results import assert_results_equal
    t = count_lattice.TIME
    fluxes = planted_batch()
    D = set(count_lattice.disagreeing_counts(len(t)))
    ctx = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        summary, periods, pt = survey.power_batch(t, fluxes, context=ctx, statistics=True, per_transit=True, **PLANTED_KW)
        results = survey.power_results(t, fluxes, context=ctx, **PLANTED_KW)
        device_s = time.perf_counter() - t0
        at_D = []
        for s in range(len(fluxes)):
            one = tls_amd.transitleastsquares(t, fluxes[s], verbose=False).power(
                context=ctx, verbose=False, show_progress_bar=False, **PLANTED_KW)
            rec = summary[s]
            assert not rec["no_fit"]
            expect_equal([rec["T0"], rec["period"]], [one.T0, one.period], "curve %d: T0, period" % s)
            count = numpy.asarray(one.per_transit_count)
            odd, even = int(count[1::2].sum()), int(count[0::2].sum())
            where = "curve %d (%d odd and %d even points in transit)" % (s, odd, even)
            for field, (key, i) in RESULT_OF.items():
                want = one[key] if i is None else one[key][i]
                expect_equal(rec[field], want, "%s: %s" % (where, field))
            e = int(pt["n_epochs"][s])
            assert e == len(one.transit_times) == rec["transit_count"]
            for key in PER_TRANSIT:
                expect_equal(pt[key][s, :e], one[key], "%s: %s" % (where, key))
                assert numpy.all(numpy.isnan(pt[key][s, e:])), (s, key)
            assert_results_equal(results[s], one, where)
            if odd in D or even in D:
                at_D.append((s, odd, even))
    print("\nnumpy %s, len(D) = %d; %d of %d curves have an odd or even count in D: %s; the two device calls took %.2f s"
          % (numpy.__version__, len(D), len(at_D), len(fluxes), at_D, device_s))
    if D:
        assert len(at_D) >= 3
    else:
        print("D is empty on this machine: the condition on the counts is dropped")
    ctx.close()


def test_a_missing_or_short_root_table_is_an_argument_error():
    """Either k ** 0.5 table NULL or shorter than n + 1 entries: TLS_E_ARG at the C entry with every output untouched, and a
    RuntimeError through the binding for a short one, for the injected picks and for the whole chain."""
    import ctypes
    ctx = _lib.Context(0)
    t = gapped_time()
    n = len(t)
    rng = numpy.random.RandomState(23)
    inp = prepared(ctx, t, 1 + rng.normal(0, 4e-4, n), period_min=1.5, period_max=9.0, oversampling_factor=1)
    n_p, dur = len(inp["periods"]), numpy.ascontiguousarray(inp["table"].duration)
    root = numpy.array([float(k) ** 0.5 for k in range(n + 1)])
    root_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(n + 1)])
    y, power = numpy.ascontiguousarray(inp["y"][None, :]), numpy.ones((1, n_p))
    period, T0, depth = numpy.array([4.321]), numpy.array([4.1]), numpy.array([0.999])
    row, no_fit, index = numpy.array([3]), numpy.array([0]), numpy.array([n_p // 2])
    dp, ip = _lib._dp, _lib._ip

    def call(root_p, count_p, n_root):
        stats = numpy.zeros(1, dtype=_lib.TRANSIT_STATS_DTYPE)
        stats.view(numpy.float64)[:] = -7.0
        rows, n_ep = numpy.full((1, 6, 32), -7.0), numpy.full(1, -7, dtype=numpy.int64)
        rc = ctx._lib.tls_debug_transit_stats(ctx._h, dp(y), 1, dp(period), dp(T0), ip(row), dp(depth), ip(no_fit), ip(index),
                                              dp(power), dp(dur), len(dur), calculate_fill_factor(t), root_p, count_p, n_root,
                                              32, stats.ctypes.data_as(ctypes.c_void_p), dp(rows), ip(n_ep))
        untouched = bool((stats.view(numpy.float64) == -7.0).all() and (rows == -7.0).all() and (n_ep == -7).all())
        return rc, untouched

    assert call(dp(root), dp(root_count), n + 1) == (0, False)
    for bad in ((None, dp(root_count), n + 1), (dp(root), None, n + 1), (None, None, n + 1), (dp(root), dp(root_count), n),
                (dp(root), dp(root_count), 0)):
        assert call(*bad) == (-1, True), bad                      # TLS_E_ARG
    fill = calculate_fill_factor(t)
    injected = (y, period, T0, row, depth, no_fit, index, power, dur, fill)
    with pytest.raises(RuntimeError, match="must cover"):
        ctx.debug_transit_stats(*injected, root, 32, root_count=root_count[:n])
    with pytest.raises(RuntimeError, match="must cover"):
        ctx.debug_transit_stats(*injected, root[:n], 32, root_count=root_count)
    # (the binding forms the second table itself when it is not given: stats.count_roots)
    given = ctx.debug_transit_stats(*injected, root, 32, root_count=root_count)
    formed = ctx.debug_transit_stats(*injected, root, 32)
    assert given[0].tobytes() == formed[0].tobytes()
    chain = (inp["t"], y, inp["dy"][None, :], inp["periods"], inp["table"], inp["params"], 30, fill)
    with pytest.raises(RuntimeError, match="must cover"):
        ctx.power_batch_stats(*chain, root, 32, root_count=root_count[:n])
    assert len(ctx.power_batch_stats(*chain, root, 32, root_count=root_count)[1]) == 1
    ctx.close()


def test_statistics_leave_the_summary_as_it_was():
    t = gapped_time()
    fluxes, _ = batch(t, 40, 7)
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    ctx = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain, periods = survey.power_batch(t, fluxes, context=ctx, **kw)
        rich, periods2 = survey.power_batch(t, fluxes, context=ctx, statistics=True, **kw)
        again, _ = survey.power_batch(t, fluxes, context=ctx, **kw)
    expect_equal(periods2, periods, "periods")
    for k in plain.dtype.names:
        expect_equal(rich[k], plain[k], k)
        expect_equal(again[k], plain[k], k)
    assert plain.dtype == again.dtype and "snr" not in plain.dtype.names
    ctx.close()


def test_two_contexts_equal_the_one_device_call():
    t = gapped_time()
    fluxes, dys = batch(t, 70, 13)
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = survey.power_batch(t, fluxes, dys, device=0, statistics=True, per_transit=True, **kw)
        two = survey.power_batch(t, fluxes, dys, devices=[0, 0], statistics=True, per_transit=True, **kw)
    for k in one[0].dtype.names:
        expect_equal(two[0][k], one[0][k], k)
    for k in one[2]:
        expect_equal(two[2][k], one[2][k], k)


def test_survey_of_1024_light_curves_with_statistics_has_no_stalled_group():
    from tls_amd import search as tsearch
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    fluxes = numpy.stack([synthetic.config("k2_90d", seed=s)[1] for s in range(1024)])
    ctx = tsearch.default_context(None)
    survey.power_batch(t, fluxes[:64], context=ctx, statistics=True, **kw)
    t0 = time.perf_counter()
    summary, _ = survey.power_batch(t, fluxes, context=ctx, statistics=True, **kw)
    wall = time.perf_counter() - t0
    groups = ctx.batch_group_ms()
    assert len(groups) == 32 and len(summary) == 1024
    assert wall < 3.0, (wall, groups.max(), int(groups.argmax()))
    assert groups.max() < 500.0, (groups.max(), int(groups.argmax()), float(numpy.median(groups)))
    assert numpy.all(summary["transit_count"] >= 8) and numpy.all(summary["snr"] > 5)
