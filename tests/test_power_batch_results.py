"""Survey-mode results objects on the device (survey.power_results, tls_power_batch_models, tls_debug_transit_models): every
one of power()'s 41 keys equal to what power() returns for the same light curve, and the model stage equal to the host
sequence of api.py:175-203 on injected picks that reach its edge branches."""
import warnings

import numpy
import pytest

import tls_amd
from tls_amd import _lib, survey, synthetic, transit_model
from tls_amd.helpers import fold
from tls_amd.results import RESULT_KEYS
from tls_amd.stats import all_transit_times, calculate_fill_factor, calculate_stretch, model_lightcurve
from tls_amd.template import fractional_transit

pytestmark = pytest.mark.gpu



def gapped_time():
    t = numpy.linspace(3.0, 33.0, 720)
    return t[(t < 14.0) | (t > 18.5)]   # a data gap: some epochs hold no point


def batch(t, n_curves, seed):
    """Transits of random period, depth and epoch in white noise, per-point dy; curve 5 is flat (no fit)."""
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


def assert_results_equal(got, want, what):
    assert tuple(got.keys()) == tuple(want.keys()) == RESULT_KEYS, what
    for key in want:
        g, w = got[key], want[key]
        if isinstance(w, tuple):
            assert isinstance(g, tuple) and len(g) == len(w), (what, key)
        if w is None:
            assert g is None, (what, key)
            continue
        numpy.testing.assert_array_equal(numpy.asarray(g, dtype=float), numpy.asarray(w, dtype=float),
                                         err_msg="%s: %s" % (what, key))


def power_of(t, y, dy, ctx, kw):
    return tls_amd.transitleastsquares(t, y, dy, verbose=False).power(context=ctx, verbose=False, show_progress_bar=False, **kw)


@pytest.mark.parametrize("weights", [False, True])
def test_results_equal_power_per_curve(weights):
    """70 light curves in three launch groups: the results object of 12 curves spread over the groups (a no-fit one among
    them) equals power()'s, all 41 keys in key order."""
    ctx = _lib.Context(0)
    t = gapped_time()
    fluxes, dys = batch(t, 70, 11)
    dy_batch = dys if weights else None
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_results(t, fluxes, dy_batch, context=ctx, **kw)
        assert len(got) == 70 and numpy.isnan(got[5].period)
        for s in (0, 1, 5, 17, 31, 32, 33, 47, 63, 64, 65, 69):
            want = power_of(t, fluxes[s], None if dy_batch is None else dy_batch[s], ctx, kw)
            assert_results_equal(got[s], want, "curve %d" % s)
    ctx.close()


def test_long_series_take_the_hbm_sort():
    """Series too long for the LDS (the fold's sort in HBM scratch, long model rows): power() key for key."""
    ctx = _lib.Context(0)
    t = numpy.linspace(2.0, 42.0, 32000)
    rng = numpy.random.RandomState(4)
    fluxes = numpy.array([transit_model.light_curve(t, 2.5 + 0.3 * s, 3.1 + 0.05 * s, 0.05, 10, 89.9, 0, 90, [0.4, 0.3],
                                                    "quadratic") + rng.normal(0, 3e-4, len(t)) for s in range(3)])
    kw = dict(period_min=3.0, period_max=3.3, oversampling_factor=1, T0_fit_margin=0.05)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_results(t, fluxes, context=ctx, **kw)
        for s in range(3):
            assert_results_equal(got[s], power_of(t, fluxes[s], None, ctx, kw), "curve %d" % s)
            assert len(got[s].model_lightcurve_time) > 5 * len(t) // 2
    ctx.close()


def host_models(inp, y, dy, period, T0, duration, depth):
    """api.py:175-203 on the host: the folded light curve in the stable order, model_folded_model, model_lightcurve."""
    t, n = inp["t"], len(inp["t"])
    shape = inp["shape"]
    maxw = int(numpy.max(inp["durations"]) * n)
    transit_times = all_transit_times(T0, t, period)
    phases = fold(t, period, T0=T0 + period / 2)
    order = numpy.argsort(phases, kind="stable")
    fill_half = 1 - ((1 - calculate_fill_factor(t)) * 0.5)
    stretch = calculate_stretch(t, period, transit_times)
    folded_model = fractional_transit(duration=duration * maxw * fill_half, maxwidth=maxw / stretch, depth=1 - depth,
                                      samples=n, **shape)
    single = fractional_transit(duration=duration * maxw, maxwidth=maxw / stretch, depth=1 - depth,
                                samples=int(len(y) / len(transit_times)) * 5, **shape)
    lc_model, lc_time = model_lightcurve(transit_times, period, t, single)
    return phases[order], y[order], dy[order], order, folded_model, lc_time, lc_model


def run_injected(ctx, inp, y, period, T0, durations, depth, lc_cap=None):
    n_c, n = len(period), len(inp["t"])
    rng = numpy.random.RandomState(2)
    power = rng.uniform(0, 1, (n_c, len(inp["periods"])))
    max_epochs = 4 * n
    root = numpy.array([float(k) ** 0.5 for k in range(n + 1)])
    root_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(n + 1)])
    row_duration = inp["table"].duration.copy()   # (one per template row; curve c takes row c)
    assert len(row_duration) >= n_c
    row_duration[:n_c] = durations
    cap = lc_cap or 15 * n + 10
    return ctx.debug_transit_models(y, period, T0, numpy.arange(n_c), depth, 0, 0, power, row_duration,
                                    calculate_fill_factor(inp["t"]), root, max_epochs, survey._model_template(inp), cap,
                                    root_count=root_count)


def test_model_stage_edges_equal_the_host_sequence():
    """Injected picks through the model stage: occupied 0 and 1, a single epoch, T0 before min(t), a crop that leaves an
    empty model light curve, many epochs (few model samples) and the ordinary case, against api.py:175-203."""
    ctx = _lib.Context(0)
    t, f = synthetic.light_curve(30.0, 24, 2e-4, per=4.321, rp=0.05, a=12)
    inp = synthetic.search_inputs(t, f, period_min=3.5, period_max=5.5, oversampling_factor=2)
    depth = 0.9993
    t, n = inp["t"], len(inp["t"])
    ctx.prepare(t, inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    span, t0 = float(t[-1] - t[0]), float(t[0])
    maxw = int(numpy.max(inp["durations"]) * n)
    fill_half = 1 - ((1 - calculate_fill_factor(t)) * 0.5)
    cases = []   # (period, T0, duration, what)
    # occupied = int((duration * maxw * fill_half / (maxw / stretch)) * n): pick durations that give 0 and 1
    P = 4.3
    E = len(all_transit_times(t0 + 1.0, t, P))
    stretch = calculate_stretch(t, P, [0.0] * E)
    for occ in (0, 1):
        d = (occ + 0.5) / (fill_half * stretch * n)
        assert int((d * maxw * fill_half / (maxw / stretch)) * n) == occ
        cases.append((P, t0 + 1.0, d, "occupied %d" % occ))
    cases += [(P, t0 + 1.0, 0.04, "ordinary"), (span, t0 + 0.5, 0.03, "single epoch"), (P, t0 - 1.3, 0.04, "T0 before min(t)"),
              (P, t0 + span + 3 * P, 0.04, "empty crop"), (0.11, t0 + 0.02, 0.01, "many epochs")]
    period = numpy.array([c[0] for c in cases])
    T0 = numpy.array([c[1] for c in cases])
    durations = [c[2] for c in cases]
    y = numpy.stack([inp["y"]] * len(cases))
    with warnings.catch_warnings(), numpy.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        stats, rows, n_epochs, folded, model, lc, lc_len = run_injected(ctx, inp, y, period, T0, durations, depth)
        for c, (P, T, d, what) in enumerate(cases):
            ph, fy, fdy, order, fm, lt, lm = host_models(inp, inp["y"], inp["dy"], P, T, d, depth)
            numpy.testing.assert_array_equal(folded[c, 0], ph, what)
            numpy.testing.assert_array_equal(folded[c, 1], fy, what)
            numpy.testing.assert_array_equal(folded[c, 2], order, what)
            numpy.testing.assert_array_equal(model[c], fm, what)
            assert lc_len[c] == len(lt), what
            numpy.testing.assert_array_equal(lc[c, 0, :lc_len[c]], lt, what)
            numpy.testing.assert_array_equal(lc[c, 1, :lc_len[c]], lm, what)
            assert numpy.all(numpy.isnan(lc[c, :, lc_len[c]:])), what
        assert lc_len[cases.index(next(c for c in cases if c[3] == "empty crop"))] == 0
        assert n_epochs[cases.index(next(c for c in cases if c[3] == "single epoch"))] == 1
        assert int(n / n_epochs[-1]) * 5 <= 10   # many epochs: few model samples
        # more epochs than points: no model samples, power() raises there -- so does the device stage
        with pytest.raises(RuntimeError, match="power\\(\\) raises"):
            run_injected(ctx, inp, y[:1], numpy.array([span / (1.5 * n)]), T0[:1], [0.001], depth)
        with pytest.raises(ValueError):
            host_models(inp, inp["y"], inp["dy"], span / (1.5 * n), T0[0], 0.001, depth)
        # a row shorter than the model light curve is an error, not a cut
        with pytest.raises(RuntimeError, match="lc_cap"):
            run_injected(ctx, inp, y[2:3], period[2:3], T0[2:3], durations[2:3], depth, lc_cap=10)
    ctx.close()


def test_tied_phases_take_the_stable_order():
    """Duplicate time stamps: equal phases come out by index, numpy.argsort(kind="stable")."""
    ctx = _lib.Context(0)
    t, f = synthetic.light_curve(30.0, 12, 2e-4, per=4.321, rp=0.05, a=12)
    t = numpy.repeat(t, 2)
    f = numpy.repeat(f, 2) + numpy.tile([0.0, 1e-5], len(f))
    inp = synthetic.search_inputs(t, f, period_min=3.5, period_max=5.5, oversampling_factor=2)
    ctx.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    with warnings.catch_warnings(), numpy.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        out = run_injected(ctx, inp, inp["y"][None, :], numpy.array([4.3]), numpy.array([inp["t"][0] + 1.0]), [0.04], 0.9993)
        folded = out[3]
        ph, fy, fdy, order, fm, lt, lm = host_models(inp, inp["y"], inp["dy"], 4.3, inp["t"][0] + 1.0, 0.04, 0.9993)
    assert numpy.any(numpy.diff(ph) == 0)   # there are ties
    numpy.testing.assert_array_equal(folded[0, 2], order)
    numpy.testing.assert_array_equal(folded[0, 1], fy)
    numpy.testing.assert_array_equal(folded[0, 0], ph)
    ctx.close()


def test_two_devices_and_existing_outputs_unchanged():
    """devices=[0, 0] gives bit for bit what one device gives; models=True leaves the summary, statistics and per-transit
    output of a statistics=True, per_transit=True call as they were."""
    t = gapped_time()
    fluxes, dys = batch(t, 40, 5)
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ctx = _lib.Context(0)
        base, periods, pt = survey.power_batch(t, fluxes, dys, context=ctx, statistics=True, per_transit=True, **kw)
        one = survey.power_batch(t, fluxes, dys, context=ctx, models=True, **kw)
        ctx.close()
        two = survey.power_batch(t, fluxes, dys, devices=[0, 0], models=True, **kw)
    assert base.dtype == one[0].dtype
    for k in base.dtype.names:
        numpy.testing.assert_array_equal(one[0][k], base[k], k)
        numpy.testing.assert_array_equal(two[0][k], base[k], k)
    for k in pt:
        numpy.testing.assert_array_equal(one[2][k], pt[k], k)
    for k in one[3]:
        numpy.testing.assert_array_equal(two[3][k], one[3][k], k)
    assert set(one[3]) == {"folded_phase", "folded_y", "folded_dy", "model_folded_model", "model_lightcurve_time",
                           "model_lightcurve_model", "lc_len", "model_folded_phase"}
