"""Event vetting on the device (survey.event_vetting / tls_event_vetting; power_batch(peaks=K, peak_fits=True,
event_vetting=True)) against tests/event_vetting_spec.py bit for bit, every field of both records: at the edges of the statement
(tests/event_vetting_cases.py: the ends of the series, gaps and span_max hit exactly, empty chases, comparable and
non-comparable neighbours, the point share, every flag bit alone, the summary's edge counts, ties, the epoch limit, bad
ephemerides), of the kernel (more chase units than threads, fewer than a wave, per-point dy) and of the call (slabs, two
contexts, argument errors), in agreement with tls_transit_times, and in the pipeline with every other result untouched.

Time stamps are multiples of 1/64 d, so every time difference is exact."""
import ctypes
import warnings

import numpy
import pytest

import event_vetting_cases as cases
import event_vetting_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

DT = cases.DT


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def equal_records(got, want, names, label):
    for k in names:
        expect_equal(got[k], want[k], (label, k))


def device(ctx, c, which=slice(None)):
    """Context.event_vetting on a case (on the candidates `which`)."""
    return ctx.event_vetting(c["t"], c["y"], c["dy"], c["period"][which], c["T0"][which], c["row"][which], c["reach"][which],
                             c["chase_reach"][which], c["guard"][which], c["chase_span"][which], c["widths"],
                             cases.shapes_of(c["widths"]), c["span_max"], curve=c["curve"][which], **c["options"])


def check(ctx, c):
    """The device equals the statement on a case: every field of both records; what the device returned."""
    got, want = device(ctx, c), cases.expected(c)
    assert got[0].dtype.names == spec.SUMMARY_FIELDS and got[1].dtype.names == spec.EVENT_FIELDS
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape == (len(c["period"]), c["options"]["max_epochs"])
    equal_records(got[0], want[0], spec.SUMMARY_FIELDS, c["label"])
    equal_records(got[1], want[1], spec.EVENT_FIELDS, c["label"])
    return got


_EDGES = cases.edge_cases()


@pytest.mark.parametrize("c", _EDGES, ids=[str(c["label"]) for c in _EDGES])
def test_every_edge(ctx, c):
    """The ends of the series, gaps, empty chases, neighbours, the point share, the flags, the summary's edge counts, ties,
    the unit counts against the workgroup's threads with per-point dy, the epoch limit and bad ephemerides: the device equals
    the statement, and the case shows on the device's result what it is there to show."""
    c["check"](*check(ctx, c))


def test_candidates_curves_and_slabs(ctx):
    """Several candidates a curve, curves out of order, 1030 candidates (more than the slab of 1024) against the call on the
    last 6 alone, and max_epochs at the entry's limit (3 candidates are enough to see the records past n_epochs filled)."""
    c = cases.many_candidates()
    out, events = check(ctx, c)
    assert (out["status"] == 0).all() and (out["n_held"] >= 2).sum() > 900
    again = device(ctx, c, slice(1024, None))
    assert again[0].tobytes() == out[1024:].tobytes() and again[1].tobytes() == events[1024:].tobytes()
    few = dict(c, options=dict(c["options"], max_epochs=65536))
    which = numpy.array([7, 0, 1029])
    got = device(ctx, few, which)
    want = cases.expected(few, which=which)
    equal_records(got[0], want[0], spec.SUMMARY_FIELDS, "65536")
    equal_records(got[1], want[1], spec.EVENT_FIELDS, "65536")
    assert numpy.isnan(got[1]["epoch"][:, 9:]).all()


def test_two_contexts(ctx):
    c = _EDGES[0]
    one = device(ctx, c)
    other = _lib.Context(0)
    try:
        two = device(other, c)
        back = device(ctx, c)
    finally:
        other.close()
    assert one[0].tobytes() == two[0].tobytes() == back[0].tobytes() and one[1].tobytes() == two[1].tobytes() == back[1].tobytes()
    assert (one[0]["n_held"] == 5).all()


def test_agreement_with_transit_times(ctx):
    """ses, depth, index and the event status 1 are tls_transit_times' fields of the same candidates, byte for byte."""
    for c in [c for c in _EDGES if c["label"] in ("gap, epochs in it", "units", "limit 13")] + [cases.many_candidates()]:
        out, events = device(ctx, c)
        eph, times = ctx.transit_times(c["t"], c["y"], c["dy"], c["period"], c["T0"], c["row"], c["reach"], c["widths"],
                                       cases.shapes_of(c["widths"]), c["span_max"], curve=c["curve"],
                                       **{k: v for k, v in c["options"].items() if k in ("depth_min", "min_ses", "max_epochs")})
        for k in ("ses", "depth", "index", "epoch", "time_linear"):
            assert events[k].tobytes() == times[k].tobytes(), (c["label"], k)
        assert numpy.array_equal(events["status"] == 1, times["status"] == 1), c["label"]
        assert out["n_epochs"].tobytes() == eph["n_epochs"].tobytes() and out["epoch_first"].tobytes() == eph["epoch_first"].tobytes()
        assert numpy.array_equal(out["status"], eph["status"])


def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; every TLS_E_ARG case returns before any device work with the outputs untouched."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = cases.series(n)
    good = dict(t=t, y=numpy.ones((2, n)), dy=numpy.full((2, n), 1e-3), n_curves=2, curve=[1], period=[1.0], T0=[1.5], row=[1],
                reach=[2], chase_reach=[10], guard=[3], chase_span=[0.1], n_fits=1, shape_values=numpy.ones(8),
                shape_offset=[0, 3], width=[3, 5], span_max=[0.1, 0.2], n_rows=2, depth_min=0.0, min_ses=3.0, chase_fraction=0.6,
                chase_min=0.5, point_fraction=0.5, step_fraction=0.5, max_epochs=4)
    out = numpy.full(1, -7.0, dtype=_lib.EVENT_SUMMARY_DTYPE)
    events = numpy.full((1, 4), -7.0, dtype=_lib.EVENT_RECORD_DTYPE)

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "y", "dy", "period", "T0", "chase_span", "shape_values", "span_max")}
        i8 = {k: _lib._i8(a[k]) for k in ("curve", "row", "reach", "chase_reach", "guard", "shape_offset", "width")}
        return lib.tls_event_vetting(ctx._h, dp(f8["t"]), dp(f8["y"]), dp(f8["dy"]), len(f8["t"]), a["n_curves"], ip(i8["curve"]),
                                     dp(f8["period"]), dp(f8["T0"]), ip(i8["row"]), ip(i8["reach"]), ip(i8["chase_reach"]),
                                     ip(i8["guard"]), dp(f8["chase_span"]), a["n_fits"], dp(f8["shape_values"]),
                                     ip(i8["shape_offset"]), ip(i8["width"]), dp(f8["span_max"]), a["n_rows"], a["depth_min"],
                                     a["min_ses"], a["chase_fraction"], a["chase_min"], a["point_fraction"], a["step_fraction"],
                                     a["max_epochs"], out.ctypes.data_as(ctypes.c_void_p), events.ctypes.data_as(ctypes.c_void_p))

    def untouched():
        return all((out[k] == -7.0).all() for k in out.dtype.names) and all((events[k] == -7.0).all() for k in events.dtype.names)

    assert call(n_fits=0) == 0 and untouched()
    assert lib.tls_event_vetting(ctx._h, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0, None, None,
                                 None, None, 0, 0.0, 3.0, 0.6, 0.5, 0.5, 0.5, 1, None, None) == 0
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - DT
    bad_t = t.copy()
    bad_t[5] = nan
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(row=[2]), dict(row=[-1]), dict(reach=[0]), dict(reach=[4097]),
               dict(max_epochs=0), dict(max_epochs=65537), dict(width=[2, 5]), dict(width=[3, 4097]), dict(width=[5, 3]),
               dict(width=[3, 3]), dict(shape_offset=[0, -1]), dict(n_rows=0), dict(span_max=[0.1, inf]), dict(span_max=[-0.1, 0.2]),
               dict(span_max=[nan, 0.2]), dict(t=late), dict(t=bad_t), dict(min_ses=nan), dict(depth_min=-1e-9), dict(depth_min=inf),
               dict(depth_min=nan), dict(n_fits=-1), dict(n_curves=-1),
               dict(chase_reach=[-1]), dict(chase_reach=[8193]), dict(guard=[-1]), dict(chase_span=[0.0]), dict(chase_span=[-0.1]),
               dict(chase_span=[nan]), dict(chase_span=[inf]), dict(chase_fraction=0.0), dict(chase_fraction=1.0001),
               dict(chase_fraction=nan), dict(chase_min=-1e-9), dict(chase_min=1.0001), dict(chase_min=nan),
               dict(point_fraction=0.0), dict(point_fraction=-1.0), dict(point_fraction=nan), dict(step_fraction=0.0),
               dict(step_fraction=-1.0), dict(step_fraction=nan)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"event vetting" in lib.tls_last_error(ctx._h), kw
    assert call(chase_reach=[8192], guard=[2 ** 40], chase_fraction=1.0, chase_min=0.0, point_fraction=inf) == 0
    assert out["status"][0] == 0 and out["n_epochs"][0] == 4 and not untouched()
    empty = ctx.event_vetting(t, numpy.ones((2, n)), numpy.ones((2, n)), [], [], [], [], [], [], [], [3], [numpy.ones(3)], [0.1],
                              curve=[])
    assert empty[0].shape == (0,) and empty[1].shape == (0, 1)


# ---- survey.event_vetting and the pipeline ----------------------------------------------------------------------------------
T = 3.0 + numpy.arange(600) / 48.0                    # 12.5 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))                   # period [d], a / R_star


def curve_of(s):
    rng = numpy.random.RandomState(1000 + s)
    f = numpy.ones(len(T))
    for per, a in PLANETS:
        tp = T[0] + rng.uniform(0.1, 0.9) * per
        f += transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3], "quadratic") - 1
    return f + rng.normal(0, 4e-4, len(T)) + 2e-3 * numpy.sin(T / 1.7 + s)


def expected_survey(flux, period, T0, duration, curve, max_epochs, dy=None, rows=(), **options):
    """survey.event_vetting stated with the spec: the rows _batch_inputs hands out, the table of event_vetting_rows."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, dy_rows = survey._batch_inputs(T, flux, dy, dict(oversampling_factor=1))
    widths, span_max, row, reach, chase_reach, guard, chase_span = survey.event_vetting_rows(T, period, duration, *rows)
    shapes = spec.shapes_of(widths, **inp["shape"])
    return spec.expected(T, y_rows, dy_rows, curve, period, T0, row, reach, chase_reach, guard, chase_span, shapes, span_max,
                         max_epochs=max_epochs, **options)


@pytest.mark.parametrize("detrend", [None, 25])
def test_pipeline(ctx, detrend):
    """power_batch(peaks=3, peak_fits=True, event_vetting=True) on 4 curves: the ev_ fields and the events equal
    survey.event_vetting on the fits' (period, T0, duration_days), which equals the statement; summary, periods, n_peaks and
    every other field of the peaks equal the call without the keyword byte for byte."""
    flux = numpy.array([curve_of(s) for s in range(4)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(context=ctx, peaks=3, peak_fits=True, phase_scan=True, transit_times=True, detrend=detrend, **KW)
        summary, periods, pk = survey.power_batch(T, flux, event_vetting=True, **more)
        without = survey.power_batch(T, flux, **more)
        searched = flux if detrend is None else survey.detrend_batch(flux, detrend, context=ctx)
    peaks, events = pk["peaks"], pk["events"]
    max_epochs = survey._max_epochs(T, periods)
    assert events.shape == (4, 3, max_epochs) and events.dtype.names == survey.event_fields()
    names = ["ev_" + k for k in survey.event_summary_fields()]
    assert list(peaks.dtype.names[-len(names):]) == names
    # everything else of the call is untouched
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(periods, without[1], "periods")
    expect_equal(pk["n_peaks"], without[2]["n_peaks"], "n_peaks")
    assert peaks.dtype.names[:-len(names)] == without[2]["peaks"].dtype.names and "events" not in without[2]
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    assert pk["transit_times"].tobytes() == without[2]["transit_times"].tobytes()
    # the fitted peaks, against survey.event_vetting and against the statement
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 8
    args = (peaks["period"][curve, rank], peaks["T0"][curve, rank], peaks["duration_days"][curve, rank])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, alone = survey.event_vetting(T, searched, *args, curve=curve, max_epochs=max_epochs, context=ctx)
        auto = survey.event_vetting(T, searched, *args, curve=curve, context=ctx)
    assert out.dtype.names == survey.event_summary_fields() and alone.dtype.names == survey.event_fields()
    for k in survey.event_summary_fields():
        expect_equal(peaks["ev_" + k][curve, rank], out[k], k)
    equal_records(events[curve, rank], alone, survey.event_fields(), "rows")
    want = expected_survey(searched, *args, curve, max_epochs)
    equal_records(out, want[0], spec.SUMMARY_FIELDS, "summary")
    equal_records(alone, want[1], spec.EVENT_FIELDS, "events")
    # the events agree with the transit times of the same call
    for k in ("ses", "depth", "index"):
        assert events[k].tobytes() == pk["transit_times"][k].tobytes(), k
    # max_epochs=None: the largest epoch count among the candidates
    assert auto[1].shape[1] == int(out["n_epochs"].max()) <= max_epochs
    equal_records(auto[1], alone[:, :auto[1].shape[1]], survey.event_fields(), "auto")
    # peaks without a fit: status 1 and NaN
    rest = peaks["status"] != 0
    assert (peaks["ev_status"][rest] == 1).all() and numpy.isnan(peaks["ev_mes"][rest]).all()
    assert numpy.isnan(peaks["ev_n_held"][rest]).all() and numpy.isnan(events["epoch"][rest]).all()
    # the two injected planets are held at most of their epochs
    found = sum(int((numpy.abs(peaks["period"] - per) < 0.02 * per)[peaks["ev_n_held"] >= 3].sum()) for per, _ in PLANETS)
    assert found >= 6


def test_survey_call_options(ctx):
    """search, chase_window, guard, the four parameters, min_ses, per-point dy and one row [n] reach the device as the
    statement has them."""
    flux = numpy.array([curve_of(s) for s in range(2)])
    rng = numpy.random.RandomState(3)
    dy = rng.uniform(3e-4, 6e-4, flux.shape)
    period, T0, duration = [1.9, 3.1, 1.9], [3.4, 4.0, 3.9], [0.09, 0.11, 0.02]
    options = dict(min_ses=5.0, chase_fraction=0.4, chase_min=0.7, point_fraction=0.3, step_fraction=0.2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, events = survey.event_vetting(T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, search=2.0,
                                           chase_window=0.25, guard=1.0, context=ctx, **options)
        one = survey.event_vetting(T, flux[0], [1.9], [3.4], [0.09], search=2.0, max_epochs=events.shape[1], context=ctx)
    rows = survey.event_vetting_rows(T, period, duration, 2.0, 0.25, 1.0)
    assert rows[0].tolist() == [3, 4, 5] and rows[3].tolist() == [8, 10, 6]
    assert rows[4].tolist() == [22, 37, 22] and rows[5].tolist() == [4, 5, 3]
    want = expected_survey(flux, period, T0, duration, [0, 1, 1], events.shape[1], dy=dy, rows=(2.0, 0.25, 1.0), **options)
    equal_records(out, want[0], spec.SUMMARY_FIELDS, "options")
    equal_records(events, want[1], spec.EVENT_FIELDS, "options")
    assert one[0].shape == (1,) and one[1].shape == (1, events.shape[1]) and one[0]["n_epochs"][0] == out["n_epochs"][0]
