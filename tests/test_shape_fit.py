"""The shape fit on the device (survey.shape_fit / tls_shape_fit; power_batch(peaks=K, peak_fits=True, shape_fit=True))
against tests/shape_fit_spec.py bit for bit, every field of the record: at the edges of the members (none, fewer than
min_count, fewer than a wave, 256 and 257, more than the LDS holds, a member exactly on the window's edge and on both
contacts, epochs on the ends of the series and in a gap), of the units (2 to 65536, around the 256 threads, exact ties) and of
the call (several candidates a curve, two slabs, two contexts, per-point dy, a NaN candidate among good ones, argument
errors), and in the pipeline with every other result untouched.

Time stamps are multiples of 1/64 d and the tables of the edge cases dyadic, so every time difference is exact.  The tables of
ingress hold 0.0 and 0.5, so the fewest units are 2 (one duration, one shift, a box and a V); 3 units are a box, a trapezoid
and a V."""
import ctypes
import warnings

import numpy
import pytest

import shape_fit_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

DT = 1 / 64.0
RATIOS, INGRESS, SHIFTS = [0.5, 1.0, 2.0], [0.0, 0.25, 0.5], [-0.25, 0.0, 0.25]      # (27 units; window >= 1.25)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def series(n, gap_at=None, gap=0):
    """n time stamps at 1/64 d, `gap` cadences missing in front of index gap_at."""
    t = 1.0 + numpy.arange(n + gap) / 64.0
    return t if gap_at is None else numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def dips(t, period, T0, T14, depth=4e-3, seed=0, sigma=1e-3, ingress=0.2):
    """Noise of `sigma` and a trapezoid of `T14` days and ingress fraction `ingress` at every T0 + e * period."""
    rng = numpy.random.RandomState(seed)
    tau = numpy.fabs((t - T0) - numpy.round((t - T0) / period) * period)
    s = numpy.clip((0.5 * T14 - tau) / (ingress * T14), 0.0, 1.0)
    return 1.0 - depth * s + (rng.normal(0, sigma, len(t)) if sigma else 0.0)


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check(ctx, t, y, dy, period, T0, duration, tables=(RATIOS, INGRESS, SHIFTS), curve=None, label="", **kw):
    """ctx.shape_fit of the candidates equals the statement in every field; what the device returned."""
    y = numpy.atleast_2d(y)
    dy = numpy.broadcast_to(numpy.asarray(dy, dtype=float), y.shape) if numpy.ndim(dy) < 2 else dy
    got = ctx.shape_fit(t, y, dy, period, T0, duration, *tables, curve=curve, **kw)
    which = numpy.arange(len(y)) if curve is None else curve
    want = spec.shape_fit_batch(t, y, dy, period, T0, duration, which, *tables, **kw)
    assert got.dtype.names == spec.FIELDS and got.shape == (len(period),)
    for i, f in enumerate(spec.FIELDS):
        expect_equal(got[f], want[:, i], (label, f))
    return got


# ---- the members ------------------------------------------------------------------------------------------------------------
def test_few_members(ctx):
    """No member at all (every epoch in a gap), fewer than min_count, fewer than a wave."""
    t = series(600, gap_at=200, gap=200)                                     # (t[200] is 400 cadences behind t[0])
    y = dips(t, 1000 * DT, t[100], 20 * DT, seed=1)
    mid = t[199] + 100 * DT                                                  # (the middle of the gap)
    got = check(ctx, t, y, 1e-3, [1000 * DT] * 4, [mid, mid, t[100], t[100]], [8 * DT, 52 * DT, DT / 2, 8 * DT], curve=[0] * 4,
                label="few")
    assert got["status"].tolist() == [2, 2, 2, 0] and got["n_points"].tolist() == [0, 9, 3, 33]
    assert got["n_in"][3] == 17 and numpy.isnan(got["ses"][:3]).all()       # (the widest box, 16 cadences, holds 17 points)
    got = check(ctx, t, y, 1e-3, [1000 * DT] * 2, [t[100]] * 2, [8 * DT] * 2, curve=[0, 0], min_count=18, label="min_count")
    assert got["status"].tolist() == [2, 2]
    got = check(ctx, t, y, 1e-3, [1000 * DT], [t[100]], [8 * DT], min_count=17, label="min_count 17")
    assert got["status"][0] == 0 and got["n_in"][0] == 17


@pytest.mark.parametrize("half_way, members", [(True, 256), (False, 257)])
def test_a_tile_of_members_and_the_exact_edges(ctx, half_way, members):
    """One epoch, d = 1 d, window 2: 256 members with T0 half-way between two stamps, 257 with T0 on one -- then two members
    lie exactly on |tau| == wd, and the unit (ratio 1, ingress 0.25, shift 0) has members exactly on u == hb = 0.25 (it counts
    with s = 1) and on u == ho = 0.5 (it does not count)."""
    t = series(600)
    T0 = t[300] + (DT / 2 if half_way else 0.0)
    y = dips(t, 16.0, T0, 1.0, seed=2, ingress=0.25)
    got = check(ctx, t, y, 1e-3, [16.0], [T0], [1.0], label=members)
    assert got["n_points"][0] == members and got["status"][0] == 0
    assert got["duration"][0] == 1.0 and got["ingress"][0] == 0.25 and got["shift"][0] == 0.0
    assert got["n_in"][0] == (64 if half_way else 63)                       # (|tau| < 0.5: the two on u == ho stay out)
    only = check(ctx, t, y, 1e-3, [16.0], [T0], [1.0], tables=([1.0], [0.0, 0.25, 0.5], [0.0]), label="one duration")
    assert only["ses_box"][0] < only["ses"][0] > only["ses_vee"][0]
    assert only["n_in"][0] == got["n_in"][0]


def test_more_members_than_the_lds_holds(ctx):
    """n = 20000, 39 epochs: the window is raised until the members cross _lib.SHAPE_LDS_MEMBERS = 2048 (tls_shape.hip.h
    kShapeLdsMembers), the members the LDS holds; beyond it they are staged from device scratch in tiles, here up to 5."""
    t = series(20000)
    P, d = 8.0, 0.25
    y = dips(t, P, t[0] + 3.0, 0.25, seed=3)
    counts = []
    for window in (1.25, 1.5625, 1.625, 4.0, 7.5):
        got = check(ctx, t, y, 1e-3, [P], [t[0] + 3.0], [d], window=window, label=window)
        counts.append(int(got["n_points"][0]))
        assert got["status"][0] == 0 and got["duration"][0] == 0.25
    assert counts == [1599, 1989, 2067, 5031, 9399], counts                 # (39 epochs of 2 floor(16 window) + 1 members)
    assert counts[1] <= _lib.SHAPE_LDS_MEMBERS < counts[2] and counts[4] > 4 * _lib.SHAPE_LDS_MEMBERS
    # three rounds of units over three tiles, and candidates in the LDS and beyond it side by side
    y2 = numpy.array([y, dips(t, P, t[0] + 5.0, 0.25, seed=4)])
    tables = (spec.DEFAULT_RATIOS, spec.DEFAULT_INGRESS, spec.DEFAULT_SHIFTS)
    got = check(ctx, t, y2, 1e-3, [P, P, P], [t[0] + 3.0, t[0] + 5.0, t[0] + 3.0], [d, 0.125, 0.0625], tables=tables,
                curve=[0, 1, 0], window=4.0, label="default tables")
    assert got["n_points"][0] > 2 * _lib.SHAPE_LDS_MEMBERS > _lib.SHAPE_LDS_MEMBERS > got["n_points"][2]


def test_epochs_on_the_ends_and_in_a_gap(ctx):
    n = 449
    t = series(n, gap_at=200, gap=64)
    P = (n + 64 - 1) * DT / 4                                                # (epochs on t[0], 128, in the gap at 256, 384, t[n-1])
    y = dips(t, P, t[0], 16 * DT, seed=5)
    got = check(ctx, t, y, 1e-3, [P, P], [t[0], t[0] - 3 * P], [16 * DT, 16 * DT], curve=[0, 0], label="ends")
    assert got["status"].tolist() == [0, 0] and got["n_points"][0] == 33 + 65 + 25 + 65 + 33      # (25 beside the gap)
    assert got[:1].tobytes() == got[1:].tobytes()                            # (T0 three periods back: the same members)


# ---- the units --------------------------------------------------------------------------------------------------------------
UNIT_TABLES = {
    2: ([1.0], [0.0, 0.5], [0.0]),
    3: ([1.0], [0.0, 0.25, 0.5], [0.0]),
    4: ([1.0, 2.0], [0.0, 0.5], [0.0]),
    255: ([0.5, 0.75, 1.0, 1.5, 2.0], [0.0, 0.25, 0.5], numpy.arange(-8, 9) / 32.0),
    256: ([0.5, 1.0, 1.5, 2.0], [0.0, 0.125, 0.25, 0.5], numpy.arange(-8, 8) / 32.0),
    257: ([1.0], numpy.linspace(0.0, 0.5, 257), [0.0]),
    2448: (spec.DEFAULT_RATIOS, spec.DEFAULT_INGRESS, spec.DEFAULT_SHIFTS),
    65536: (numpy.geomspace(0.5, 2.0, 64), numpy.linspace(0.0, 0.5, 64), numpy.linspace(-0.25, 0.25, 16)),
}


@pytest.mark.parametrize("units", sorted(UNIT_TABLES))
def test_unit_counts(ctx, units):
    """Around the 256 threads of a workgroup and the 1024 units of a round, up to the entry's limit."""
    tables = UNIT_TABLES[units]
    assert len(tables[0]) * len(tables[1]) * len(tables[2]) == units
    t = series(449)
    y = numpy.array([dips(t, 128 * DT, t[37], 12 * DT, seed=6), dips(t, 100 * DT, t[11], 9 * DT, seed=7, ingress=0.5)])
    got = check(ctx, t, y, 1e-3, [128 * DT, 100 * DT], [t[37] + DT / 4, t[11]], [12 * DT, 10 * DT], tables=tables, label=units)
    assert (got["status"] == 0).all() and (got["ses"] >= numpy.fmax(got["ses_box"], got["ses_vee"])).all()
    if units == 2:
        assert (got["ses"] == numpy.fmax(got["ses_box"], got["ses_vee"])).all()


def test_exact_ties_go_to_the_first_unit(ctx):
    """Equal entries in a table make equal units; a symmetric noise-free dip makes shifts -c and +c equal: the first in unit
    order is reported, within a thread (units 256 apart) and across threads."""
    t = series(449)
    y = dips(t, 128 * DT, t[37], 12 * DT, seed=8)
    twice = ([1.0] * 2, [0.0, 0.0, 0.25, 0.25, 0.5, 0.5], [0.0] * 64)        # 768 units, every one 64 * 2 * 2 times
    got = check(ctx, t, y, 1e-3, [128 * DT], [t[37]], [12 * DT], tables=twice, label="equal entries")
    assert got["i_duration"][0] == 0 and got["i_shift"][0] == 0 and got["i_ingress"][0] in (0, 2, 4)
    t1 = numpy.arange(-32, 33) / 64.0
    y1 = 1.0 - numpy.where(numpy.fabs(t1) <= 4 / 64.0, 1 / 64.0, 0.0)
    got = check(ctx, t1, y1, 0.5, [4.0], [0.0], [0.125], tables=([1.0, 2.0], [0.0, 0.5], [-0.25, 0.25]), label="mirror")
    assert got["status"][0] == 0 and got["i_shift"][0] == 0 and got["shift"][0] == -0.03125
    got = check(ctx, t1, y1, 0.5, [4.0], [0.0], [0.125], tables=([1.0], [0.0, 0.5], [0.0]), label="box and V alone")
    assert got["i_ingress"][0] == 0 and got["ses_box"][0] == got["ses"][0] > got["ses_vee"][0]


# ---- the call ---------------------------------------------------------------------------------------------------------------
def test_candidates_curves_and_slabs(ctx):
    """Several candidates a curve, curves out of order, per-point dy, NaN candidates among good ones, and 1025 candidates: two
    slabs of the entry."""
    n = 161
    t = series(n)
    rng = numpy.random.RandomState(11)
    P = 64 * DT
    y = numpy.array([dips(t, P, t[10 + 3 * i], 6 * DT, seed=20 + i) for i in range(5)])
    dy = rng.uniform(0.5e-3, 1.5e-3, (5, n))
    n_fits = 1025
    curve = rng.randint(0, 5, n_fits)
    period = numpy.where(rng.uniform(size=n_fits) < 0.1, P / 2, P)
    T0 = t[10 + 3 * curve] + rng.randint(-2, 3, n_fits) * DT / 4
    duration = rng.randint(3, 9, n_fits) * DT
    for bad, values in ((5, (numpy.nan, T0[5], duration[5])), (6, (P, numpy.inf, duration[6])), (700, (P, T0[700], -1.0)),
                        (1024, (0.0, T0[1024], duration[1024]))):
        period[bad], T0[bad], duration[bad] = values
    small = ([0.75, 1.5], [0.0, 0.25, 0.5], [-0.125, 0.125])
    got = check(ctx, t, y, dy, period, T0, duration, tables=small, curve=curve, label="slabs")
    # (status 1 too: 8 cadences at half the period, window * d == P / 2 exactly)
    assert (got["status"][[5, 6, 700, 1024]] == 1).all() and (got["status"] == 0).sum() > 900
    assert ((got["status"] == 1) == ((numpy.arange(n_fits) == 5) | (numpy.arange(n_fits) == 6) | (numpy.arange(n_fits) == 700)
                                     | (numpy.arange(n_fits) == 1024) | ((period == P / 2) & (duration == 8 * DT)))).all()
    assert all(numpy.isnan(got[k][[5, 6, 700, 1024]]).all() for k in spec.FIELDS[1:])
    again = ctx.shape_fit(t, y, dy, period[1000:], T0[1000:], duration[1000:], *small, curve=curve[1000:])
    assert again.tobytes() == got[1000:].tobytes()


def test_two_contexts(ctx):
    t = series(300)
    y = dips(t, 50 * DT, t[7], 8 * DT, seed=12)
    args = (t, [y], numpy.full((1, 300), 1e-3), [50 * DT, 25 * DT], [t[7], t[7]], [8 * DT, 4 * DT], RATIOS, INGRESS, SHIFTS)
    one = ctx.shape_fit(*args, curve=[0, 0])
    other = _lib.Context(0)
    try:
        two = other.shape_fit(*args, curve=[0, 0])
        back = ctx.shape_fit(*args, curve=[0, 0])
    finally:
        other.close()
    assert one.tobytes() == two.tobytes() == back.tobytes() and (one["status"] == 0).all()


def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; every TLS_E_ARG case returns before any device work with the output untouched."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = series(n)
    good = dict(t=t, y=numpy.ones((2, n)), dy=numpy.full((2, n), 1e-3), n_curves=2, period=[1.0], T0=[1.5], duration=[0.1],
                curve=[1], n_fits=1, ratio=[0.5, 1.0], ingress=[0.0, 0.5], shift=[-0.25, 0.25], window=2.0, min_count=3,
                depth_min=0.0)
    out = numpy.full(1, -7.0, dtype=_lib.SHAPE_DTYPE)

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "y", "dy", "period", "T0", "duration", "ratio", "ingress", "shift")}
        curve = _lib._i8(a["curve"])
        return lib.tls_shape_fit(ctx._h, dp(f8["t"]), dp(f8["y"]), dp(f8["dy"]), len(f8["t"]), a["n_curves"], dp(f8["period"]),
                                 dp(f8["T0"]), dp(f8["duration"]), ip(curve), a["n_fits"], dp(f8["ratio"]), len(f8["ratio"]),
                                 dp(f8["ingress"]), len(f8["ingress"]), dp(f8["shift"]), len(f8["shift"]), a["window"],
                                 a["min_count"], a["depth_min"], out.ctypes.data_as(ctypes.c_void_p))

    def untouched():
        return all((out[k] == -7.0).all() for k in out.dtype.names)

    assert call(n_fits=0) == 0 and untouched()
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - DT
    bad_t = t.copy()
    bad_t[5] = nan
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(ratio=[1.0, 0.5]), dict(ratio=[0.0, 1.0]), dict(ratio=[nan]), dict(ratio=[]),
               dict(ingress=[0.0, 0.4]), dict(ingress=[0.1, 0.5]), dict(ingress=[0.0, 0.3, 0.2, 0.5]), dict(ingress=[0.0]),
               dict(shift=[0.25, -0.25]), dict(shift=[inf]), dict(ratio=numpy.linspace(0.5, 2.0, 16385)), dict(window=0.74),
               dict(window=nan), dict(window=inf), dict(min_count=0), dict(depth_min=-1e-9), dict(depth_min=nan), dict(t=late),
               dict(t=bad_t), dict(n_fits=-1), dict(n_curves=-1)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"shape fit" in lib.tls_last_error(ctx._h), kw
    assert call() == 0 and out["status"][0] == 2 and out["n_points"][0] > 0 and not untouched()      # (constant flux)
    assert call(window=0.75) == 0                                            # (0.5 * 1.0 + 0.25: the model just fits)
    empty = ctx.shape_fit(t, numpy.ones((2, n)), numpy.ones((2, n)), [], [], [], RATIOS, INGRESS, SHIFTS, curve=[])
    assert empty.shape == (0,)


# ---- survey.shape_fit and the pipeline --------------------------------------------------------------------------------------
T = 3.0 + numpy.arange(1440) / 48.0                   # 30 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))                   # period [d], a / R_star
_FLUX = []


def flux_rows():
    """64 rows of 1440 points with two planets each, formed once."""
    if not _FLUX:
        rows = []
        for s in range(64):
            rng = numpy.random.RandomState(1000 + s)
            f = numpy.ones(len(T))
            for per, a in PLANETS:
                tp = T[0] + rng.uniform(0.1, 0.9) * per
                f += transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3], "quadratic") - 1
            rows.append(f + rng.normal(0, 4e-4, len(T)) + 2e-3 * numpy.sin(T / 1.7 + s))
        _FLUX.append(numpy.array(rows))
    return _FLUX[0]


def expected_survey(flux, period, T0, duration, curve, dy=None, **kw):
    """survey.shape_fit stated with the spec: the rows _batch_inputs hands out, the default tables."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, dy_rows = survey._batch_inputs(T, flux, dy, dict(oversampling_factor=1))
    return spec.shape_fit_batch(T, y_rows, dy_rows, period, T0, duration, curve, spec.DEFAULT_RATIOS, spec.DEFAULT_INGRESS,
                                spec.DEFAULT_SHIFTS, **kw)


def test_pipeline(ctx):
    """power_batch(peaks=4, peak_fits=True, shape_fit=True) on 64 rows of 1440 points: every other field equals the call
    without the keyword bit for bit; the shape fields equal survey.shape_fit on the returned peaks, which equals the statement
    (every eighth candidate is put to it)."""
    flux = flux_rows()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(context=ctx, peaks=4, peak_fits=True, **KW)
        summary, periods, pk = survey.power_batch(T, flux, shape_fit=True, **more)
        without = survey.power_batch(T, flux, **more)
    peaks = pk["peaks"]
    names = survey.shape_fit_fields()
    assert peaks.shape == (64, 4) and peaks.dtype.names[-len(names):] == names
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(periods, without[1], "periods")
    expect_equal(pk["n_peaks"], without[2]["n_peaks"], "n_peaks")
    assert peaks.dtype.names[:-len(names)] == without[2]["peaks"].dtype.names and set(pk) == set(without[2])
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 128
    args = (peaks["period"][curve, rank], peaks["T0"][curve, rank], peaks["duration_days"][curve, rank])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alone = survey.shape_fit(T, flux, *args, curve=curve, context=ctx)
    assert alone.dtype.names == names
    for k in names:
        expect_equal(peaks[k][curve, rank], alone[k], k)
    some = numpy.arange(0, len(curve), 8)
    want = expected_survey(flux, *(v[some] for v in args), curve[some])
    for i, f in enumerate(spec.FIELDS):
        expect_equal(alone["shape_" + f][some], want[:, i], f)
    with numpy.errstate(all="ignore"):
        expect_equal(alone["shape_delta_chi2"], alone["shape_ses"] ** 2 - alone["shape_ses_vee"] ** 2, "delta chi2")
        geometry = survey.transit_geometry(args[0], alone["shape_depth"], alone["shape_duration"], alone["shape_ingress"])
    for k, v in zip(("shape_impact", "shape_a_rs", "shape_rho_star"), geometry):
        expect_equal(alone[k], v, k)
    rest = peaks["status"] != 0
    assert (peaks["shape_status"][rest] == 1).all() and all(numpy.isnan(peaks[k][rest]).all() for k in names[1:])
    # the two injected planets are fitted, with a duration near the search's
    for per, _ in PLANETS:
        hit = (numpy.abs(peaks["period"] - per) < 0.02 * per) & (peaks["shape_status"] == 0)
        assert hit.sum() >= 48 and numpy.median(peaks["shape_duration"][hit] / peaks["duration_days"][hit]) < 2.0


def test_pipeline_combines(ctx):
    """With phase_scan, transit_times, detrend and devices=[0, 0]: the shape fields are those of survey.shape_fit on the rows
    the search saw, and every other field is that of the same call without the keyword."""
    flux = flux_rows()[:16]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(devices=[0, 0], peaks=4, peak_fits=True, phase_scan=True, transit_times=True, detrend=25, **KW)
        summary, periods, pk = survey.power_batch(T, flux, shape_fit=True, shape_fit_window=2.5, shape_fit_min_count=4, **more)
        without = survey.power_batch(T, flux, **more)
        searched = survey.detrend_batch(flux, 25, context=ctx)
    peaks = pk["peaks"]
    names = survey.shape_fit_fields()
    assert summary.tobytes() == without[0].tobytes() and peaks.dtype.names[-len(names):] == names
    assert "tt_status" in peaks.dtype.names and "scan_status" in peaks.dtype.names
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    assert pk["transit_times"].tobytes() == without[2]["transit_times"].tobytes()
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alone = survey.shape_fit(T, searched, peaks["period"][curve, rank], peaks["T0"][curve, rank],
                                 peaks["duration_days"][curve, rank], curve=curve, window=2.5, min_count=4, context=ctx)
    for k in names:
        expect_equal(peaks[k][curve, rank], alone[k], k)


def test_survey_call_options(ctx):
    """Tables, window, min_count, transit_depth_min, per-point dy, detrend and one row [n] reach the device as the statement
    has them."""
    flux = flux_rows()[:2]
    rng = numpy.random.RandomState(3)
    dy = rng.uniform(3e-4, 6e-4, flux.shape)
    period, T0, duration = [1.9, 3.1, 1.9], [3.4, 4.0, 3.9], [0.09, 0.11, 0.02]
    tables = dict(ratios=[0.5, 1.0, 1.5], ingress=[0.0, 0.2, 0.5], shifts=[-0.5, 0.0, 0.5])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.shape_fit(T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, window=3.0, min_count=5,
                               transit_depth_min=1e-4, context=ctx, **tables)
        inp, y_rows, dy_rows = survey._batch_inputs(T, flux, dy, dict(oversampling_factor=1))
        one = survey.shape_fit(T, flux[0], [1.9], [3.4], [0.09], context=ctx)
        flat = survey.shape_fit(T, flux, period[:2], T0[:2], duration[:2], detrend=25, context=ctx)
        searched = survey.detrend_batch(flux, 25, context=ctx)
    want = spec.shape_fit_batch(T, y_rows, dy_rows, period, T0, duration, [0, 1, 1], tables["ratios"], tables["ingress"],
                                tables["shifts"], 3.0, 5, 1e-4)
    for i, f in enumerate(spec.FIELDS):
        expect_equal(got["shape_" + f], want[:, i], f)
    assert one.shape == (1,) and one["shape_status"][0] in (0, 2)
    want = expected_survey(searched, period[:2], T0[:2], duration[:2], [0, 1])
    for i, f in enumerate(spec.FIELDS):
        expect_equal(flat["shape_" + f], want[:, i], ("detrend", f))
