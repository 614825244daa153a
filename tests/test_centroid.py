"""The centroid-shift test on the device (survey.centroid_test / tls_centroid_test; power_batch(peaks=K, peak_fits=True,
centroids=(cx, cy))) against tests/centroid_spec.py bit for bit, every field, NaN positions included: at the edges of the
statement (tests/centroid_cases.py: every status 1 cause, both kinds of status 2, one used epoch, epochs cut by the ends of the
series, inside a gap, short of min_out, NaN centroids in transit and over an epoch, tau at +-wd, v at 0 and 1, constant
centroids), of the kernel (series of 1, 7, 255, 257 and 1500 points; more used epochs than the 256 threads of a workgroup and
than the 256 epochs its LDS holds; Julian dates) and of the call (unsorted and repeated curves, a candidate above a slab,
n_fits = 0, argument errors), and in the pipeline with every other result untouched."""
import ctypes
import warnings

import numpy
import pytest

import centroid_cases as cases
import centroid_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def device(ctx, c, which=slice(None)):
    """Context.centroid_test on a case (on the candidates `which`)."""
    return ctx.centroid_test(c["t"], c["y"], c["cx"], c["cy"], c["period"][which], c["T0"][which], c["duration"][which], c["b"],
                             curve=c["curve"][which], **c["options"])


def check(ctx, c):
    """The device equals the statement on a case, every field; what the device returned."""
    got, want = device(ctx, c), cases.expected(c)
    assert got.dtype.names == spec.FIELDS and got.shape == want.shape == (len(c["period"]),)
    for k in spec.FIELDS:
        expect_equal(got[k], want[k], (c["label"], k))
    return got


_EDGES = cases.edge_cases()


@pytest.mark.parametrize("c", _EDGES, ids=[str(c["label"]) for c in _EDGES])
def test_every_edge(ctx, c):
    """The device equals the statement, and the case shows on the device's result what it is there to show."""
    assert len(c["t"]) in (1, 7, 255, 257, 1500) or c["label"] == "gaps and holes"
    c["check"](check(ctx, c))


def test_many_epochs_reach_the_scratch(ctx):
    """The case of 300 epochs has more used epochs than a workgroup has threads and than its LDS holds."""
    c = cases.many_epochs()
    got = device(ctx, c)
    assert got["n_epochs"][0] > max(_lib.CENTROID_THREADS, _lib.CENTROID_LDS_EPOCHS)
    assert c["options"]["max_epochs"] == _lib.CENTROID_MAX_EPOCHS


def test_candidates_over_a_slab(ctx):
    """1025 candidates, one above the slab of 1024, against the statement and against the call on the last two alone."""
    c = cases.over_a_slab()
    got = check(ctx, c)
    c["check"](got)
    again = device(ctx, c, slice(1023, None))
    assert again.tobytes() == got[1023:].tobytes()


def test_two_contexts(ctx):
    c = cases.julian_dates()
    one = device(ctx, c)
    other = _lib.Context(0)
    try:
        two = device(other, c)
        back = device(ctx, c)
    finally:
        other.close()
    assert one.tobytes() == two.tobytes() == back.tobytes() and (one["status"] == 0).all()


def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; every TLS_E_ARG case returns before any device work with the output untouched."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = cases.series(n)
    y, cx, cy = cases.curves(t, 2, 0, 0.01, T0=0.5)
    good = dict(t=t, y=y, cx=cx, cy=cy, n_curves=2, period=[1.0], T0=[0.5], duration=[0.125], curve=[1], n_fits=1,
                shape=cases.shape_of(9), L=9, window=3.0, min_in=1, min_out=3, max_epochs=16)
    out = numpy.full(1, -7.0, dtype=_lib.CENTROID_DTYPE)

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "y", "cx", "cy", "period", "T0", "duration", "shape")}
        return lib.tls_centroid_test(ctx._h, dp(f8["t"]), dp(f8["y"]), dp(f8["cx"]), dp(f8["cy"]), len(f8["t"]), a["n_curves"],
                                     dp(f8["period"]), dp(f8["T0"]), dp(f8["duration"]), ip(_lib._i8(a["curve"])), a["n_fits"],
                                     dp(f8["shape"]), a["L"], a["window"], a["min_in"], a["min_out"], a["max_epochs"],
                                     out.ctypes.data_as(ctypes.c_void_p))

    def untouched():
        return all((out[k] == -7.0).all() for k in out.dtype.names)

    assert call(n_fits=0) == 0 and untouched()
    assert lib.tls_centroid_test(ctx._h, None, None, None, None, 0, 0, None, None, None, None, 0, dp(_lib._f8(good["shape"])), 9,
                                 3.0, 1, 3, 1, None) == 0
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - cases.DT
    bad_t = t.copy()
    bad_t[5] = nan
    bad_shape = cases.shape_of(9)
    bad_shape[4] = nan
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(max_epochs=0), dict(max_epochs=65537), dict(window=0.999), dict(window=nan),
               dict(window=inf), dict(min_in=0), dict(min_out=0), dict(min_in=-3), dict(L=1), dict(L=0), dict(L=(1 << 20) + 1),
               dict(shape=bad_shape), dict(t=late), dict(t=bad_t), dict(n_fits=-1), dict(n_curves=-1)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"centroid test" in lib.tls_last_error(ctx._h), kw
    assert call(window=1.0, min_in=2 ** 40, max_epochs=65536) == 0
    assert out["status"][0] == 2 and out["n_skipped"][0] == 8 and not untouched()
    assert call() == 0 and out["status"][0] == 0 and out["n_epochs"][0] == 8
    empty = ctx.centroid_test(t, y, cx, cy, [], [], [], cases.shape_of(9), curve=[])
    assert empty.shape == (0,)


# ---- survey.centroid_test and the pipeline ----------------------------------------------------------------------------------
T = 3.0 + numpy.arange(600) / 48.0                    # 12.5 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))                   # period [d], a / R_star
N_CURVES = 8


def curve_of(s):
    """(flux, cx, cy) of curve s: two planets; the dip of the first also moves the photocentre of the odd curves."""
    rng = numpy.random.RandomState(1000 + s)
    f, dip = numpy.ones(len(T)), []
    for per, a in PLANETS:
        tp = T[0] + rng.uniform(0.1, 0.9) * per
        dip.append(1 - transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3], "quadratic"))
        f -= dip[-1]
    f = f + rng.normal(0, 4e-4, len(T)) + 2e-3 * numpy.sin(T / 1.7 + s)
    drift = 0.01 * numpy.sin(T / 0.9 + s)
    cx = 10.0 + drift + (s % 2) * 3.0 * dip[0] + rng.normal(0, 1e-3, len(T))
    cy = 20.0 - drift - (s % 2) * 2.0 * dip[0] + rng.normal(0, 1e-3, len(T))
    if s == 2:
        cx[100:110], cy[300] = numpy.nan, numpy.inf
    return f, cx, cy


@pytest.fixture(scope="module")
def batch():
    rows = [curve_of(s) for s in range(N_CURVES)]
    return tuple(numpy.array([r[i] for r in rows]) for i in range(3))


def expected_survey(flux, cx, cy, period, T0, duration, curve, **options):
    """survey.centroid_test stated with the spec: the rows _batch_inputs hands out, the search's template as a dip."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, _ = survey._batch_inputs(T, flux, None, dict(oversampling_factor=1))
    b = survey._centroid_shape(inp)
    raw = spec.centroid_batch(T, y_rows, cx, cy, period, T0, duration, curve, b, **options)
    return {k: raw[:, i] for i, k in enumerate(spec.FIELDS)}


@pytest.mark.parametrize("detrend", [None, 25])
def test_pipeline(ctx, batch, detrend):
    """power_batch(peaks=4, peak_fits=True, centroids=(cx, cy)) on 8 curves: the cen_ fields equal survey.centroid_test on the
    fits' (period, T0, duration_days) byte for byte, which equals the statement; an unfitted peak gives status 1; summary,
    periods, n_peaks and every other field of the peaks equal the call without the keyword byte for byte."""
    flux, cx, cy = batch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(context=ctx, peaks=4, peak_fits=True, phase_scan=True, shape_fit=True, detrend=detrend, **KW)
        summary, periods, pk = survey.power_batch(T, flux, centroids=(cx, cy), **more)
        without = survey.power_batch(T, flux, **more)
        searched = flux if detrend is None else survey.detrend_batch(flux, detrend, context=ctx)
    peaks = pk["peaks"]
    names = list(survey.centroid_fields())
    assert peaks.shape == (N_CURVES, 4) and list(peaks.dtype.names[-len(names):]) == names
    # everything else of the call is untouched
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(periods, without[1], "periods")
    expect_equal(pk["n_peaks"], without[2]["n_peaks"], "n_peaks")
    assert peaks.dtype.names[:-len(names)] == without[2]["peaks"].dtype.names and set(pk) == set(without[2])
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    # the fitted peaks, against survey.centroid_test byte for byte and against the statement
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 16
    args = (peaks["period"][curve, rank], peaks["T0"][curve, rank], peaks["duration_days"][curve, rank])
    max_epochs = min(survey._max_epochs(T, periods), _lib.CENTROID_MAX_EPOCHS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alone = survey.centroid_test(T, searched, cx, cy, *args, curve=curve, max_epochs=max_epochs, context=ctx)
        auto = survey.centroid_test(T, searched, cx, cy, *args, curve=curve, context=ctx)
    assert alone.dtype.names == survey.centroid_fields() and alone.tobytes() == auto.tobytes()
    for k in names:
        assert peaks[k][curve, rank].tobytes() == alone[k].tobytes(), k
    want = expected_survey(searched, cx, cy, *args, curve, max_epochs=max_epochs)
    for k in spec.FIELDS:
        expect_equal(alone["cen_" + k], want[k], k)
    # peaks without a fit: status 1 and NaN
    rest = peaks["status"] != 0
    assert rest.any() or detrend is not None
    assert (peaks["cen_status"][rest] == 1).all() and all(numpy.isnan(peaks[k][rest]).all() for k in names[1:])
    # the first planet moves the photocentre of the odd curves and of no other: 5 is the line (4e-6 by chance without a shift)
    first = (numpy.abs(peaks["period"] - PLANETS[0][0]) < 0.02 * PLANETS[0][0]) & (peaks["cen_status"] == 0)
    odd = (numpy.arange(N_CURVES) % 2 == 1)[:, None] & first
    even = (numpy.arange(N_CURVES) % 2 == 0)[:, None] & first
    assert odd.sum() >= 3 and even.sum() >= 3
    assert (peaks["cen_significance"][odd] > 5).all() and (peaks["cen_significance"][even] < 5).all()


def test_survey_call_options(ctx, batch):
    """window, min_in, min_out, max_epochs, the template keywords and one row [n] reach the device as the statement has them."""
    flux, cx, cy = (v[:3] for v in batch)
    period, T0, duration = [1.9, 3.1, 1.9, numpy.nan], [3.4, 4.0, 3.9, 3.0], [0.09, 0.11, 0.02, 0.1]
    options = dict(window=2.0, min_in=2, min_out=4, max_epochs=7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = survey.centroid_test(T, flux, cx, cy, period, T0, duration, curve=[2, 1, 1, 0], context=ctx, **options)
        one = survey.centroid_test(T, flux[2], cx[2], cy[2], [1.9], [3.4], [0.09], context=ctx, **options)
        other = survey.centroid_test(T, flux, cx, cy, period, T0, duration, curve=[2, 1, 1, 0], context=ctx, u=[0.1, 0.1], **options)
    want = expected_survey(flux, cx, cy, period, T0, duration, [2, 1, 1, 0], **options)
    for k in spec.FIELDS:
        expect_equal(out["cen_" + k], want[k], k)
    assert out["cen_status"].tolist() == [0, 0, 2, 1] and out["cen_n_skipped"][2] == 7
    assert one.shape == (1,) and one.tobytes() == out[:1].tobytes()
    assert other["cen_n_points"].tobytes() == out["cen_n_points"].tobytes() and other["cen_depth"][0] != out["cen_depth"][0]
