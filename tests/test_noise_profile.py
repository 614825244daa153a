"""The noise profile on the device (survey.noise_profile / tls_noise_profile; power_batch(peaks=K, peak_fits=True, noise=True))
against tests/noise_profile_spec.py bit for bit (NaN equal to NaN): the records and the three arrays in type, shape and bytes,
at the smallest shapes at which it can go wrong -- n = 3, a single window (n == w), odd and even n, odd and even counts of
valid windows, min_count - 1 of them and none (every window across a gap), w = 1 and the widest window, one clip infinite,
every point of one sign clipped, a constant row beside normal ones, 1, 3 and 40 curves, n on both sides of
_lib.NOISE_LDS_POINTS, and without t --, after poisoned LDS and scratch, behind detrend=, over two contexts, and in the
pipeline with every other result untouched.

Time stamps are multiples of 1/64 d, so every time difference is exact; the flux of some rows lies on a few levels, so ties
are common."""
import warnings

import numpy
import pytest

import noise_profile_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

DT = 1 / 64.0
CAP = _lib.NOISE_LDS_POINTS


@pytest.fixture
def ctx(gpu):
    return gpu


def same(a, b):
    """Bit for bit: the same type, shape and bytes."""
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(got, want, err_msg=str(what))       # (NaN equal to NaN)
    assert same(got, want), what


def stamps(n, gaps=()):
    """n time stamps DT apart, with a hole of 10 samples in front of every index of gaps."""
    step = numpy.ones(n)
    step[0] = 0
    for g in gaps:
        step[g] += 10
    return 1.0 + numpy.cumsum(step) * DT


def noisy(n, seed, levels=0, red=0.0):
    """A row around 1 with scatter 3e-4; levels: on that many quantised levels a sigma; red: plus a random walk."""
    rng = numpy.random.RandomState(seed)
    f = rng.normal(0, 3e-4, n) + red * numpy.cumsum(rng.normal(0, 3e-5, n))
    if levels:
        f = numpy.round(f / 3e-4 * levels) / levels * 3e-4
    return 1.0 + f


def check(ctx, y, widths, t=None, label="", **kw):
    """The device's four arrays equal the statement's; (records, count, robust, rms, the statement's tuple)."""
    y = numpy.atleast_2d(numpy.asarray(y, dtype=float))
    gap = kw.pop("gap_tolerance", 0.5)
    span_max, pair_span = spec.span_limits(t, widths, gap)
    records, count, robust, rms = ctx.noise_profile(t, y, widths, span_max, pair_span, **kw)
    want = spec.noise_profile_batch(y, widths, t, gap_tolerance=gap, **kw)
    assert records.dtype.names == spec.CURVE_FIELDS and records.shape == (len(y),)
    for f in spec.CURVE_FIELDS:
        expect_equal(records[f], want[0][f], (label, f))
    assert count.dtype == numpy.int64
    expect_equal(count, want[1], (label, "count"))
    expect_equal(robust, want[2], (label, "robust"))
    expect_equal(rms, want[3], (label, "rms"))
    return records, count, robust, rms, want


# ---- the smallest shapes ------------------------------------------------------------------------------------------------------
def test_three_points_and_a_single_window(ctx):
    """n = 3 with every width up to n == w (one window), at min_count 1, 2 and 3; ties and a constant row."""
    rows = [[1.0, 1.001, 0.999], [1.0, 1.0, 1.002], [1.0, 1.0, 1.0], [0.0, -0.0, 3.0], [2.0, -1.0, 0.5]]
    for min_count in (1, 2, 3):
        for t in (None, stamps(3), stamps(3, gaps=(2,))):
            records, count, robust, rms, _ = check(ctx, rows, [1, 2, 3], t, min_count=min_count, clip_upper=numpy.inf,
                                                   clip_lower=numpy.inf, label=("n3", min_count))
            assert records["status"].tolist() == [0, 1, 1, 1, 0]
            assert (count[records["status"] == 1] == 0).all() and numpy.isnan(robust[records["status"] == 1]).all()
    assert count[0].tolist() == [3, 1, 1] and count[4].tolist() == [3, 1, 1]        # (the gap cuts one window of 2; the median cadence of 3 stamps is half of it)
    single = check(ctx, rows, [3], None, min_count=1, label="n == w")
    assert single[1][0, 0] == 1 and single[2][0, 0] == 0.0 and single[3][0, 0] == 0.0


@pytest.mark.parametrize("n", (4, 63, 64, 255, 256, 257, 300, 1001))
def test_odd_and_even_rows_with_ties(ctx, n):
    """Odd and even n around the wave and the workgroup, continuous and quantised rows, with and without t."""
    y = [noisy(n, n), noisy(n, n + 1, levels=2), noisy(n, n + 2, levels=1, red=1.0)]
    widths = sorted({1, 2, 3, min(n, 7), min(n, 64), n})
    check(ctx, y, widths, stamps(n, gaps=(n // 2,)), label=("gap", n))
    check(ctx, y, widths, None, label=("no t", n))


def test_counts_odd_even_short_and_none(ctx):
    """Two stretches of 5 and 6 samples: the widths 3 .. 7 leave 7, 5, 3, 1 and 0 valid windows; min_count 4 makes the
    count 3 one short, min_count 1 keeps the single window; every window of the widest is across the gap."""
    t = stamps(11, gaps=(5,))
    y = [noisy(11, 5), noisy(11, 6, levels=1)]
    for min_count in (1, 3, 4):
        _, count, robust, rms, _ = check(ctx, y, [2, 3, 4, 5, 6, 7], t, min_count=min_count, clip_upper=numpy.inf,
                                         clip_lower=numpy.inf, label=("counts", min_count))
        assert count[0].tolist() == [9, 7, 5, 3, 1, 0]
        assert numpy.isnan(robust[0]).tolist() == [c < min_count for c in count[0]]
        assert numpy.isnan(rms[0]).tolist() == [c < min_count for c in count[0]]
    # even counts of valid windows (an even median of v), by clipping
    _, count, _, _, _ = check(ctx, y, [1, 2, 3], stamps(11), clip_upper=1.0, clip_lower=1.0, min_count=1, label="clipped counts")
    assert (count < [11, 10, 9]).all()


def test_narrowest_and_widest_window(ctx):
    """w = 1 and w = NOISE_MAX_WIDTH in one call, in the LDS and beyond it."""
    for n, seed in ((_lib.NOISE_MAX_WIDTH + 7, 3), (CAP + 300, 4)):
        y = [noisy(n, seed, red=1.0), noisy(n, seed + 10, levels=3)]
        _, count, robust, _, _ = check(ctx, y, [1, 450, _lib.NOISE_MAX_WIDTH], stamps(n), label=("widest", n))
        assert (count[:, 0] > count[:, 2]).all() and (count[:, 2] >= 3).all() and numpy.isfinite(robust).all()


@pytest.mark.parametrize("n", (CAP - 1, CAP, CAP + 1))
def test_both_sides_of_the_lds_cap(ctx, n):
    y = [noisy(n, 20, levels=2), noisy(n, 21, red=1.0), numpy.ones(n)]
    records, count, _, _, _ = check(ctx, y, [1, 6, 13, 100], stamps(n, gaps=(n // 3, n // 2)), label=("cap", n))
    assert records["status"].tolist() == [0, 0, 1]
    check(ctx, y[:2], [2, 30], None, clip_upper=2.0, clip_lower=numpy.inf, label=("cap, no t", n))


def test_clips(ctx):
    """One clip infinite, the other tight; a clip of 0 drops every point of one sign; an eclipse is clipped whole."""
    n = 400
    y = noisy(n, 30)
    y[100:110] -= 0.01
    y[250] += 0.02
    rows = [y, noisy(n, 31, levels=2)]
    t = stamps(n, gaps=(200,))
    widths = [1, 2, 5, 12]
    both = check(ctx, rows, widths, t, label="5 5")[0]
    assert both["n_clipped"][0] == 11
    up = check(ctx, rows, widths, t, clip_upper=numpy.inf, clip_lower=5.0, label="inf 5")[0]
    assert up["n_clipped"][0] == 10
    down = check(ctx, rows, widths, t, clip_upper=5.0, clip_lower=numpy.inf, label="5 inf")[0]
    assert down["n_clipped"][0] == 1
    none = check(ctx, rows, widths, t, clip_upper=numpy.inf, clip_lower=numpy.inf, label="inf inf")[0]
    assert (none["n_clipped"] == 0).all()
    # every point below the median goes, then every point above it
    low = check(ctx, rows, widths, t, clip_upper=numpy.inf, clip_lower=0.0, min_count=1, label="inf 0")
    assert (low[0]["n_clipped"] >= n // 4).all() and (low[0]["n_clipped"] <= n // 2).all()
    high = check(ctx, rows, widths, t, clip_upper=0.0, clip_lower=numpy.inf, min_count=1, label="0 inf")
    assert (high[0]["n_clipped"] >= n // 4).all() and (high[0]["n_clipped"] <= n // 2).all()
    # both: only the points ON the median stay (ties on the quantised row)
    on = check(ctx, rows, widths, t, clip_upper=0.0, clip_lower=0.0, min_count=1, label="0 0")
    assert on[0]["n_clipped"][1] < n and on[0]["n_pairs"][0] == 0 and numpy.isnan(on[0]["sigma_p2p"][0])


@pytest.mark.parametrize("curves", (1, 3, 40))
def test_curves_of_a_call(ctx, curves):
    """1, 3 and 40 curves; a constant row and a row with more than half of it on one value beside normal ones."""
    n = 333
    y = [noisy(n, 40 + r, levels=r % 3, red=float(r % 2)) for r in range(curves)]
    if curves > 1:
        y[1] = numpy.full(n, 0.75)
    if curves > 3:
        y[7] = numpy.where(numpy.arange(n) % 3 == 0, noisy(n, 99), 1.0)
    records, count, _, _, _ = check(ctx, y, [1, 3, 6, 13, 48], stamps(n, gaps=(100, 101)), label=("curves", curves))
    want = [1 if r in ((1,) if curves > 1 else ()) + ((7,) if curves > 3 else ()) else 0 for r in range(curves)]
    assert records["status"].tolist() == want
    assert (count[numpy.array(want) == 0] > 0).all()


def test_argument_errors(ctx):
    y = noisy(50, 1)
    for bad in (dict(widths=[0, 2]), dict(widths=[2, 2]), dict(widths=[51]), dict(widths=[3, 2]), dict(clip_upper=-1.0),
                dict(clip_lower=numpy.nan), dict(min_count=0)):
        kw = dict(dict(widths=[1, 2]), **bad)
        widths = kw.pop("widths")
        with pytest.raises(ValueError):
            ctx.noise_profile(None, y, widths, [numpy.inf] * len(widths), numpy.inf, **kw)
    with pytest.raises(ValueError):
        ctx.noise_profile(None, y[:2], [1], [numpy.inf], numpy.inf)
    with pytest.raises(ValueError):
        ctx.noise_profile(stamps(50)[::-1], y, [1], [numpy.inf], numpy.inf)


# ---- memory -----------------------------------------------------------------------------------------------------------------
def test_poisoned_lds_and_reused_scratch(ctx):
    """The same call before and after tls_debug_poison_lds (every CU's LDS and the call's device buffers smeared) agrees byte
    for byte, in the LDS and beyond it; a small call behind a large one reuses the buffers and agrees."""
    for n in (700, CAP + 300):
        t = stamps(n, gaps=(n // 2,))
        y = numpy.array([noisy(n, 17), noisy(n, 18, levels=2), numpy.ones(n)])
        span, pair = spec.span_limits(t, [1, 4, 9], 0.5)
        span_l, pair_l = spec.span_limits(t, [1, 2, 3, 5, 8, 13, 21, 34, 55], 0.5)
        small_args = (t[:n // 3], y[:2, :n // 3], [1, 4, 9], span, pair)
        large_args = (t, y, [1, 2, 3, 5, 8, 13, 21, 34, 55], span_l, pair_l)
        small = ctx.noise_profile(*small_args)
        large = ctx.noise_profile(*large_args)
        behind = ctx.noise_profile(*small_args)
        ctx.poison_lds(0xFFFFFFFF)
        again = ctx.noise_profile(*small_args)
        ctx.poison_lds(0x7FF00000)
        large_again = ctx.noise_profile(*large_args)
        for a, b in zip(small + small + large, behind + again + large_again):
            assert same(a, b), n
        want = spec.noise_profile_batch(y[:2, :n // 3], [1, 4, 9], t[:n // 3])
        for f in spec.CURVE_FIELDS:
            expect_equal(again[0][f], want[0][f], (n, f))
        for got, w in zip(again[1:], want[1:4]):
            expect_equal(got, w, n)


# ---- survey.noise_profile and the pipeline ----------------------------------------------------------------------------------
T = 3.0 + numpy.arange(500) / 16.0                    # 31 d at 90 min
KW = dict(period_min=1.5, period_max=6, oversampling_factor=1)
_RUNS = {}


def flux_rows():
    """4 rows of 500 points: three with a planet, one quiet."""
    if "flux" not in _RUNS:
        rows = []
        for s, (per, rp) in enumerate(((2.9, 0.1), (4.3, 0.12), (3.7, 0.15), (0.0, 0.0))):
            rng = numpy.random.RandomState(3000 + s)
            f = 1.0 + rng.normal(0, 3e-4, len(T)) + 1e-3 * numpy.sin(T / 2.3 + s)
            if per:
                f += transit_model.light_curve(T, T[0] + 0.8, per, rp, 9.0, 89.9, 0, 90, [0.4, 0.3], "quadratic") - 1
            rows.append(f)
        _RUNS["flux"] = numpy.array(rows)
    return _RUNS["flux"]


def run(ctx, **more):
    key = tuple(sorted((k, repr(v)) for k, v in more.items()))
    if key not in _RUNS:
        kw = dict(more)
        if "devices" not in kw:
            kw["context"] = ctx
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _RUNS[key] = survey.power_batch(T, flux_rows(), peaks=4, peak_fits=True, **kw, **KW)
    return _RUNS[key]


def expect_profile(got, want_rows, widths, t):
    want = spec.noise_profile_batch(want_rows, widths, t)
    expect_equal(got["widths"], numpy.asarray(widths, dtype=numpy.int64), "widths")
    for f in spec.CURVE_FIELDS:
        expect_equal(got["curves"][f], want[0][f], f)
    for k, w in zip(("count", "robust", "rms", "beta"), want[1:]):
        expect_equal(got[k], w, k)


def test_survey_entry(ctx):
    """survey.noise_profile: the default widths, one row in and one row out, detrend=25 and two contexts."""
    flux = flux_rows()
    widths = survey.noise_widths(T)
    assert widths.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10]
    got = survey.noise_profile(flux, T, context=ctx)
    assert set(got) == {"widths", "curves", "count", "robust", "rms", "beta"}
    assert got["curves"].dtype.names == survey.noise_curve_fields()
    expect_profile(got, flux, widths, T)
    one = survey.noise_profile(flux[2], T, context=ctx)
    assert one["robust"].shape == (len(widths),) and one["curves"].shape == ()
    for k in ("count", "robust", "rms", "beta", "curves"):
        assert same(one[k], got[k][2]), k
    no_t = survey.noise_profile(flux, widths=[1, 5], context=ctx)
    expect_profile(no_t, flux, [1, 5], None)
    flat = survey.detrend_batch(flux, 25, context=ctx)
    detrended = survey.noise_profile(flux, T, detrend=25, context=ctx)
    expect_profile(detrended, flat, widths, T)
    assert (detrended["robust"][:, -1] < got["robust"][:, -1]).all()            # (the sinusoid is gone: less red noise)
    two = survey.noise_profile(flux, T, devices=[0, 0])
    for k in got:
        assert same(two[k], got[k]), k


def test_pipeline(ctx):
    """noise=True: the profile is survey.noise_profile of the rows searched, the three peak fields are the host formula, and
    every other output is byte-equal to the call without the keyword."""
    got, without = run(ctx, noise=True), run(ctx)
    assert got[0].dtype == without[0].dtype and got[0].tobytes() == without[0].tobytes()
    expect_equal(got[1], without[1], "periods")
    pk, base = got[2], without[2]
    assert set(pk) == set(base) | {"noise"}
    assert pk["peaks"].dtype.names == base["peaks"].dtype.names + ("noise_width", "noise_sigma", "noise_mes")
    for k in base["peaks"].dtype.names:
        assert pk["peaks"][k].tobytes() == base["peaks"][k].tobytes(), k
    for k in base:
        if k != "peaks":
            assert same(pk[k], base[k]), k
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y_rows = survey._batch_inputs(T, flux_rows(), None, dict(KW))[1]
    alone = survey.noise_profile(y_rows, T, context=ctx)
    assert set(pk["noise"]) == set(alone)
    for k in alone:
        assert same(pk["noise"][k], alone[k]), k
    expect_profile(pk["noise"], y_rows, survey.noise_widths(T), T)
    # the host formula, peak by peak
    peaks, widths, cadence = pk["peaks"], alone["widths"], numpy.median(numpy.diff(T))
    assert peaks.shape == (4, 4) and (peaks["status"] == 0).sum() >= 4
    for c in range(4):
        for r in range(4):
            p = peaks[c, r]
            width, sigma, mes = -1.0, numpy.nan, numpy.nan
            if p["status"] == 0:
                distance = numpy.abs(widths - p["duration_days"] / cadence)
                k = int(numpy.flatnonzero(distance == distance.min())[0])
                if not numpy.isnan(alone["robust"][c, k]):
                    width, sigma = float(widths[k]), alone["robust"][c, k]
                    mes = p["depth_mean"] * numpy.sqrt(p["transit_count"]) / sigma
            expect_equal(p["noise_width"], numpy.float64(width), (c, r))
            expect_equal(p["noise_sigma"], numpy.float64(sigma), (c, r))
            expect_equal(p["noise_mes"], numpy.float64(mes), (c, r))
    assert (peaks["noise_width"][peaks["status"] == 0] >= 1).all()
    # two contexts and explicit widths
    two = run(ctx, noise=True, devices=[0, 0])
    assert two[2]["peaks"].tobytes() == pk["peaks"].tobytes()
    for k in alone:
        assert same(two[2]["noise"][k], alone[k]), k
    given = run(ctx, noise=[2, 9])
    expect_profile(given[2]["noise"], y_rows, [2, 9], T)
    assert set(given[2]["peaks"]["noise_width"][peaks["status"] == 0]) <= {2.0, 9.0}
    with pytest.raises(ValueError):
        survey.power_batch(T, flux_rows(), peaks=4, noise=True, context=ctx, **KW)
    with pytest.raises(ValueError):
        survey.power_batch(T, flux_rows(), peaks=4, peak_fits=True, noise=[3, 2], context=ctx, **KW)
