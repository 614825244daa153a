"""tls_clean_rows on the device against the statement (tests/clean_spec.py), bit for bit in rows, flags and records: on the
small shapes of tests/clean_cases.py (1 to 1367 points and 1 to 5 rows, windows across tile boundaries, of one sample, longer
than the row and short of min_points, missing points at both ends, a segment and a row of them, a constant row, ties,
duplicated stamps, runs at a boundary and across a missing point, max_run 1 to 3, 0, 1 and 16 rounds a point each, the guard,
the caller's flags), on both sides of the selection's LDS limit, on a 2-minute row of 19 440 points, behind poisoned memory
and a larger call, on two contexts, and as a step of power_batch."""
import math
import warnings

import numpy
import pytest

import clean_cases as cases
import clean_spec as spec
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu


def device(ctx, t, y, bad, kw):
    return ctx.clean_rows(t, y, bad=bad, return_flags=True, return_record=True, **kw)


def expect_equal(got, want, what=""):
    rows, flags, record = got
    assert cases.same(flags, want[1]), (what, numpy.argwhere(flags != want[1])[:5])
    assert cases.same(rows, want[0]), (what, numpy.argwhere(rows != want[0])[:5])
    for k in spec.FIELDS:
        assert cases.same(record[k], want[2][k]), (what, k, record[k], want[2][k])
    assert record.dtype == _lib.CLEAN_DTYPE and _lib.CLEAN_FIELDS == spec.FIELDS
    assert numpy.all(numpy.isfinite(rows) & (rows > 0.0))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_bit_equal_to_the_statement(gpu, name):
    t, y, bad, kw = cases.CASES[name]
    expect_equal(device(gpu, t, y, bad, kw), cases.expected(name), name)


def test_bad_of_zeros_changes_no_byte(gpu):
    for name in ("bad", "bad_slide"):
        t, y, _, kw = cases.CASES[name]
        plain = device(gpu, t, y, None, kw)
        zeros = device(gpu, t, y, numpy.zeros(y.shape, dtype=numpy.uint8), kw)
        for a, b in zip(plain, zeros):
            assert cases.same(a, b), name


def test_one_row_is_a_row(gpu):
    t, y, _, kw = cases.CASES["slide_n64"]
    rows, flags, record = device(gpu, t, y[1], None, kw)
    want = cases.expected("slide_n64")
    assert rows.shape == (64,) and cases.same(rows, want[0][1]) and cases.same(flags, want[1][1]) and record == want[2][1]


@pytest.mark.parametrize("n", [_lib.CLEAN_LDS_POINTS, _lib.CLEAN_LDS_POINTS + 1])
def test_both_sides_of_the_lds_limit(gpu, n):
    """Two rows with the row's median as their centre: the residuals of a round in the LDS, and in device memory."""
    assert _lib.CLEAN_LDS_POINTS == _lib.NOISE_LDS_POINTS == 8192
    t = cases.series(n, gap_at=5000)
    y = cases.dirty_rows(n, 2, seed=n, nan_share=0.01, flares=6, dips=4)
    kw = dict(sigma_upper=4.0, sigma_lower=5.0, n_iter=4)
    want = spec.clean(t, y, **kw)
    assert want[2]["n_high"].min() > 0 and want[2]["n_low"].min() > 0 and want[2]["rounds"].min() >= 2
    expect_equal(device(gpu, t, y, None, kw), want, n)


def test_two_minute_row(gpu):
    """One row of 19 440 points (27 d at 2 minutes) with a sliding centre of 0.5 d, 361 points a window: many tiles, and the
    rounds' medians in device memory."""
    n = 19440
    t = numpy.arange(n, dtype=numpy.float64) / 720.0
    t[n // 2:] += 1.0
    y = cases.dirty_rows(n, 1, seed=27, nan_share=0.01, flares=10, dips=6)
    kw = dict(window_length=0.5, sigma_upper=4.0, sigma_lower=5.0)
    want = spec.clean(t, y, **kw)
    assert want[2]["n_high"][0] > 0 and want[2]["rounds"][0] >= 2
    expect_equal(device(gpu, t, y, None, kw), want)


def test_poisoned_lds_and_reused_scratch(gpu):
    """The same small call before a large one, and behind it with every CU's LDS and the context's scratch smeared, agrees byte
    for byte, in the LDS and beyond it, with the row's median and with a sliding centre."""
    small = [(name,) + cases.CASES[name] for name in ("slide_n64", "flat_n64", "segment_missing_slide", "row_missing")]
    first = [device(gpu, t, y, bad, kw) for _, t, y, bad, kw in small]
    n = _lib.CLEAN_LDS_POINTS + 300
    t = cases.series(n, gap_at=3000)
    y = cases.dirty_rows(n, 3, seed=4, nan_share=0.01)
    large = [device(gpu, t, y, None, dict(window_length=0.5, sigma_upper=4.0, sigma_lower=5.0)),
             device(gpu, t, y, None, dict(sigma_upper=4.0, sigma_lower=5.0))]
    for word in (0xFFFFFFFF, 0x7FF00000):
        gpu.poison_lds(word)
        for (name, t_s, y_s, bad, kw), before in zip(small, first):
            again = device(gpu, t_s, y_s, bad, kw)
            for a, b in zip(again, before):
                assert cases.same(a, b), (name, word)
            expect_equal(again, cases.expected(name), name)
    gpu.poison_lds(0xFFFFFFFF)
    again = [device(gpu, t, y, None, dict(window_length=0.5, sigma_upper=4.0, sigma_lower=5.0)),
             device(gpu, t, y, None, dict(sigma_upper=4.0, sigma_lower=5.0))]
    for got, before in zip(again, large):
        for a, b in zip(got, before):
            assert cases.same(a, b)


def test_on_two_contexts(gpu):
    t, y, bad, kw = cases.CASES["bad_slide"]
    args = dict(kw, bad=bad, return_flags=True, return_record=True)
    one = survey.clean_batch(t, y, context=gpu, **args)
    expect_equal(one, cases.expected("bad_slide"))
    for devices in ([0, 0], [0]):
        other = survey.clean_batch(t, y, devices=devices, **args)
        for a, b in zip(one, other):
            assert cases.same(a, b), devices
    assert survey.clean_fields() == spec.FIELDS
    assert cases.same(survey.clean_batch(t, y, context=gpu, **dict(kw, bad=bad)), one[0])


def test_the_c_entry_refuses(gpu):
    """TLS_E_ARG with the outputs untouched for what the header names; NULL flags are allowed."""
    import ctypes
    t, y, _, _ = cases.CASES["flat_n64"]
    t, y = numpy.ascontiguousarray(t), numpy.ascontiguousarray(y)
    rows = numpy.full(y.shape, -7.0)
    record = numpy.full(len(y), -7.0, dtype=_lib.CLEAN_DTYPE)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731

    def call(**over):
        a = dict(t=t, n=len(t), window_length=0.0, break_tolerance=0.5, sigma_upper=4.0, sigma_lower=math.inf, max_run=1, n_iter=3,
                 min_points=3)
        a.update(over)
        return gpu._lib.tls_clean_rows(gpu._h, dp(a["t"]), dp(y), None, a["n"], len(y), a["window_length"], a["break_tolerance"],
                                       a["sigma_upper"], a["sigma_lower"], a["max_run"], a["n_iter"], a["min_points"], dp(rows), None,
                                       record.ctypes.data_as(ctypes.c_void_p))

    for over in (dict(n=0), dict(window_length=-1.0), dict(window_length=math.nan), dict(window_length=math.inf),
                 dict(break_tolerance=0.0), dict(sigma_upper=0.0), dict(sigma_lower=math.nan), dict(max_run=0), dict(n_iter=-1),
                 dict(n_iter=17), dict(min_points=0), dict(t=numpy.ascontiguousarray(t[::-1]))):
        assert call(**over) == -1, over
        assert numpy.all(rows == -7.0) and numpy.all(record["status"] == -7.0), over
        assert b"cleaning" in gpu._lib.tls_last_error(gpu._h), over
    assert call() == 0
    want = spec.clean(t, y, **spec.DEFAULTS)
    assert cases.same(rows, want[0]) and cases.same(record, want[2])


# ---- as a step of the survey calls ------------------------------------------------------------------------------------------
SEARCH = dict(period_min=2.0, period_max=5.0, oversampling_factor=2)


def _rows_with_nans():
    """Five rows of 1440 points with a 0.3 % transit every 3.37 d, noise of 3e-4, NaN and a flare each."""
    n = 1440
    t = 1.0 + numpy.arange(n, dtype=numpy.float64) / 48.0
    rng = numpy.random.default_rng(12)
    rows = []
    for s in range(5):
        inside = numpy.abs((t - 1.5 - 0.4 * s + 0.5 * 3.37) % 3.37 - 0.5 * 3.37) <= 0.06
        y = numpy.where(inside, 1.0 - 3e-3, 1.0) + 3e-4 * rng.standard_normal(n)
        y[rng.choice(n, size=20, replace=False)] = numpy.nan
        a = int(rng.integers(0, n - 6))
        y[a:a + 6] += 0.01 * numpy.exp(-numpy.arange(6) / 2.0)
        rows.append(y)
    return t, numpy.array(rows)


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_power_batch_step(gpu):
    t, raw = _rows_with_nans()
    step = survey.Clean(None, 4.0, 5.0)
    cleaned, flags = survey.clean_batch(t, raw, None, 0.5, 4.0, 5.0, return_flags=True, context=gpu)
    assert numpy.array_equal((flags & 1) != 0, numpy.isnan(raw)) and ((flags & 4) != 0).sum() >= 5
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError):
            survey.power_batch(t, raw, detrend=25, context=gpu, **SEARCH)
        got = survey.power_batch(t, raw, detrend=(step, 25), with_arrays=True, context=gpu, **SEARCH)
        expect = survey.power_batch(t, cleaned, detrend=25, with_arrays=True, context=gpu, **SEARCH)
        _same_summary(got[0], expect[0])
        for a, b in zip(got[1:], expect[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert numpy.all(numpy.abs(got[0]["period"] / 3.37 - 1.0) < 0.01), got[0]["period"]
        # alone, on the other calls, and with a mask for the steps behind it
        _same_summary(survey.power_batch(t, raw, detrend=step, context=gpu, **SEARCH)[0],
                      survey.power_batch(t, cleaned, context=gpu, **SEARCH)[0])
        assert numpy.asarray(survey.search_batch(t, raw, detrend=step, context=gpu, **SEARCH)[1]).tobytes() == \
            numpy.asarray(survey.search_batch(t, cleaned, context=gpu, **SEARCH)[1]).tobytes()
        assert survey.lomb_scargle(t, raw, detrend=step, context=gpu)["power"].tobytes() == \
            survey.lomb_scargle(t, cleaned, context=gpu)["power"].tobytes()
        mask = numpy.zeros(raw.shape, dtype=numpy.uint8)
        mask[:, 100:110] = 1
        _same_summary(survey.power_batch(t, raw, detrend=(step, survey.Biweight(0.5)), detrend_mask=mask, context=gpu, **SEARCH)[0],
                      survey.power_batch(t, cleaned, detrend=survey.Biweight(0.5), detrend_mask=mask, context=gpu, **SEARCH)[0])
        # the rows formed on the device: injections into a row with NaN, and null rows
        inj = survey.injection_grid(t, [3.37], [0.05], per_cell=2, seed=3)
        rec, summary, rows = survey.injection_recovery(t, raw[0], inj, detrend=step, return_rows=True, context=gpu, **SEARCH)
        injected, _ = gpu.inject_transits(t, raw[0], survey.injection_constants(inj), *survey._injection_law(None, None, SEARCH)[1:])
        assert rows.tobytes() == gpu.clean_rows(t, injected, None, 0.5, 4.0, 5.0).tobytes()
        summary, rows = survey.null_sde(t, 3, seed=9, sigma=3e-4, detrend=step, return_rows=True, context=gpu, **SEARCH)
        plain = survey.null_sde(t, 3, seed=9, sigma=3e-4, return_rows=True, context=gpu, **SEARCH)[1]
        assert rows.tobytes() == gpu.clean_rows(t, plain, None, 0.5, 4.0, 5.0).tobytes()
