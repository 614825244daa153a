"""tls_spline_detrend on the device against the statement (tests/spline_spec.py), bit for bit in flat, trend and the segment
records, and in the curve records but for the BIC's log (within the ulp bound of spline_cases.equal_curves): on the small shapes
of tests/spline_cases.py (one, two and three points, q = 1 and 2, points on the knots, duplicated stamps, empty and protected
intervals, a lonely point, 255 / 256 / 257 points, an interval with more members than threads, one curve and five, with and
without dy, no clip round, a clip that stops at two members, rows scaled to 1e-100 and 1e100, a segment on either side of
TLS_SPLINE_LDS_POINTS, the widest band, one spacing and three); behind poisoned memory and a larger call, on two contexts,
through the C entry's refusals, and as a step of the survey calls."""
import warnings

import numpy
import pytest

import spline_cases as cases
import spline_spec as spec
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu


def device(ctx, case, **kw):
    flat, trend, fit = ctx.spline_detrend(case["t"], case["y"], dy=case.get("dy"), mask=case.get("mask"), return_trend=True,
                                          return_fit=True, **kw)
    segment = fit["segment"].view("f8").reshape(fit["segment"].shape + (len(spec.SEGMENT_FIELDS),))
    curve = fit["curve"].view("f8").reshape(len(fit["curve"]), -1)
    assert fit["segments"].tolist() == spec.segment_starts(case["t"], kw.get("break_tolerance", 0.5))
    return {"flat": flat, "trend": trend, "segment": segment, "curve": curve}


def check(got, want, kw):
    cases.equal_bits(got, want)
    S = len(numpy.atleast_1d(kw.get("knot_spacing", 0.75)))
    return cases.equal_curves(got["curve"], want["curve"], S)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_bit_equal_to_the_statement(gpu, name):
    """No case leaves the choice open: the two lowest BIC values of every curve stand clear of the log's ulp bound (0 of the
    10 curves of the two cases with several spacings do not; a case with one spacing has one value a curve)."""
    make, kw = cases.CASES[name]
    assert check(device(gpu, make(), **kw), cases.want(name), kw) == 0


def test_the_picks_differ_between_curves():
    """(no device work) the case of three spacings chooses more than one of them."""
    assert len(set(cases.want("three_spacings")["curve"][:, 0].tolist())) >= 2


def test_a_mask_of_zeros_changes_no_byte(gpu):
    make, kw = cases.CASES["n257_5"]
    case = make()
    plain = device(gpu, case, **kw)
    case["mask"] = numpy.zeros(case["y"].shape, dtype=numpy.uint8)
    cases.equal_bits(device(gpu, case, **kw), plain, ("flat", "trend", "segment", "curve"))


def test_a_single_spacing_equals_the_winning_entry(gpu):
    make, kw = cases.CASES["three_spacings"]
    case = make()
    many = device(gpu, case, **kw)
    picks = many["curve"][:, 0].astype(int)
    for k in sorted(set(picks.tolist())):
        one = device(gpu, case, knot_spacing=kw["knot_spacing"][k])
        chosen = picks == k
        for key in ("flat", "trend", "segment"):
            numpy.testing.assert_array_equal(one[key][chosen], many[key][chosen], err_msg=key)
        numpy.testing.assert_array_equal(one["curve"][chosen, 3], many["curve"][chosen, 3 + k])
        assert numpy.all(one["curve"][:, 0] == 0.0)
    first = device(gpu, case, **cases.CASES["two_equal_spacings"][1])
    assert numpy.all(first["curve"][:, 0] != 1.0) and numpy.array_equal(first["curve"][:, 3], first["curve"][:, 4])


def test_poisoned_lds_and_reused_scratch(gpu):
    """The same bytes behind poison_lds with two different words and behind a larger call, in the LDS and on the device-memory
    path: no pass reads LDS or scratch it has not written."""
    names = ("n255_5_dy", "lds_points_and_one", "three_spacings", "lonely_point")
    runs = {k: (cases.CASES[k][0](), cases.CASES[k][1]) for k in names}
    first = {k: device(gpu, case, **kw) for k, (case, kw) in runs.items()}
    for k in names:
        check(first[k], cases.want(k), runs[k][1])
    everything = ("flat", "trend", "segment", "curve")
    cases.equal_bits(device(gpu, *runs["n255_5_dy"][:1], **runs["n255_5_dy"][1]), first["n255_5_dy"], everything)   # behind the larger calls
    for word in (0xFFFFFFFF, 0x7FF00000):
        for k in names:
            gpu.poison_lds(word)
            case, kw = runs[k]
            cases.equal_bits(device(gpu, case, **kw), first[k], everything)


def test_two_contexts_equal_one(gpu):
    make, kw = cases.CASES["three_spacings"]
    case = make()
    dy = numpy.full(case["y"].shape, 5e-4) * (1.0 + 0.5 * (numpy.arange(case["y"].shape[1]) % 2))
    args = dict(kw, dy_batch=dy, return_trend=True, return_fit=True)
    one = survey.spline_batch(case["t"], case["y"], context=gpu, **args)
    two = survey.spline_batch(case["t"], case["y"], devices=[0, 0], **args)
    again = survey.spline_batch(case["t"], case["y"], devices=[0], **args)
    for other in (two, again):
        for a, b in zip(one[:2], other[:2]):
            assert a.tobytes() == b.tobytes()
        assert sorted(one[2]) == sorted(other[2]) == ["curve", "segment", "segments", "spacings"]
        for k in one[2]:
            assert numpy.asarray(one[2][k]).tobytes() == numpy.asarray(other[2][k]).tobytes(), k
    cases.equal_bits({"flat": one[0], "trend": one[1]}, spec.fit(case["t"], case["y"], dy, **kw), ("flat", "trend"))
    # one row
    flat, fit = survey.spline_batch(case["t"], case["y"][2], dy_batch=dy[2], return_fit=True, context=gpu, **kw)
    assert flat.tobytes() == one[0][2].tobytes() and fit["segment"].shape == (1,) and fit["curve"].shape == ()
    assert fit["curve"].tobytes() == one[2]["curve"][2].tobytes()


def test_c_entry_arguments(gpu):
    """n_rows == 0 is a no-op; every TLS_E_ARG case returns before any device work with the outputs untouched."""
    lib, dp = gpu._lib, _lib._dp
    case = cases.rows(numpy.concatenate([cases.grid(30), cases.grid(30, 3.0)]), 2, dy=True)
    n = 60
    flat, trend = numpy.full((2, n), -7.0), numpy.full((2, n), -7.0)
    segment, curve = numpy.full((2, 2, len(spec.SEGMENT_FIELDS)), -7.0), numpy.full((2, 3 + spec.MAX_SPACINGS), -7.0)
    outputs = [flat, trend, segment, curve]
    wide = cases.CASES["widest_band"][0]()

    def call(**kw):
        a = dict(t=case["t"], y=case["y"], dy=case["dy"], n=n, n_rows=2, spacings=[0.75], n_spacings=1, break_tolerance=0.5,
                 penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0)
        a.update(kw)
        arr = lambda v: None if v is None else dp(numpy.ascontiguousarray(v, dtype=numpy.float64))
        return lib.tls_spline_detrend(gpu._h, arr(a["t"]), arr(a["y"]), arr(a["dy"]), None, a["n"], a["n_rows"], arr(a["spacings"]),
                                      a["n_spacings"], a["break_tolerance"], a["penalty"], a["n_iter"], a["sigma_upper"],
                                      a["sigma_lower"], dp(flat), dp(trend), segment.ctypes.data_as(_lib.ctypes.c_void_p),
                                      curve.ctypes.data_as(_lib.ctypes.c_void_p))

    untouched = lambda: all(numpy.all(v == -7.0) for v in outputs)
    assert call(n_rows=0) == 0 and untouched()
    bad_y, bad_dy, bad_t, back = case["y"].copy(), case["dy"].copy(), case["t"].copy(), case["t"].copy()
    bad_y[1, 3], bad_dy[0, 0], bad_t[7], back[5] = 0.0, numpy.inf, numpy.nan, 0.0
    for kw in (dict(n=0), dict(n=100000001), dict(n_rows=-1), dict(n_spacings=0), dict(n_spacings=17), dict(spacings=[0.0]),
               dict(spacings=[numpy.inf]), dict(spacings=[0.5, numpy.nan], n_spacings=2), dict(break_tolerance=0.0),
               dict(break_tolerance=numpy.nan), dict(penalty=-1.0), dict(penalty=numpy.inf), dict(penalty=numpy.nan), dict(n_iter=-1),
               dict(n_iter=17), dict(sigma_upper=0.0), dict(sigma_lower=-1.0), dict(sigma_upper=numpy.nan), dict(sigma_lower=numpy.nan),
               dict(t=bad_t), dict(t=back), dict(y=bad_y), dict(dy=bad_dy), dict(t=None), dict(y=None), dict(spacings=None),
               dict(spacings=[1e-3]),                                                    # 605 intervals in 0.6 d: over the band
               dict(t=wide["t"][:60], spacings=[cases.ONE_MORE_SPACING * 59.0 / 1099.0], break_tolerance=numpy.inf)):   # m = 513
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        message = lib.tls_last_error(gpu._h)
        assert b"spline detrending" in message or b"null argument" in message, (kw, message)
    assert call(sigma_upper=numpy.inf, sigma_lower=numpy.inf, break_tolerance=numpy.inf, n_iter=0) == 0 and not untouched()
    assert call() == 0
    want = spec.fit(case["t"], case["y"], case["dy"])
    cases.equal_bits({"flat": flat, "trend": trend, "segment": segment}, want)
    assert cases.equal_curves(curve, want["curve"], 1) == 0


# ---- as a step of the survey calls ------------------------------------------------------------------------------------------
N_ROWS, STAR_PERIOD, STAR_DEPTH = 1440, 3.37, 1.5e-3
SEARCH = dict(period_min=2.0, period_max=5.0, oversampling_factor=2)
STEP = survey.Spline(0.75)


def _rotators(n_stars=3):
    """n_stars stars of 1440 points that vary by 1 % in 4 to 6 days, with a 0.15 % transit every 3.37 d and noise of 3e-4."""
    t = cases.grid(N_ROWS)
    rng = numpy.random.default_rng(8)
    rows, masks = [], []
    for s in range(n_stars):
        T0 = 1.5 + 0.4 * s
        inside = numpy.abs((t - T0 + 0.5 * STAR_PERIOD) % STAR_PERIOD - 0.5 * STAR_PERIOD) <= 0.06
        star = 1.0 + 0.01 * numpy.sin(2.0 * numpy.pi * t / (4.0 + s) + s)
        rows.append(star * (numpy.where(inside, 1.0 - STAR_DEPTH, 1.0) + 3e-4 * rng.standard_normal(N_ROWS)))
        masks.append(numpy.abs((t - T0 + 0.5 * STAR_PERIOD) % STAR_PERIOD - 0.5 * STAR_PERIOD) <= 0.09)
    return t, numpy.array(rows), numpy.array(masks)


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_power_batch_detrend(gpu):
    t, raw, mask = _rotators()
    flat = survey.spline_batch(t, raw, 0.75, context=gpu)
    assert numpy.std(flat) < 0.2 * numpy.std(raw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_batch(t, raw, detrend=STEP, with_arrays=True, context=gpu, **SEARCH)
        expect = survey.power_batch(t, flat, with_arrays=True, context=gpu, **SEARCH)
        _same_summary(got[0], expect[0])
        for a, b in zip(got[1:], expect[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert numpy.all(numpy.abs(got[0]["period"] / STAR_PERIOD - 1.0) < 0.01), got[0]["period"]
        # in a tuple with the biweight
        got = survey.power_batch(t, raw, detrend=(STEP, survey.Biweight(0.5)), context=gpu, **SEARCH)
        _same_summary(got[0], survey.power_batch(t, survey.biweight_batch(t, flat, 0.5, context=gpu), context=gpu, **SEARCH)[0])
        # with detrend_mask: the step's mask
        masked = survey.spline_batch(t, raw, 0.75, mask=mask, context=gpu)
        assert masked.tobytes() != flat.tobytes()
        got = survey.power_batch(t, raw, detrend=STEP, detrend_mask=mask, context=gpu, **SEARCH)
        _same_summary(got[0], survey.power_batch(t, masked, context=gpu, **SEARCH)[0])
        # weighted with dy_batch, a list of spacings, devices=[0]
        dy = numpy.full(raw.shape, 3e-4) * (1.0 + 0.5 * (numpy.arange(N_ROWS) % 2))
        ladder = survey.Spline([0.5, 0.75, 1.5], n_iter=3)
        got = survey.power_batch(t, raw, dy_batch=dy, detrend=ladder, devices=[0], **SEARCH)
        weighted = survey.spline_batch(t, raw, [0.5, 0.75, 1.5], n_iter=3, dy_batch=dy, context=gpu)
        _same_summary(got[0], survey.power_batch(t, weighted, dy_batch=dy, context=gpu, **SEARCH)[0])
        # the other survey calls
        assert numpy.asarray(survey.search_batch(t, raw, detrend=STEP, context=gpu, **SEARCH)[1]).tobytes() == \
            numpy.asarray(survey.search_batch(t, flat, context=gpu, **SEARCH)[1]).tobytes()
        assert survey.lomb_scargle(t, raw, detrend=STEP, context=gpu)["power"].tobytes() == \
            survey.lomb_scargle(t, flat, context=gpu)["power"].tobytes()
        result, info = survey.power_batch_protected(t, raw, STEP, 7.0, context=gpu, **SEARCH)
        assert info["mask"].shape == raw.shape and info["protected"].shape == (len(raw),)


def test_injection_recovery_and_null_sde_detrend(gpu):
    t, raw, _ = _rotators(1)
    inj = survey.injection_grid(t, [3.0], [0.04, 0.08], per_cell=3, b_max=0.5, seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec, summary, rows = survey.injection_recovery(t, raw[0], inj, detrend=STEP, return_rows=True, context=gpu, **SEARCH)
        injected, count = gpu.inject_transits(t, raw[0], survey.injection_constants(inj), *survey._injection_law(None, None, SEARCH)[1:])
        assert rows.tobytes() == gpu.spline_detrend(t, injected, *STEP).tobytes()
        assert numpy.array_equal(rec["n_in_transit"], count)
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **SEARCH)[0])
        summary, rows = survey.null_sde(t, 5, seed=9, sigma=3e-4, detrend=STEP, return_rows=True, context=gpu, **SEARCH)
        plain = survey.null_sde(t, 5, seed=9, sigma=3e-4, return_rows=True, context=gpu, **SEARCH)[1]
        assert rows.tobytes() == gpu.spline_detrend(t, plain, *STEP).tobytes()
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **SEARCH)[0])
