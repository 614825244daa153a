"""tls_decorrelate on the device against the statement (tests/decorrelate_spec.py), bit for bit in flat, trend, the record and
the three tables: on both sides of a tile of 256 points and of two, one column and sixteen, shared, own and both, with and
without dy, one curve and five, segments (a single point, fewer points than columns, one wholly protected), dropped columns,
no clip round, a clip that empties F, rows scaled to 1e-300 and 1e300, and F in device scratch; behind poisoned memory and a
larger call, through the C entry's refusals, on two contexts, and as a step of the survey calls."""
import hashlib
import warnings

import numpy
import pytest

import decorrelate_cases as cases
import decorrelate_spec as spec
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu


def device(ctx, case, **kw):
    flat, trend, fit = ctx.decorrelate(case["y"], case.get("own"), case.get("shared"), case.get("dy"), case.get("mask"),
                                       case.get("segments"), return_trend=True, return_fit=True, **kw)
    record = fit["record"].view("f8").reshape(fit["record"].shape + (len(spec.FIELDS),))
    return {"flat": flat, "trend": trend, "record": record, "coef": fit["coef"], "mean": fit["mean"], "scale": fit["scale"],
            "coefficients": fit["coefficients"]}


def _segmented():
    n = 300
    case = cases.small(n, 2, 3, n_curves=2, dy=True)
    case["segments"] = [0, 1, 4, 150, n]                     # a single point, fewer points than columns, two ordinary ones
    case["mask"] = numpy.zeros((2, n), dtype=numpy.uint8)
    case["mask"][0, 150:] = 1                                # a whole segment protected
    case["mask"][1, 20:30] = 1
    return case


def _degenerate():
    case = cases.small(120, 1, 4, n_curves=2)
    case["own"][:, 2] = case["own"][:, 0]
    case["own"][:, 3] = 0.0
    return case


def _scaled():
    case = cases.small(257, 1, 2, n_curves=3)
    case["y"] = case["y"] * numpy.array([1e-300, 1.0, 1e300])[:, None]
    return case


def _scratch():
    """One segment of LDS_POINTS + 1 points: F lives in device scratch; a mask and outliers, so that it is read and cleared."""
    n = spec.LDS_POINTS + 1
    case = cases.small(n, 1, 1, n_curves=2)
    case["mask"] = (numpy.random.default_rng(4).random((2, n)) < 0.05).astype(numpy.uint8)
    return case


CASES = {
    "n1_shared": (lambda: cases.small(1, 1, 0), {}),
    "n2_own_dy": (lambda: cases.small(2, 0, 1, dy=True), {}),
    "n255_both_dy_5": (lambda: cases.small(255, 2, 3, n_curves=5, dy=True), {}),
    "n256_own16": (lambda: cases.small(256, 0, 16), {}),
    "n257_shared16_dy_5": (lambda: cases.small(257, 16, 0, n_curves=5, dy=True, strength=0.005), {}),
    "n513_both_5": (lambda: cases.small(513, 3, 2, n_curves=5), {"ridge": 1e-6, "sigma_upper": 3.0, "sigma_lower": numpy.inf}),
    "segments": (_segmented, {}),
    "dropped_columns": (_degenerate, {}),
    "no_clip_round": (lambda: cases.small(257, 2, 3, n_curves=2, dy=True), {"n_iter": 0}),
    "clip_empties_F": (lambda: cases.small(9, 0, 3, n_curves=4), {"sigma_upper": 0.5, "sigma_lower": 0.5}),
    "scaled_rows": (_scaled, {}),
    "scratch_F": (_scratch, {}),
}
_WANT = {}


def want(name):
    """The statement of a case, formed once."""
    if name not in _WANT:
        make, kw = CASES[name]
        _WANT[name] = cases.statement(make(), **kw)
    return _WANT[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_equal_to_the_statement(gpu, name):
    make, kw = CASES[name]
    cases.equal_bits(device(gpu, make(), **kw), want(name))


def test_the_cases_are_what_they_say():
    """(no device work) the statement reaches the paths the names promise."""
    record = want("segments")["record"]
    assert record[:, :2, 0].tolist() == [[1.0, 1.0], [1.0, 1.0]] and record[0, 3, 0] == 1.0 and record[1, 2:, 0].tolist() == [0.0, 0.0]
    assert numpy.all(want("dropped_columns")["record"][:, 0, 1] == 24.0)
    record = want("clip_empties_F")["record"][:, 0]
    assert numpy.any((record[:, 0] == 1.0) & (record[:, 4] >= 1.0) & (record[:, 3] > 0.0)), record     # status 1 behind a clip round
    assert numpy.all(want("no_clip_round")["record"][..., 4] == 0.0) and numpy.all(want("no_clip_round")["record"][..., 3] == 0.0)
    assert numpy.all(want("scratch_F")["record"][..., 3] > 0.0) and numpy.all(want("scaled_rows")["record"][..., 0] == 0.0)
    assert numpy.all(want("n513_both_5")["record"][..., 3] > 0.0)


def test_a_mask_of_zeros_changes_no_byte(gpu):
    case = cases.small(257, 2, 3, n_curves=2, dy=True)
    plain = device(gpu, case)
    case["mask"] = numpy.zeros(case["y"].shape, dtype=numpy.uint8)
    cases.equal_bits(device(gpu, case), plain)


def test_dropped_columns_leave_the_others(gpu):
    case = _degenerate()
    full = device(gpu, case)
    assert numpy.all(full["record"][:, 0, 1] == 24.0) and numpy.all(full["coef"][..., 3:] == 0.0)
    assert numpy.all(full["coefficients"][..., 3:] == 0.0)
    case["own"] = numpy.ascontiguousarray(case["own"][:, :2])
    kept = device(gpu, case)
    cases.equal_bits({"coef": full["coef"][..., :3], "flat": full["flat"]}, {"coef": kept["coef"], "flat": kept["flat"]}, ("coef", "flat"))


def test_poisoned_lds_and_reused_scratch(gpu):
    """The same bytes behind poison_lds and behind a larger call: no pass reads LDS or scratch it has not written."""
    small, large = CASES["n255_both_dy_5"][0](), _scratch()
    first = device(gpu, small)
    cases.equal_bits(first, want("n255_both_dy_5"))
    first_large = device(gpu, large)
    cases.equal_bits(device(gpu, small), first)
    gpu.poison_lds()
    cases.equal_bits(device(gpu, small), first)
    gpu.poison_lds()
    cases.equal_bits(device(gpu, large), first_large)
    cases.equal_bits(device(gpu, _segmented()), want("segments"))


def test_c_entry_arguments(gpu):
    """n_curves == 0 is a no-op; every TLS_E_ARG case returns before any device work with the outputs untouched."""
    lib, dp, ip = gpu._lib, _lib._dp, _lib._ip
    case = cases.small(40, 1, 2, n_curves=2, dy=True)
    n = 40
    flat, trend = numpy.full((2, n), -7.0), numpy.full((2, n), -7.0)
    record = numpy.full((2, 1, 8), -7.0)
    tables = [numpy.full((2, 1, 3), -7.0) for _ in range(3)]
    outputs = [flat, trend, record] + tables

    def call(**kw):
        a = dict(y=case["y"], dy=case["dy"], n=n, n_curves=2, shared=case["shared"], n_shared=1, own=case["own"], n_own=2,
                 segments=[0, n], n_segments=1, ridge=0.0, n_iter=3, sigma_upper=5.0, sigma_lower=5.0)
        a.update(kw)
        arr = lambda v: None if v is None else dp(numpy.ascontiguousarray(v, dtype=numpy.float64))
        seg = numpy.ascontiguousarray(a["segments"], dtype=numpy.int64)
        return lib.tls_decorrelate(gpu._h, arr(a["y"]), arr(a["dy"]), None, a["n"], a["n_curves"], arr(a["shared"]), a["n_shared"],
                                   arr(a["own"]), a["n_own"], ip(seg), a["n_segments"], a["ridge"], a["n_iter"], a["sigma_upper"],
                                   a["sigma_lower"], dp(flat), dp(trend), record.ctypes.data_as(_lib.ctypes.c_void_p),
                                   *(dp(v) for v in tables))

    untouched = lambda: all(numpy.all(v == -7.0) for v in outputs)
    assert call(n_curves=0) == 0 and untouched()
    bad_y, bad_dy, bad_own, bad_shared = case["y"].copy(), case["dy"].copy(), case["own"].copy(), case["shared"].copy()
    bad_y[1, 3], bad_dy[0, 0], bad_own[1, 1, 5], bad_shared[0, 39] = 0.0, numpy.inf, numpy.nan, -numpy.inf
    for kw in (dict(n=0), dict(n=100000001), dict(n_curves=-1), dict(n_shared=0, n_own=0), dict(n_shared=-1), dict(n_own=17),
               dict(n_shared=15, n_own=2), dict(n_segments=0), dict(n_segments=n + 1), dict(segments=[1, n]), dict(segments=[0, n - 1]),
               dict(segments=[0, 20, 20, n], n_segments=3), dict(segments=[0, 30, 20, n], n_segments=3), dict(ridge=-1.0),
               dict(ridge=numpy.inf), dict(ridge=numpy.nan), dict(n_iter=-1), dict(n_iter=17), dict(sigma_upper=0.0),
               dict(sigma_lower=-1.0), dict(sigma_upper=numpy.nan), dict(sigma_lower=numpy.nan), dict(y=bad_y), dict(dy=bad_dy),
               dict(own=bad_own), dict(shared=bad_shared), dict(y=None), dict(own=None), dict(shared=None)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        message = lib.tls_last_error(gpu._h)
        assert b"decorrelation" in message or b"null argument" in message, (kw, message)
    assert call(sigma_upper=numpy.inf, sigma_lower=numpy.inf) == 0 and not untouched()
    assert call() == 0
    cases.equal_bits({"flat": flat, "trend": trend, "record": record, "coef": tables[0], "mean": tables[1], "scale": tables[2]},
                     cases.statement(case))


def test_two_contexts_equal_one(gpu):
    case = CASES["n255_both_dy_5"][0]()
    kw = dict(own=case["own"], shared=case["shared"], dy_batch=case["dy"], return_trend=True, return_fit=True)
    one = survey.decorrelate_batch(case["y"], context=gpu, **kw)
    two = survey.decorrelate_batch(case["y"], devices=[0, 0], **kw)
    for a, b in zip(one[:2], two[:2]):
        assert a.tobytes() == b.tobytes()
    assert sorted(one[2]) == sorted(two[2]) == ["coef", "coefficients", "mean", "record", "scale", "segments"]
    for k in one[2]:
        assert numpy.asarray(one[2][k]).tobytes() == numpy.asarray(two[2][k]).tobytes(), k
    cases.equal_bits({"flat": one[0], "trend": one[1]}, want("n255_both_dy_5"), ("flat", "trend"))
    # one row, with own [n_own, n]
    flat, fit = survey.decorrelate_batch(case["y"][2], own=case["own"][2], shared=case["shared"], dy_batch=case["dy"][2],
                                         return_fit=True, context=gpu)
    assert flat.tobytes() == one[0][2].tobytes() and fit["record"].shape == (1,) and fit["coef"].tobytes() == one[2]["coef"][2].tobytes()


# ---- as a step of the survey calls ------------------------------------------------------------------------------------------
N_ROLL, ROLL_PERIOD, ROLL_DEPTH = 1440, 3.37, 5e-4
SEARCH = dict(period_min=2.0, period_max=5.0, oversampling_factor=2)


def _roll_batch(n_stars=8):
    """n_stars K2 stars of 1440 points with a 0.05 % transit every 3.37 d: 15 sigma on a flat row, under 3 sigma of the roll's
    own scatter on a raw one."""
    stars = [cases.roll_star(seed, n=N_ROLL, period=ROLL_PERIOD, depth=ROLL_DEPTH) for seed in range(n_stars)]
    return stars[0]["t"], numpy.array([s["flux"] for s in stars]), numpy.array([s["own"] for s in stars]), stars


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_power_batch_detrend(gpu):
    t, raw, own, stars = _roll_batch(3)
    step = survey.Decorrelate(own=own)
    flat = survey.decorrelate_batch(raw, own=own, context=gpu)
    assert numpy.std(flat) < 0.5 * numpy.std(raw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_batch(t, raw, detrend=step, with_arrays=True, context=gpu, **SEARCH)
        expect = survey.power_batch(t, flat, with_arrays=True, context=gpu, **SEARCH)
        _same_summary(got[0], expect[0])
        for a, b in zip(got[1:], expect[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert survey.power_batch(t, raw, context=gpu, **SEARCH)[0]["SDE"].tobytes() != got[0]["SDE"].tobytes()
        # in a tuple with the biweight
        both = (step, survey.Biweight(0.5))
        got = survey.power_batch(t, raw, detrend=both, context=gpu, **SEARCH)
        _same_summary(got[0], survey.power_batch(t, survey.biweight_batch(t, flat, 0.5, context=gpu), context=gpu, **SEARCH)[0])
        # with detrend_mask: the step's mask
        mask = numpy.array([s["in_transit"] for s in stars])
        masked = survey.decorrelate_batch(raw, own=own, mask=mask, context=gpu)
        assert masked.tobytes() != flat.tobytes()
        got = survey.power_batch(t, raw, detrend=step, detrend_mask=mask, context=gpu, **SEARCH)
        _same_summary(got[0], survey.power_batch(t, masked, context=gpu, **SEARCH)[0])
        # weighted with dy_batch
        dy = numpy.full(raw.shape, cases.NOISE) * (1.0 + 0.5 * (numpy.arange(N_ROLL) % 2))
        got = survey.power_batch(t, raw, dy_batch=dy, detrend=step, context=gpu, **SEARCH)
        weighted = survey.decorrelate_batch(raw, own=own, dy_batch=dy, context=gpu)
        _same_summary(got[0], survey.power_batch(t, weighted, dy_batch=dy, context=gpu, **SEARCH)[0])
        # the other survey calls
        assert numpy.asarray(survey.search_batch(t, raw, detrend=step, context=gpu, **SEARCH)[1]).tobytes() == \
            numpy.asarray(survey.search_batch(t, flat, context=gpu, **SEARCH)[1]).tobytes()
        assert survey.lomb_scargle(t, raw, detrend=step, context=gpu)["power"].tobytes() == \
            survey.lomb_scargle(t, flat, context=gpu)["power"].tobytes()
        # the protected form takes the step
        result, info = survey.power_batch_protected(t, raw, step, 7.0, context=gpu, **SEARCH)
        assert info["mask"].shape == raw.shape and info["protected"].shape == (len(raw),)


# sha256 of power_batch's summary on _roll_batch(3)'s raw rows without detrend=, taken from a build of the parent commit (the
# step absent) with tests/decorrelate_cases.py as it is here
PARENT_DIGEST = "68574e57515ae515e0926c9a08c1c3184cbc8c45ac1c38bcfdab1ea2f907f601"


def test_power_batch_without_the_keyword_is_unchanged(gpu):
    t, raw, _, _ = _roll_batch(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        summary = survey.power_batch(t, raw, context=gpu, **SEARCH)[0]
    digest = hashlib.sha256(b"".join(summary[k].tobytes() for k in summary.dtype.names)).hexdigest()
    print("power_batch digest", digest)
    assert digest == PARENT_DIGEST


def test_recovery_on_the_roll(gpu):
    """The injected period is found on the decorrelated rows and on none of the raw ones.  Seeds 0 to 7: on the CPU, the
    statement's flat rows put the chi2 minimum of the oracle's search at 3.369 d for every one of them, and the raw rows give
    the oracle no dip at all (a flat chi2)."""
    t, raw, own, _ = _roll_batch(8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        found = survey.power_batch(t, raw, detrend=survey.Decorrelate(own=own), context=gpu, **SEARCH)[0]["period"]
        blind = survey.power_batch(t, raw, context=gpu, **SEARCH)[0]["period"]
    print("decorrelated:", found, "raw:", blind)
    assert numpy.all(numpy.abs(found / ROLL_PERIOD - 1.0) < 0.01)
    assert not numpy.any(numpy.abs(blind / ROLL_PERIOD - 1.0) < 0.01)
