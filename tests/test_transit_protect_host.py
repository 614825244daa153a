"""Transit-protected detrending without a GPU: the arguments of every new call, the properties of the statement
(tests/transit_protect_spec.py), and the two relations the feature exists for, measured on the statement.

Measured here (run with -s to see them; DESIGN.md "Transit-protected detrending" quotes them).  depth kept: 1 = the whole
transit, as tests/test_prewhiten_host.py measures it.

    pre-whitening, the pulsator of test_prewhiten_host.py (1367 points, three pulsations, a 0.5 % box of 0.12 d every 3.3 d),
    four terms, seeds 0-4: unmasked 0.914 .. 0.937; with the true ephemeris masked (factor 1.5) 0.987 .. 1.011 (the fourth
    term then lands on noise, at 5.4 .. 21.5 cycles a day)
    biweight, BIWEIGHT_CASE below (90 d at 48 points a day, a 1 % rotator of 1.3 d, a 0.5 % box of 0.2 d every 7 d, noise 3e-4,
    a window of 1.5 durations = 0.3 d), seeds 0-2: unmasked 0.235 .. 0.247; with the true ephemeris masked (factor 1.5)
    1.003 .. 1.023, 65 open points a row

Only the relations are asserted: masked keeps a depth closer to 1 (pre-whitening), masked keeps more depth (biweight)."""
import numpy
import pytest

import biweight_spec
import prewhiten_spec
import transit_protect_spec as spec
from test_prewhiten_host import DURATION, PERIOD, depth_kept, pulsator
from tls_amd import _lib, survey


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


# ---- arguments ------------------------------------------------------------------------------------------------------------
T = 1000.0 + numpy.arange(40) / 48.0
Y = numpy.ones((2, 40))
M = numpy.zeros((2, 40), dtype=numpy.uint8)


def test_transit_mask_arguments():
    good = dict(period=[3.0, 2.0], T0=[1000.1, 1000.2], duration=[0.1, 0.1])
    a = _lib.transit_mask_arguments(T, **good)
    assert a["n_curves"] == 2 and a["curve"] is None and a["factor"] == 1.5
    assert _lib.transit_mask_arguments(T, curve=[3, 0], **good)["n_curves"] == 4
    assert _lib.transit_mask_arguments(T, [], [], [])["n_curves"] == 0
    for kw in (dict(factor=0.0), dict(factor=-1.0), dict(factor=numpy.inf), dict(factor=numpy.nan), dict(factor=True),
               dict(curve=[0, 2], n_curves=2), dict(curve=[-1, 0]), dict(curve=[0]), dict(curve=[0.0, 1.0]), dict(n_curves=1),
               dict(n_curves=-1), dict(n_curves=2.5)):
        with pytest.raises(ValueError, match="transit mask"):
            _lib.transit_mask_arguments(T, **dict(good, **kw))
        with pytest.raises(ValueError, match="transit mask"):
            survey.transit_mask(T, **dict(good, **kw))
    for bad_t in (T.reshape(2, 20), numpy.where(numpy.arange(40) == 3, numpy.nan, T), numpy.empty(0)):
        with pytest.raises(ValueError, match="transit mask"):
            survey.transit_mask(bad_t, **good)
    with pytest.raises(ValueError, match="one shape"):
        survey.transit_mask(T, [3.0, 2.0], [1000.1], [0.1, 0.1])
    # a candidate that takes no part is no error
    _lib.transit_mask_arguments(T, [numpy.nan, -1.0], [numpy.inf, 0.0], [0.0, numpy.nan])


def test_mask_arguments_of_the_detrenders():
    for bad in (M.astype(numpy.int64), M.astype(numpy.float64), M[:1], M[:, :39], M.ravel()):
        with pytest.raises(ValueError, match="mask"):
            _lib.biweight_masked_arguments(T, Y, bad, 0.5, 0.5)
        with pytest.raises(ValueError, match="mask"):
            survey.biweight_batch(T, Y, 0.5, mask=bad)
        with pytest.raises(ValueError, match="mask"):
            survey.prewhiten_batch(T, Y, mask=bad)
        for call in (survey.power_batch, survey.search_batch, survey.power_results, survey.lomb_scargle):
            with pytest.raises(ValueError, match="detrend_mask"):
                call(T, Y, detrend=survey.Biweight(0.5), detrend_mask=bad)
    for low in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="min_points"):
            survey.biweight_batch(T, Y, 0.5, mask=M, min_points=low)
    with pytest.raises(ValueError, match="return_status"):
        survey.biweight_batch(T, Y, 0.5, return_status=True)
    with pytest.raises(ValueError, match="window_length"):
        survey.biweight_batch(T, Y, 0.0, mask=M)
    # a bool mask and a [n] mask of one row are taken
    t, rows, mk, wl, bt, low = _lib.biweight_masked_arguments(T, Y[0], M[0] != 0, 0.5, 0.5, 1)
    assert mk.dtype == numpy.uint8 and mk.shape == rows.shape == (1, 40) and low == 1


def test_a_median_filter_takes_no_mask():
    for detrend in (25, (survey.Biweight(0.5), 25), [25, survey.Prewhiten(2)]):
        for call in (survey.power_batch, survey.search_batch, survey.power_results, survey.lomb_scargle):
            with pytest.raises(ValueError, match="median filter"):
                call(T, Y, detrend=detrend, detrend_mask=M)
        with pytest.raises(ValueError, match="median filter"):
            survey.power_batch_protected(T, Y, detrend, 9.0)


def test_power_batch_protected_arguments():
    bw = survey.Biweight(0.5)
    for kw in (dict(factor=0.0), dict(factor=numpy.inf), dict(factor=numpy.nan), dict(n_peaks=0), dict(n_peaks=33),
               dict(n_peaks=1.5), dict(detrend_mask=M)):
        with pytest.raises(ValueError):
            survey.power_batch_protected(T, Y, bw, 9.0, **kw)
    for sde_min in (numpy.nan, None, "9"):
        with pytest.raises(ValueError, match="sde_min"):
            survey.power_batch_protected(T, Y, bw, sde_min)
    with pytest.raises(TypeError):
        survey.power_batch_protected(T, Y, bw)          # (sde_min has no default)


def test_the_new_methods_lie_behind_the_stage_methods():
    """tests/test_stage_memory_host.py demands a case for every public Context method from inject_transits to ephemeris_match;
    the new ones lie behind noise_profile and are run behind poison by tests/test_transit_protect.py."""
    names = [k for k in vars(_lib.Context) if not k.startswith("_")]
    for new in ("transit_mask", "biweight_detrend_masked", "prewhiten_masked"):
        assert names.index(new) > names.index("noise_profile") > names.index("ephemeris_match")
    for entry in ("tls_transit_mask", "tls_biweight_detrend_masked", "tls_prewhiten_masked"):
        assert entry in _lib.SYMBOLS


# ---- the statement: the mask ------------------------------------------------------------------------------------------------
def test_transit_mask_statement():
    t = 2458000.0 + numpy.arange(700) / 48.0
    got = spec.transit_mask(t, [3.3, numpy.nan, 2.0, 0.2, 3.3], [t[0] + 1.0, t[0], t[0], t[0], t[0] + 1.0 - 3.3e4],
                            [0.12, 0.1, 0.0, 0.3, 0.12], curve=[2, 2, 0, 1, 3], n_curves=5)
    phase = ((t - t[0] - 1.0) / 3.3 + 0.5) % 1.0 - 0.5
    assert numpy.array_equal(got[2] != 0, numpy.abs(phase) * 3.3 <= 0.09 + 1e-9)
    assert not got[0].any() and not got[4].any()         # a zero duration is skipped; a curve without a candidate
    assert got[1].all()                                   # factor * duration >= period: everything
    assert abs(int(got[3].sum()) - int(got[2].sum())) <= 2   # T0 1e4 periods earlier: the same transits to rounding
    assert got.dtype == numpy.uint8 and set(numpy.unique(got)) <= {0, 1}


# ---- the statement: the masked biweight ----------------------------------------------------------------------------------------
def _row(n, seed):
    rng = numpy.random.default_rng(seed)
    return 1.0 + 0.01 * numpy.sin(numpy.arange(n) / 7.0) + 3e-4 * rng.standard_normal(n)


def test_an_empty_mask_is_the_unmasked_biweight_and_a_full_one_too():
    t = 1000.0 + numpy.arange(120) / 48.0
    t[70:] += 2.0                                         # two segments
    y = numpy.array([_row(120, 1), _row(120, 2)])
    flat, trend = biweight_spec.detrend(t, y, 0.3, 0.5)
    for fill, status in ((0, 0), (1, 2), (7, 2)):
        got = spec.biweight_masked(t, y, numpy.full(y.shape, fill, dtype=numpy.uint8), 0.3, 0.5)
        assert numpy.array_equal(_bits(got[0]), _bits(flat)) and numpy.array_equal(_bits(got[1]), _bits(trend))
        assert numpy.all(got[2] == status)
    # windows of fewer than min_points points (below one cadence: the point alone) are fitted under an empty mask all the same
    short = biweight_spec.detrend(t, y, 0.005, 0.5)
    for fill, status in ((0, 0), (1, 2)):
        got = spec.biweight_masked(t, y, numpy.full(y.shape, fill, dtype=numpy.uint8), 0.005, 0.5, min_points=3)
        assert numpy.array_equal(_bits(got[0]), _bits(short[0])) and numpy.array_equal(_bits(got[1]), _bits(short[1]))
        assert numpy.all(got[2] == status)
    # a whole segment protected next to an unprotected one: status 2 there, the unmasked bits everywhere
    mask = numpy.zeros(y.shape, dtype=numpy.uint8)
    mask[0, 70:] = 1
    got = spec.biweight_masked(t, y, mask, 0.3, 0.5)
    assert numpy.all(got[2][0, 70:] == 2) and numpy.all(got[2][0, :70] == 0) and numpy.all(got[2][1] == 0)
    assert numpy.array_equal(_bits(got[1]), _bits(trend))


def test_the_interpolation_formula():
    """One-sided and two-sided open runs, the latter across duplicate time stamps.  t[a] == t[b] cannot be reached through the
    call -- points that share a time stamp share their window, so an open point between two fitted ones of its own stamp does
    not exist -- and is held on the formula itself."""
    n = 60
    t = 1000.0 + numpy.arange(n) / 48.0
    t[30:34] = t[29]                                      # duplicate time stamps: 29 .. 33 share one
    y = _row(n, 3)
    wl = 5.5 / 48.0                                       # windows of 5 points (7 at the duplicates: two to the left and the five)
    mask = numpy.zeros(n, dtype=numpy.uint8)
    mask[:9] = 1                                          # a run at the first point: one-sided
    mask[20:38] = 1                                       # a run in the middle, the duplicates inside: two-sided
    mask[50:] = 1                                         # a run at the last point: one-sided
    flat, trend, status = spec.biweight_masked(t, y, mask, wl, 0.5, min_points=3)
    lo, hi = biweight_spec.windows(t, wl, 0.5)
    assert hi[29] - lo[29] == 7 and numpy.all(lo[29:34] == lo[29]) and numpy.all(hi[29:34] == hi[29])
    members = numpy.array([int((mask[a:b] == 0).sum()) for a, b in zip(lo, hi)])
    assert numpy.array_equal(status == 0, members >= numpy.minimum(3, hi - lo))
    for i in numpy.flatnonzero(status == 0):
        assert _bits(trend[i]) == _bits(biweight_spec.location(y[lo[i]:hi[i]][mask[lo[i]:hi[i]] == 0])), i
    fitted = numpy.flatnonzero(status == 0)
    seen = set()
    for i in numpy.flatnonzero(status != 0):
        assert status[i] == 1
        left, right = fitted[fitted < i], fitted[fitted > i]
        if len(left) and len(right):
            a, b = left[-1], right[0]
            want = trend[a] + (trend[b] - trend[a]) * ((t[i] - t[a]) / (t[b] - t[a]))
            seen.add("two-sided")
        else:
            want = trend[left[-1]] if len(left) else trend[right[0]]
            seen.add("left only" if len(left) else "right only")
        assert _bits(trend[i]) == _bits(want), i
    assert seen == {"two-sided", "left only", "right only"}, seen
    assert numpy.all(status[29:34] == 1) and len(set(_bits(trend[29:34]).tolist())) == 1      # one stamp, one trend
    assert numpy.array_equal(_bits(flat), _bits(y / trend))
    # t[a] == t[b]: the trend is ta, not 0 / 0
    assert _bits(spec.interpolate(t, 31, 29, 33, 1.25, 1.5)) == _bits(1.25)
    assert _bits(spec.interpolate(t, 20, 10, 40, 1.25, 1.5)) == _bits(1.25 + (1.5 - 1.25) * ((t[20] - t[10]) / (t[40] - t[10])))
    # min_points 1: only a window without any member is open
    status1 = spec.biweight_masked(t, y, mask, wl, 0.5, min_points=1)[2]
    assert numpy.array_equal(status1 == 0, members >= 1) and (status1 == 1).any() and (status1 == 0).sum() > (status == 0).sum()


# ---- the statement: masked pre-whitening --------------------------------------------------------------------------------------
def test_masked_prewhitening_statement():
    t, y, inside = pulsator(0)
    f = survey.variability_frequencies(t)[::8]
    none = numpy.zeros(len(t), dtype=numpy.uint8)
    plain = prewhiten_spec.prewhiten(t, y, f, n_terms=2)
    empty = spec.prewhiten_masked(t, y, f, none, n_terms=2)
    # an empty mask: W is the sum of n ones, so the weights are 1.0 / n and the run is the unmasked statement's
    assert numpy.array_equal(_bits(empty["weights"]), _bits(numpy.full(len(t), 1.0 / len(t))))
    assert numpy.array_equal(_bits(empty["trend"]), _bits(plain["trend"])) and empty["n_iterations"] == 2
    # fewer than 3 points left: nothing removed, status 2, the mean with the mask ignored
    few = numpy.ones(len(t), dtype=numpy.uint8)
    few[[5, 9]] = 0
    left = spec.prewhiten_masked(t, y, f, few, n_terms=2)
    assert left["status"] == 2.0 and left["n_iterations"] == 0 and not left["terms"]
    assert numpy.array_equal(_bits(left["trend"]), _bits(numpy.full(len(t), plain["mean0"])))
    assert numpy.array_equal(_bits(left["flat"]), _bits(y / plain["mean0"]))
    # a mask: protected points carry no weight, the subtraction reaches them all the same
    run = spec.prewhiten_masked(t, y, f, inside.astype(numpy.uint8), n_terms=2)
    assert numpy.all(run["weights"][inside] == 0.0) and numpy.all(run["weights"][~inside] > 0.0)
    assert numpy.all(run["trend"][inside] != run["mean0"]) and numpy.all(run["r"][inside] != y[inside])


def test_masking_the_transit_keeps_its_depth_through_a_fourth_term():
    """The measured relation (the module's docstring): with the true ephemeris masked, four terms keep a depth closer to 1
    than four terms unmasked, on every seed."""
    for seed in range(5):
        t, y, inside = pulsator(seed)
        f = survey.variability_frequencies(t)
        mask = spec.transit_mask(t, [PERIOD], [t[0] + 1.0], [DURATION], factor=1.5)[0]
        assert numpy.all(mask[inside] == 1)
        unmasked = depth_kept(prewhiten_spec.prewhiten(t, y, f, n_terms=4)["flat"], inside)
        run = spec.prewhiten_masked(t, y, f, mask, n_terms=4)
        masked = depth_kept(run["flat"], inside)
        print("seed %d: depth kept by four terms: unmasked %.3f, masked %.3f (fourth term at %.4f cycles a day)"
              % (seed, unmasked, masked, run["terms"][3][0]["frequency"]))
        assert abs(masked - 1.0) < abs(unmasked - 1.0), (seed, unmasked, masked)


# The biweight case: a rapid rotator needs a window far below three durations.
BIWEIGHT_CASE = dict(days=90.0, per_day=48, noise=3e-4, rotation=(1.3, 0.01), period=7.0, T0=2.1, duration=0.2, depth=5e-3)


def biweight_case(seed, c=BIWEIGHT_CASE):
    rng = numpy.random.default_rng(seed)
    t = 2457000.0 + numpy.arange(int(c["days"] * c["per_day"])) / c["per_day"]
    y = 1.0 + c["rotation"][1] * numpy.sin(2.0 * numpy.pi * ((t - t[0]) / c["rotation"][0] + rng.uniform()))
    phase = ((t - t[0] - c["T0"]) / c["period"] + 0.5) % 1.0 - 0.5
    inside = numpy.abs(phase) * c["period"] <= 0.5 * c["duration"]
    y = y * numpy.where(inside, 1.0 - c["depth"], 1.0)
    return t, y + c["noise"] * rng.standard_normal(len(t)), inside


def test_masking_the_transit_keeps_its_depth_under_a_short_biweight_window():
    """The measured relation (the module's docstring): a biweight window of 1.5 durations eats the transit; with the true
    ephemeris masked it keeps more depth, on every seed."""
    c = BIWEIGHT_CASE
    for seed in range(3):
        t, y, inside = biweight_case(seed)
        assert len(t) == 4320
        mask = spec.transit_mask(t, [c["period"]], [t[0] + c["T0"]], [c["duration"]], factor=1.5)[0]
        assert numpy.all(mask[inside] == 1)
        window = 1.5 * c["duration"]
        unmasked = biweight_spec.detrend(t, y, window, 0.5)[0]
        masked, _, status = spec.biweight_masked(t, y, mask, window, 0.5)
        kept = [(1.0 - flat[inside].mean() / flat[~inside].mean()) / c["depth"] for flat in (unmasked, masked)]
        print("seed %d: depth kept by a biweight of 1.5 durations: unmasked %.3f, masked %.3f (%d open points)"
              % (seed, kept[0], kept[1], int((status != 0).sum())))
        assert (status[inside] == 1).any() and not (status[~mask.astype(bool)] != 0).any() and not (status == 2).any()
        assert kept[1] > kept[0], (seed, kept)
