"""The noise profile without a GPU: the statement (tests/noise_profile_spec.py) on light curves whose noise is known, the
host layer of survey.noise_profile (the default widths, every ValueError, the peak fields of power_batch(noise=True)) and the
places where the limits and the kernel's invariants are written down.

The light curves: 1920 points at 48 a day with a 3 d gap in the middle, white noise of 3e-4.  The bands below are those of
the estimators, not of one run: a MAD over N windows of w samples rests on about N / w independent values, so its relative
scatter is about 1 / sqrt(0.74 N / w) -- 3 % at w = 1, 6 % at w = 3, 8 % at w = 6 and 12 % at w = 13 for N = 1900 -- and a
band holds three of those on either side of the expected value (seeds 0 to 4 lie within one and a half)."""
import os
import re

import numpy
import pytest

import gls_spec
import noise_profile_spec as spec
from tls_amd import _lib, survey

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1920
T = numpy.arange(N) / 48.0
T[N // 2:] += 3.0
W = [1, 3, 6, 13]
SIGMA = 3e-4


def white(seed):
    return 1.0 + numpy.random.RandomState(seed).normal(0, SIGMA, N)


def red(seed):
    """White noise plus an AR(1) process, phi 0.95, innovations 1e-4."""
    rng = numpy.random.RandomState(seed)
    w, e, a = rng.normal(0, SIGMA, N), rng.normal(0, 1e-4, N), numpy.zeros(N)
    for i in range(1, N):
        a[i] = 0.95 * a[i - 1] + e[i]
    return 1.0 + w + a


def boxes(seed, depth):
    """White noise with a box of 6 samples every 2.1 d (21 epochs, one of them in the gap: 20 boxes): (y, the samples
    inside)."""
    y, inside = white(seed), numpy.zeros(N, dtype=bool)
    for k in range(21):
        epoch = T[0] + 0.5 + 2.1 * k
        i = numpy.searchsorted(T, epoch)
        if T[i] - epoch < 1 / 48.0:
            inside[i:i + 6] = True
    y[inside] -= depth
    return y, inside


# ---- the statement on known noise -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_white_noise_has_beta_one(seed):
    p = spec.noise_profile(white(seed), W, T)
    # a window across the gap is dropped: n - w + 1 windows, less the w - 1 that straddle it
    assert p["count"].tolist() == [N, N - 3 + 1 - 2, N - 6 + 1 - 5, N - 13 + 1 - 12] == [1920, 1916, 1910, 1896]
    assert p["curve"]["status"] == 0 and p["curve"]["n_clipped"] <= 2 and p["curve"]["n_pairs"] >= N - 2 - 4
    assert p["beta"][0] == 1.0                                          # (w = 1: v = d, mu = 0, robust = sigma)
    for k, band in ((1, 0.18), (2, 0.24), (3, 0.36)):
        assert 1.0 - band < p["beta"][k] < 1.0 + band, (k, p["beta"])
    assert 0.9 * SIGMA < p["curve"]["sigma"] < 1.1 * SIGMA and 0.9 * SIGMA < p["curve"]["sigma_p2p"] < 1.1 * SIGMA
    assert numpy.all(numpy.abs(p["rms"] * numpy.sqrt(W) / SIGMA - 1.0) < 0.2)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_red_noise_grows_with_the_width(seed):
    """AR(1) with phi 0.95 and innovations 1e-4 has a stationary sigma of 3.2e-4: the means of w samples keep most of it
    while the white part falls as 1 / sqrt(w), so robust_w sqrt(w) / robust_1 is expected at 1.42, 1.86 and 2.55."""
    r = spec.noise_profile(red(seed), W, T)["robust"]
    ratio = r * numpy.sqrt(W) / r[0]
    for k, expected, band in ((1, 1.42, 0.18), (2, 1.86, 0.24), (3, 2.55, 0.36)):
        assert expected * (1.0 - band) < ratio[k] < expected * (1.0 + band), (k, ratio)
    assert ratio[1] > 1.2 and ratio[2] > 1.5 and ratio[3] > 1.9         # (white noise stays below 1.18, 1.24 and 1.36)


@pytest.mark.parametrize("seed", (0, 1, 2, 3, 4))
def test_a_shallow_transit_inflates_the_rms_not_the_robust_value(seed):
    """A 0.1 % box (3.3 sigma a point: not clipped) of 6 samples every 2.1 d: 20 of the 1910 windows of 6 samples hold the
    whole box and 200 a part of it, so the rms at w = 6 rises by sqrt(1 + 2.3) while the median absolute deviation moves by a
    few per cent."""
    y, inside = boxes(seed, 1e-3)
    assert inside.sum() == 120
    p = spec.noise_profile(y, W, T)
    assert p["curve"]["n_clipped"] <= 8
    rms, robust = p["rms"][2] * numpy.sqrt(6.0) / SIGMA, p["robust"][2] * numpy.sqrt(6.0) / SIGMA
    assert 1.6 < rms < 2.05, rms
    assert 0.85 < robust < 1.3, robust
    assert robust < 0.72 * rms


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_a_deep_transit_is_clipped_whole(seed):
    """A 1 % box is 33 sigma deep: every one of its 120 points is clipped, no window holds one, and what is left is white."""
    y, inside = boxes(seed, 1e-2)
    record, d, keep = spec.curve_part(y, T, spec.span_limits(T, W)[1], 5.0, 5.0)
    assert not keep[inside].any() and 120 <= record["n_clipped"] <= 122
    p = spec.noise_profile(y, W, T)
    assert p["count"][0] == N - record["n_clipped"] and p["count"][2] < 1910 - 20 * 11 + 20
    assert 0.76 < p["beta"][2] < 1.24
    unclipped = spec.noise_profile(y, W, T, clip_lower=numpy.inf)
    assert unclipped["curve"]["n_clipped"] <= 2 and unclipped["rms"][2] > 3 * p["rms"][2]


def test_the_statement_in_small():
    """Medians of odd and even counts, the direct sums, a constant row, -0.0, and the ordered sum it imports."""
    assert spec.lanes_sum is gls_spec.lanes_sum
    assert spec.median([3.0, 1.0, 2.0]) == 2.0 and spec.median([4.0, 1.0, 2.0, 3.0]) == 2.5 and spec.median([7.0]) == 7.0
    d = numpy.array([1e16, 1.0, -1e16, 1.0])
    assert spec.window_means(d, 3).tolist() == [0.0, (1.0 - 1e16 + 1.0) / 3.0] and spec.window_means(d, 4)[0] == 0.25
    p = spec.noise_profile(numpy.full(30, 0.5), [1, 2])
    assert p["curve"]["status"] == 1 and p["curve"]["n_clipped"] == 0 and numpy.isnan(p["curve"]["sigma_p2p"])
    assert p["curve"]["sigma"] == 0.0 and p["curve"]["median"] == 0.5
    assert p["count"].tolist() == [0, 0] and numpy.isnan(p["robust"]).all() and numpy.isnan(p["rms"]).all() and numpy.isnan(p["beta"]).all()
    # more than half of the row on one value: the MAD is 0 although the row is not constant
    assert spec.noise_profile([1.0, 1.0, 1.0, 2.0, 0.0], [1])["curve"]["status"] == 1
    zero = spec.noise_profile([0.0, -0.0, 1.0, -1.0, 2.0], [1, 2], clip_upper=numpy.inf, clip_lower=numpy.inf, min_count=1)
    assert not numpy.signbit(zero["curve"]["median"]) and zero["count"].tolist() == [5, 4]
    # one clip switched off, and a clip of 0
    y = numpy.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 60.0, -60.0, 2.5])
    assert spec.noise_profile(y, [1])["curve"]["n_clipped"] == 2
    assert spec.noise_profile(y, [1], clip_upper=numpy.inf)["curve"]["n_clipped"] == 1
    assert spec.noise_profile(y, [1], clip_upper=0.0, clip_lower=numpy.inf)["curve"]["n_clipped"] == 4
    # without t no window is across a gap
    assert spec.noise_profile(white(0), W)["count"].tolist() == [N, N - 2, N - 5, N - 12]
    # min_count
    short = spec.noise_profile(white(0)[:8], [6, 7, 8], min_count=3)
    assert short["count"].tolist() == [3, 2, 1] and numpy.isnan(short["robust"]).tolist() == [False, True, True]


# ---- the host layer -----------------------------------------------------------------------------------------------------------
def test_default_widths():
    assert survey.KEPLER_PULSE_HOURS == (1.5, 2.0, 2.5, 3.0, 3.5, 4.5, 5.0, 6.0, 7.5, 9.0, 10.5, 12.0, 12.5, 15.0)
    half_hour = survey.noise_widths(numpy.arange(4320) / 48.0)
    assert half_hour.dtype == numpy.int64 and half_hour.tolist() == [1, 3, 4, 5, 6, 7, 9, 10, 12, 15, 18, 21, 24, 25, 30]
    two_minutes = survey.noise_widths(numpy.arange(19440) / 720.0)
    assert two_minutes.tolist() == [1, 45, 60, 75, 90, 105, 135, 150, 180, 225, 270, 315, 360, 375, 450]
    assert survey.noise_widths(T).tolist() == half_hour.tolist()          # (the gap does not move the median cadence)
    assert survey.noise_widths(numpy.arange(20) / 48.0).tolist() == [1, 3, 4, 5, 6, 7, 9, 10, 12, 15, 18]   # (cut at n)
    assert survey.noise_widths(numpy.arange(10 ** 4) / 86400.0, hours=[0.5, 2.0]).tolist() == [1, 1800]      # (cut at the cap)
    assert survey.noise_widths(numpy.arange(50.0), hours=[1.0]).tolist() == [1]                             # (below a sample: 1)
    for bad in (numpy.arange(2.0), [0.0, 1.0, numpy.nan], [2.0, 1.0, 3.0], numpy.zeros(5), numpy.zeros((3, 3))):
        with pytest.raises(ValueError):
            survey.noise_widths(bad)
    with pytest.raises(ValueError):
        survey.noise_widths(T, hours=[1.0, -2.0])


def test_span_limits_are_the_statement_s():
    for gap in (0.0, 0.5, 1.25):
        got, pair = survey._noise_spans(T, [1, 3, 30, 4096], gap)
        want, want_pair = spec.span_limits(T, [1, 3, 30, 4096], gap)
        assert got.tobytes() == want.tobytes() and numpy.float64(pair).tobytes() == numpy.float64(want_pair).tobytes()
    got, pair = survey._noise_spans(None, [1, 2], 0.5)
    assert numpy.isinf(got).all() and got.shape == (2,) and numpy.isinf(pair)


BAD_CALLS = {
    "nan in the flux": dict(flux=numpy.where(numpy.arange(N) == 7, numpy.nan, 1.0)),
    "inf in the flux": dict(flux=numpy.where(numpy.arange(N) == 7, numpy.inf, 1.0)),
    "nan in t": dict(t=numpy.where(numpy.arange(N) == 7, numpy.nan, T)),
    "t not ascending": dict(t=T[::-1]),
    "n < 3": dict(flux=numpy.ones(2), t=numpy.arange(2.0), widths=[1]),
    "n < 3 without t": dict(flux=numpy.ones((4, 2)), t=None, widths=[1]),
    "widths not integers": dict(widths=[1.5, 3]),
    "widths are text": dict(widths=["a"]),
    "widths not ascending": dict(widths=[3, 2]),
    "widths repeat": dict(widths=[2, 2]),
    "width below 1": dict(widths=[0, 2]),
    "width above n": dict(flux=numpy.ones(10), t=numpy.arange(10.0), widths=[1, 11]),
    "width above the cap": dict(flux=numpy.ones(5000), t=numpy.arange(5000.0), widths=[_lib.NOISE_MAX_WIDTH + 1]),
    "too many widths": dict(widths=list(range(1, _lib.NOISE_MAX_WIDTHS + 2))),
    "no widths": dict(widths=[]),
    "negative clip": dict(clip_upper=-1.0),
    "nan clip": dict(clip_lower=numpy.nan),
    "clip is text": dict(clip_lower="5"),
    "min_count 0": dict(min_count=0),
    "min_count a fraction": dict(min_count=2.5),
    "negative gap_tolerance": dict(gap_tolerance=-0.5),
    "widths=None without t": dict(t=None, widths=None),
    "shapes disagree": dict(flux=numpy.ones((2, N - 1))),
    "three axes": dict(flux=numpy.ones((2, 2, N))),
    "t with two axes": dict(t=numpy.ones((2, N)), widths=[1]),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_bad_arguments_raise_before_any_device_work(name):
    """Every ValueError comes before a context exists: context=object() is never touched."""
    kw = dict(dict(flux=white(0), t=T, widths=W), **BAD_CALLS[name])
    flux = kw.pop("flux")
    with pytest.raises(ValueError):
        survey.noise_profile(flux, context=object(), detrend=25, **kw)


def test_the_arguments_a_good_call_hands_over():
    span_max, pair_span = survey._noise_spans(T, W, 0.5)
    a = _lib.noise_arguments(T, white(1), numpy.array(W, dtype=float), span_max, pair_span, numpy.inf, 0.0, 1)
    assert a["y"].shape == (1, N) and a["widths"].dtype == numpy.int64 and a["widths"].tolist() == W
    assert a["clip_upper"] == numpy.inf and a["clip_lower"] == 0.0 and a["min_count"] == 1
    assert _lib.noise_arguments(None, numpy.ones((2, 3)), [3], [numpy.inf], numpy.inf)["t"] is None
    assert survey.noise_curve_fields() == spec.CURVE_FIELDS == _lib.NOISE_CURVE_DTYPE.names


def test_noise_needs_peak_fits_and_good_widths():
    flux = numpy.array([white(0), white(1)])
    with pytest.raises(ValueError, match="peak_fits"):
        survey.power_batch(T, flux, peaks=4, noise=True, context=object())
    with pytest.raises(ValueError):
        survey.power_batch(T, flux, peaks=4, peak_fits=True, noise=[3, 2], context=object())
    with pytest.raises(ValueError):
        survey.power_batch(T, flux, peaks=4, peak_fits=True, noise=[N + 1], context=object())
    assert survey._noise_request(None, True, T) is None and survey._noise_request(False, False, T) is None
    request = survey._noise_request(True, True, T)
    assert request["widths"].tolist() == survey.noise_widths(T).tolist() and request["cadence"] == numpy.median(numpy.diff(T))
    assert request["span_max"].tobytes() == spec.span_limits(T, request["widths"])[0].tobytes()
    assert survey._noise_request([2, 9], True, T)["widths"].tolist() == [2, 9]


def test_the_peak_fields():
    """noise_width is the profile width nearest duration_days / cadence, the smaller one on a tie; the fields are NaN and -1
    where status != 0 or the profile has no value."""
    widths = numpy.array([1, 3, 4, 6, 30], dtype=numpy.int64)
    cadence = 1 / 48.0
    days = numpy.array([3.5, 3.49, 3.51, 5.0, 0.2, 100.0, 2.0, numpy.nan, 18.0]) * cadence
    assert survey.noise_width_index(days, cadence, widths).tolist() == [1, 1, 2, 2, 0, 4, 0, -1, 3]
    records = numpy.zeros((2, 3), dtype=[("status", "f8"), ("duration_days", "f8"), ("depth_mean", "f8"), ("transit_count", "f8")])
    records["status"] = [[0, 0, 1], [0, 2, 0]]
    records["duration_days"] = numpy.array([[3.5, 29.0, 3.0], [5.0, 4.0, 6.2]]) * cadence
    records["depth_mean"] = [[1e-3, 2e-3, 3e-3], [4e-3, 5e-3, 6e-3]]
    records["transit_count"] = [[4, 9, 1], [16, 2, 25]]
    robust = numpy.array([[1e-4, 2e-4, 3e-4, 4e-4, numpy.nan], [5e-4, 6e-4, 7e-4, 8e-4, 9e-4]])
    out = survey._with_noise(records, dict(widths=widths, robust=robust), cadence)
    assert out.dtype.names == records.dtype.names + ("noise_width", "noise_sigma", "noise_mes")
    for k in records.dtype.names:
        assert out[k].tobytes() == records[k].tobytes()
    numpy.testing.assert_array_equal(out["noise_width"], [[3, -1, -1], [4, -1, 6]])
    numpy.testing.assert_array_equal(out["noise_sigma"], [[2e-4, numpy.nan, numpy.nan], [7e-4, numpy.nan, 8e-4]])
    want = [[1e-3 * numpy.sqrt(4.0) / 2e-4, numpy.nan, numpy.nan], [4e-3 * numpy.sqrt(16.0) / 7e-4, numpy.nan, 6e-3 * numpy.sqrt(25.0) / 8e-4]]
    numpy.testing.assert_array_equal(out["noise_mes"], want)


# ---- where the limits and the invariants are written down ---------------------------------------------------------------------
def test_limits_are_mirrored():
    header = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_noise.hip.h")).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)" % name, header).group(1))

    def constant(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, kernel).group(1))

    assert define("TLS_NOISE_MAX_WIDTH") == constant("kNoiseMaxWidth") == _lib.NOISE_MAX_WIDTH == 4096
    assert define("TLS_NOISE_MAX_WIDTHS") == constant("kNoiseMaxWidths") == _lib.NOISE_MAX_WIDTHS == 64
    assert define("TLS_NOISE_LDS_POINTS") == constant("kNoiseLdsPoints") == _lib.NOISE_LDS_POINTS
    assert define("TLS_NOISE_MAX_POINTS") == _lib.NOISE_MAX_POINTS
    assert constant("kNoiseThreads") == _lib.NOISE_THREADS == gls_spec.LANES
    assert _lib.NOISE_LDS_POINTS >= 4320                                  # (a k2_90d row is measured in the LDS)
    assert 16 * _lib.NOISE_LDS_POINTS + _lib.NOISE_LDS_POINTS // 8 + 4096 <= 160 * 1024
    assert "%.16f" % spec.K in kernel and "%.16f" % spec.ROOT2 in kernel
    assert "(8: tls_noise_profile)" in header and define("TLS_AMD_ABI_VERSION") == 8


def test_the_kernels_keep_their_invariants():
    """Contraction off, the stage's own check code, integer atomics only, and the stage behind ephemeris_match."""
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_noise.hip.h")).read()
    code = re.sub(r"//[^\n]*", "", kernel)
    assert code.count("#pragma clang fp contract(off)") >= 4 and "kChkNoise" in code
    assert "kChkNoise = 16" in open(os.path.join(REPO, "tls_amd", "csrc", "tls_kernels.hip.h")).read()
    atomics = re.findall(r"atomic\w+\(&sh->(\w+)", code)
    assert atomics and set(atomics) <= {"hist", "cnt", "word"}            # (the integer members of NoiseShared)
    assert len(re.findall(r"\batomic\w+\(", code)) == len(atomics)
    assert re.search(r"unsigned int hist\[", code) and re.search(r"unsigned int cnt\[", code) and re.search(r"unsigned long long word\[", code)
    methods = [k for k in vars(_lib.Context) if not k.startswith("_")]
    assert methods.index("noise_profile") > methods.index("ephemeris_match")
    assert not [k for k in methods if k.startswith("power_batch") and "noise" in k]
