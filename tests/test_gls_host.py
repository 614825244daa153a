"""The variability periodogram and the sine test without a GPU: the statement (tests/gls_spec.py) against
scipy.signal.lombscargle, on an injected sinusoid and on noise; the sine test on a planet and on a contact binary; the
default frequency grid; the argument checks of the Python layer, all raised before any device work; and the header, the
binding and the version comment name the three entries."""
import ctypes
import math
import os
import re
import warnings

import numpy
import pytest
from scipy.signal import lombscargle

import gls_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, transit_model

T = 1.0 + numpy.arange(300) / 64.0


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


def gapped(seed, period=3.7, amplitude=2e-3):
    """40 d at 48 a day less a gap of 2.5 d: noise of 3e-4 with per-point errors, and a sinusoid."""
    rng = numpy.random.RandomState(seed)
    t = numpy.delete(2.0 + numpy.arange(1920) / 48.0, numpy.r_[700:820])
    dy = 3e-4 * (1.0 + 0.5 * rng.uniform(size=len(t)))
    y = 1.0 + rng.normal(0, 1.0, len(t)) * dy + amplitude * numpy.sin(2 * numpy.pi * t / period + 0.4)
    return t, y, dy


# ---- the statement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
def test_the_statement_against_scipy(weighted):
    """The statement's power against scipy's floating-mean, normalised periodogram: they differ by scipy's own cancellation
    at y ~ 1 (it does not centre y): 1.6e-10 with weights and 1.7e-11 without on this curve, below 1e-8."""
    t, y, dy = gapped(0)
    f = survey.variability_frequencies(t, oversampling=2, f_max=12.0)
    mine = spec.lomb_scargle(t, y, f, dy if weighted else None)["power"]
    kw = dict(weights=1 / dy ** 2) if weighted else {}
    theirs = lombscargle(t, y, 2 * numpy.pi * f, normalize=True, floating_mean=True, **kw)
    worst = numpy.abs(mine - theirs).max()
    print("max|statement - scipy| = %.3g" % worst)
    assert worst < 1e-8


def test_an_injected_sinusoid_is_recovered_and_noise_has_no_such_power():
    t, y, dy = gapped(1)
    f = survey.variability_frequencies(t)
    assert len(f) == 4797 == int(24 * 5 * (t[-1] - t[0]))           # (k / (5 T) up to 24 a day, half the median cadence's rate)
    f = f[:600]                                      # (up to 3 a day: the statement is slow)
    got = spec.lomb_scargle(t, y, f, dy)
    best = int(numpy.nanargmax(got["power"]))
    assert abs(f[best] - 1 / 3.7) <= f[1] - f[0]
    assert abs(got["amplitude"][best] - 2e-3) < 0.05 * 2e-3
    assert got["power"][best] > 0.9
    # the phase is that of the sinusoid at t_0, in cycles: y = mean + A cos(2 pi (f (t - t_0) - phase))
    model = got["mean"] + got["amplitude"][best] * numpy.cos(2 * numpy.pi * (f[best] * (t - t[0]) - got["phase"][best]))
    assert numpy.std(y - model) < 1.1 * numpy.sqrt(numpy.mean(dy ** 2))      # (the noise is left; the sinusoid's rms is 1.4e-3)
    _, noise, _ = gapped(1, amplitude=0.0)
    quiet = spec.lomb_scargle(t, noise, f, dy)
    assert numpy.nanmax(quiet["power"]) < 0.05 < got["power"][best]


def test_epilogue_refuses_with_nan():
    power, amplitude, phase = spec.epilogue([1e-3, 1e-3, 1e-3], [0.0] * 3, [1.0, 0.1, 0.1], [0.0] * 3, [1.0, 0.2, 0.2], [0.0] * 3,
                                            [1.0, 1.0, 0.0])
    assert numpy.isnan(power).tolist() == [True, False, True] and numpy.isnan(amplitude).tolist() == [True, False, True]
    w, a, ybar, YY = spec.prologue(numpy.full(7, 0.75))
    assert YY == 0.0 and (a == 0.0).all() and ybar == 0.75 or abs(ybar - 0.75) < 1e-15


def test_the_ordered_sum_of_the_sine_test():
    """Lane j = i mod 256 adds its terms over i ascending from 0.0, the lanes are added in lane order."""
    rng = numpy.random.RandomState(3)
    v = rng.normal(0, 1, 700)
    used = rng.uniform(size=700) > 0.2
    lanes = []
    for j in range(256):
        s = 0.0
        for i in range(j, 700, 256):
            s = s + (v[i] if used[i] else 0.0)
        lanes.append(s)
    total = lanes[0]
    for j in range(1, 256):
        total = total + lanes[j]
    assert spec.lanes_sum(v, used) == total
    assert abs(total - math.fsum(v[used])) < 1e-12 and spec.LANES == _lib.SINE_LANES == 256


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_sine_test_separates_a_planet_from_a_contact_binary(seed):
    """A planet of rp 0.07 at 3.7 d against a contact binary of the same depth (a sinusoid at P / 2 whose minima are the
    'transits'), transits masked 1.5 durations wide, noise 3e-4: the largest significance over P / 2, P and 2 P is 1.6, 1.2,
    2.5, 1.8, 1.4 for the planet and 242, 234, 239, 233, 246 for the binary (seeds 0 to 4).  No threshold is fixed."""
    rng = numpy.random.RandomState(seed)
    t = numpy.delete(2.0 + numpy.arange(1920) / 48.0, numpy.r_[700:820])
    noise = rng.normal(0, 3e-4, len(t))
    P, T0 = 3.7, t[0] + 1.3
    planet = transit_model.light_curve(t, T0, P, 0.07, 10.0, 89.5, 0, 90, [0.4, 0.3], "quadratic") + noise
    binary = 1 - 0.5 * 0.07 ** 2 * (1 + numpy.cos(2 * numpy.pi * (t - T0) / (P / 2))) + noise
    largest = []
    for y in (planet, binary):
        s = spec.sine_test(t, y, P, None, T0, 0.15)
        assert s["status"] == 0 and s["n_used"] == 1691
        largest.append(numpy.max(spec.sine_harmonics(s["exact"], s["variance"], s["n_used"])[4]))
    print("largest significance: planet %.1f, contact binary %.1f" % tuple(largest))
    assert largest[1] > 20 * largest[0]


def test_sine_test_statement_statuses():
    t, y, dy = gapped(2)
    for bad in (dict(P=numpy.nan), dict(P=0.0), dict(P=-1.0), dict(P=numpy.inf), dict(T0=numpy.nan, d=0.1), dict(T0=3.0, d=0.0),
                dict(T0=3.0, d=numpy.inf)):
        assert spec.sine_test(t, y, **dict(dict(P=3.7), **bad))["status"] == 1
    few = spec.sine_test(t[:40], y[:40], 1024.0, None, t[0], (36.5 / 48) / 0.75)
    assert few["status"] == 2 and few["n_used"] == 3
    four = spec.sine_test(t[:40], y[:40], 1024.0, None, t[0], (35.5 / 48) / 0.75)
    assert four["status"] == 0 and four["n_used"] == 4
    s = spec.sine_test(t, y, 3.7, dy)
    assert s["n_used"] == len(t) and abs(s["mean"] - spec.prologue(y, dy)[2]) < 1e-15


# ---- the frequency grid ------------------------------------------------------------------------------------------------------
def test_variability_frequencies():
    t = numpy.arange(100) / 10.0                     # T = 9.9 d at 10 a day: Nyquist 5 a day
    f = survey.variability_frequencies(t)
    step = 1.0 / (5 * 9.9)
    assert len(f) == int(5.0 / step) == 247 and f[0] == step and numpy.allclose(f, numpy.arange(1, 248) * step, rtol=1e-15)
    assert f[-1] <= 5.0 < f[-1] + step
    g = survey.variability_frequencies(t, oversampling=2, f_max=1.0)
    assert len(g) == 19 and g[0] == 1.0 / (2 * 9.9) and g[-1] <= 1.0
    uneven = numpy.delete(t, numpy.r_[30:50])
    assert survey.variability_frequencies(uneven)[-1] <= 5.0      # (the median cadence, not the gap)
    for bad in (dict(t=t[::-1]), dict(t=[1.0]), dict(t=[1.0, 1.0]), dict(t=[0.0, numpy.nan, 1.0]), dict(t=t[None, :]),
                dict(oversampling=0), dict(oversampling=numpy.inf), dict(oversampling=True), dict(f_max=0.0),
                dict(f_max=numpy.nan), dict(f_max=1e-3), dict(f_max="1")):
        with pytest.raises(ValueError, match="periodogram"):
            survey.variability_frequencies(**dict(dict(t=t), **bad))


# ---- the Python layer --------------------------------------------------------------------------------------------------------
FLUX = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
BAD_T = numpy.where(numpy.arange(300) == 7, numpy.nan, T)
BAD_PERIODOGRAM = [
    (dict(t=T[::-1]), "ascending"), (dict(t=BAD_T), "ascending"), (dict(t=T[:-1]), "over the time stamps"),
    (dict(t=T[None, :]), "periodogram"), (dict(t=T[:2], flux_batch=FLUX[:, :2], frequencies=[1.0]), r"n in \[3"),
    (dict(flux_batch=numpy.where(numpy.arange(300) == 9, numpy.inf, FLUX)), "NaN or an infinite"),
    (dict(flux_batch=FLUX[None]), "over the time stamps"), (dict(flux_batch="x"), "numbers"),
    (dict(dy_batch=numpy.zeros((2, 300))), "dy has"), (dict(dy_batch=numpy.full((2, 300), numpy.nan)), "dy has"),
    (dict(dy_batch=numpy.ones((3, 300))), "over the time stamps"), (dict(dy_batch=numpy.ones(300)), "over the time stamps"),
    (dict(frequencies=[1.0, 0.0]), "frequency"), (dict(frequencies=[1.0, -2.0]), "frequency"),
    (dict(frequencies=[numpy.nan]), "frequency"), (dict(frequencies=[numpy.inf]), "frequency"), (dict(frequencies=[]), "frequencies"),
    (dict(frequencies=[[1.0, 2.0]]), "frequencies"), (dict(frequencies="f"), "numbers"),
    (dict(peaks=0), "peaks"), (dict(peaks=33), "peaks"), (dict(peaks=2.5), "peaks"), (dict(peaks=3, peak_separation=1.0), "separation")]


@pytest.mark.parametrize("kw, match", BAD_PERIODOGRAM)
def test_lomb_scargle_refuses_before_any_device_work(no_device, kw, match):
    args = dict(dict(t=T, flux_batch=FLUX, frequencies=[0.5, 1.0]), **kw)
    with pytest.raises(ValueError, match=match):
        survey.lomb_scargle(**args)
    with pytest.raises(ValueError, match=match):                  # (nor is anything detrended first)
        survey.lomb_scargle(detrend=25, **args)


def test_lomb_scargle_reaches_the_device(no_device):
    for kw in (dict(), dict(frequencies=[2.0, 0.5, 0.5]), dict(dy_batch=numpy.ones((2, 300)), peaks=4), dict(flux_batch=FLUX[0])):
        with pytest.raises(AssertionError, match="a context was created"):
            survey.lomb_scargle(**dict(dict(t=T, flux_batch=FLUX), **kw))


BAD_SINE = [
    (dict(t=T[::-1]), "ascending"), (dict(t=BAD_T), "ascending"), (dict(t=T[:-1]), "over the time stamps"),
    (dict(flux_batch=numpy.where(numpy.arange(300) == 9, numpy.nan, FLUX)), "NaN or an infinite"),
    (dict(dy_batch=numpy.zeros((2, 300))), "dy has"), (dict(dy_batch=numpy.ones((1, 300))), "over the time stamps"),
    (dict(period=[1.0]), "one candidate a light curve"), (dict(period=[[1.0, 1.5]]), "n_fits"), (dict(period=["a", "b"]), "numbers"),
    (dict(T0=[1.2, 1.3]), "come together"), (dict(duration=[0.1, 0.1]), "come together"),
    (dict(T0=[1.2], duration=[0.1, 0.1]), "n_fits"), (dict(curve=[0, 2]), "curve"), (dict(curve=[0.0, 1.0]), "curve"),
    (dict(curve=[0]), "curve"), (dict(curve=[-1, 0]), "curve"),
    (dict(mask=-0.5), "mask"), (dict(mask=numpy.nan), "mask"), (dict(mask=numpy.inf), "mask"), (dict(mask="1"), "mask"),
    (dict(mask=True), "mask"), (dict(harmonics=[]), "harmonics"), (dict(harmonics=[1.0, 0.0]), "harmonics"),
    (dict(harmonics=[numpy.nan]), "harmonics"), (dict(harmonics=numpy.arange(1, 10)), "harmonics"), (dict(harmonics=[[1.0]]), "harmonics")]


@pytest.mark.parametrize("kw, match", BAD_SINE)
def test_sine_test_refuses_before_any_device_work(no_device, kw, match):
    args = dict(dict(t=T, flux_batch=FLUX, period=[1.0, 1.5]), **kw)
    with pytest.raises(ValueError, match=match):
        survey.sine_test(**args)
    with pytest.raises(ValueError, match=match):
        survey.sine_test(detrend=25, **args)


def test_sine_test_reaches_the_device(no_device):
    for kw in (dict(), dict(period=[numpy.nan, -1.0]), dict(T0=[1.2, numpy.nan], duration=[0.1, -1.0]), dict(mask=0.0),
               dict(curve=[1, 1], harmonics=[1.0])):
        with pytest.raises(AssertionError, match="a context was created"):
            survey.sine_test(**dict(dict(t=T, flux_batch=FLUX, period=[1.0, 1.5]), **kw))


@pytest.mark.parametrize("kw, match", [
    (dict(sine_test=True), "needs peak_fits"), (dict(sine_test=True, peaks=3), "needs peak_fits"),
    (dict(sine_test=True, peaks=3, peak_fits=True, sine_test_mask=-1.0), "mask"),
    (dict(sine_test=True, peaks=3, peak_fits=True, sine_test_mask=numpy.nan), "mask"),
    (dict(sine_test=True, peaks=3, peak_fits=True, sine_test_harmonics=[0.0]), "harmonics"),
    (dict(sine_test=True, peaks=3, peak_fits=True, sine_test_harmonics=[]), "harmonics")])
def test_power_batch_refuses_before_any_device_work(no_device, kw, match):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, FLUX, **kw)
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, FLUX, detrend=25, **kw)


def test_arguments_pack():
    a = _lib.lomb_scargle_arguments(T, FLUX[0], None, [2.0, 1.0], peaks=3)
    assert a["y"].shape == (1, 300) and a["dy"] is None and a["k"] == 3 and a["separation"] == 0.02
    assert a["frequencies"].tolist() == [2.0, 1.0] and a["t"].flags.c_contiguous
    a = _lib.lomb_scargle_arguments(T, FLUX, numpy.ones((2, 300)), 1.5)
    assert a["k"] == 0 and a["dy"].shape == (2, 300) and a["frequencies"].shape == (1,)
    s = _lib.sine_test_arguments(T, FLUX, None, [1.0, 2.0], None, None, None, 1.5, (0.5, 1.0, 2.0))
    assert s["curve"].tolist() == [0, 1] and s["curve"].dtype == numpy.int64 and s["T0"] is None and s["duration"] is None
    assert s["harmonics"].tolist() == [0.5, 1.0, 2.0] and s["mask"] == 1.5
    s = _lib.sine_test_arguments(T, FLUX[1], numpy.ones(300), 1.0, 1.2, 0.1, [0], 0, [1.0])
    assert s["y"].shape == s["dy"].shape == (1, 300) and s["T0"].tolist() == [1.2] and s["mask"] == 0.0


def test_field_lists():
    names = survey.sine_test_fields()
    assert names == ("sine_status", "sine_n_used", "sine_mean", "sine_variance", "sine_power", "sine_amplitude", "sine_phase",
                     "sine_amplitude_err", "sine_significance")
    rec = numpy.zeros((2, 3), dtype=_lib.SINE_DTYPE)
    har = numpy.zeros((2, 3, 4), dtype=_lib.SINE_HARMONIC_DTYPE)
    har["power"] = numpy.arange(24).reshape(2, 3, 4)
    base = numpy.zeros((2, 3), dtype=[("period", "f8")])
    base["period"] = 7.0
    out = survey._with_sines(base, rec, har)
    assert out.dtype.names == ("period",) + names and out["sine_power"].shape == (2, 3, 4)
    assert (out["period"] == 7.0).all() and out["sine_power"][1, 2].tolist() == [20.0, 21.0, 22.0, 23.0]
    assert survey._with_sines(None, rec[0], har[0]).dtype.names == names


# ---- the header and the binding ----------------------------------------------------------------------------------------------
def test_the_records_of_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for struct, fields, ctype in (("tls_sine_record", _lib.SINE_FIELDS, _lib.SineRecord),
                                  ("tls_sine_harmonic", _lib.SINE_HARMONIC_FIELDS, _lib.SineHarmonic)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
        assert tuple(declared) == fields and ctypes.sizeof(ctype) == 8 * len(fields)
    assert "#define TLS_GLS_MAX_POINTS (1 << 22)" in text and _lib.GLS_MAX_POINTS == 1 << 22
    assert "#define TLS_GLS_MAX_FREQUENCIES (1 << 24)" in text and _lib.GLS_MAX_FREQUENCIES == 1 << 24
    assert "#define TLS_SINE_MAX_HARMONICS 8" in text and _lib.SINE_MAX_HARMONICS == 8
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_gls.hip.h")).read()
    for name, value in (("kGlsRowTile", _lib.GLS_ROW_TILE), ("kGlsSmallRows", _lib.GLS_SMALL_ROWS), ("kGlsFreqTile", _lib.GLS_FREQ_TILE),
                        ("kGlsChunk", _lib.GLS_CHUNK), ("kSineThreads", _lib.SINE_LANES), ("kSineMaxHarmonics", 8),
                        ("kSineWords", 4), ("kSineHarmonicWords", 5)):
        assert "constexpr int %s = %d;" % (name, value) in kernel, name
    assert "constexpr int kGlsMaxPoints = 1 << 22;" in kernel
    assert "__syncthreads" not in re.sub(r"//[^\n]*", "", kernel) and "wg_sync();" in kernel
    assert "#pragma clang fp contract(off)" in kernel and "__builtin_fma(" in kernel
    assert "constexpr double kGlsTwoPi = %r;" % (2 * numpy.pi) in kernel and spec.TWO_PI == 2 * numpy.pi


def test_header_binding_and_library_declare_the_entries():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    for name, count in (("tls_nudft", 8), ("tls_lomb_scargle", 20), ("tls_sine_test", 17)):
        assert re.search(r"\bint\s+%s\s*\(" % name, code)
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
        assert len(getattr(lib, name).argtypes) == declared.count(",") + 1 == count, name
    # (additive entries keep the version: the comment lists what it gained)
    assert "(7: tls_nudft, tls_lomb_scargle, tls_sine_test)" in text.split("#define TLS_AMD_ABI_VERSION")[0]
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_gls.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    for name in ("nudft", "lomb_scargle", "sine_test"):
        assert hasattr(_lib.Context, name)
    assert callable(_lib.lomb_scargle_arguments) and callable(_lib.sine_test_arguments)
