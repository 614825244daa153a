"""Periodogram peaks without a GPU: the properties of the selection's numpy statement (tests/peaks_spec.py), the host-side
argument checks of survey.power_batch(peaks=...) and survey.find_peaks, and the two entries in the header and the binding."""
import os
import re

import numpy
import pytest

import peaks_spec
from conftest import REPO
from tls_amd import _lib, survey


def spectra(seed, n, smooth=True):
    rng = numpy.random.RandomState(seed)
    power = rng.normal(0, 1, n)
    if smooth:
        power = numpy.convolve(power, numpy.ones(5) / 5, mode="same")
    periods = numpy.sort(rng.uniform(0.5, 20.0, n))
    return power, periods


@pytest.mark.parametrize("seed", range(6))
def test_first_peak_is_argmax_and_peaks_are_distinct_candidates(seed):
    power, periods = spectra(seed, 700)
    j = peaks_spec.find_peaks(power, periods, 12)
    assert len(j) and j[0] == numpy.argmax(power)
    assert len(set(j.tolist())) == len(j)
    assert peaks_spec.candidates(power)[j].all()
    assert numpy.all(numpy.diff(power[j]) <= 0)   # (greedy: what is taken later was alive earlier)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("ratios", [(), peaks_spec.HARMONICS])
def test_no_peak_in_an_earlier_peaks_windows(seed, ratios):
    power, periods = spectra(seed + 10, 900)
    sep = 0.03
    j = peaks_spec.find_peaks(power, periods, 16, sep, ratios)
    assert len(j) > 3
    for a in range(len(j)):
        inside = peaks_spec.windows(periods, periods[j[a]], sep, ratios)
        assert inside[j[a]]
        assert not inside[j[a + 1:]].any()
    # and the selection is maximal: an untaken candidate above the last peak lies in some taken peak's windows
    left = peaks_spec.candidates(power)
    for a in j:
        left &= ~peaks_spec.windows(periods, periods[a], sep, ratios)
    assert len(j) == 16 or not left.any()
    assert not (left & (power > power[j[-1]])).any()


def test_k_beyond_the_candidates_returns_fewer():
    power = numpy.array([0.0, 3.0, 1.0, 2.0, 0.5, 0.5, 4.0, numpy.nan, 9.0])
    periods = numpy.arange(1.0, 10.0)
    cand = peaks_spec.candidates(power)
    assert cand.tolist() == [False, True, False, True, False, False, False, False, False]
    j = peaks_spec.find_peaks(power, periods, 32, 0.0, ())
    assert j.tolist() == [1, 3]
    rec, m = peaks_spec.expected(power, periods, 5, 0.0, ())
    assert m == 2 and rec["index"].tolist() == [1, 3, -1, -1, -1]
    assert numpy.isnan(rec["period"][2:]).all() and numpy.isnan(rec["chi2"]).all() and (rec["row"] == -1).all()
    assert len(peaks_spec.find_peaks(power, periods, 32, 0.0, (), min_power=10.0)) == 0
    assert peaks_spec.find_peaks(power, periods, 32, 0.0, (), min_power=3.0).tolist() == [1]


def test_plateaus_ends_and_single_points():
    assert peaks_spec.candidates([1.0]).tolist() == [True]
    assert peaks_spec.candidates([numpy.nan]).tolist() == [False]
    assert peaks_spec.candidates([2.0, 2.0, 2.0]).tolist() == [True, False, False]     # the first of a plateau
    assert peaks_spec.candidates([1.0, 2.0, 3.0]).tolist() == [False, False, True]
    assert peaks_spec.candidates([3.0, 2.0, 1.0]).tolist() == [True, False, False]
    assert peaks_spec.candidates([1.0, 2.0, 2.0, 1.0]).tolist() == [False, True, False, False]


def test_zero_separation_suppresses_equal_periods_only():
    power = numpy.array([0.0, 5.0, 0.0, 4.0, 0.0, 3.0, 0.0])
    periods = numpy.array([1.0, 2.0, 3.0, 2.0, 5.0, 2.0 * (1 + 2.0 ** -52), 7.0])
    assert peaks_spec.find_peaks(power, periods, 8, 0.0, ()).tolist() == [1, 5]
    # ratio 2 with sep 0: exactly twice the period goes, its neighbour in the last place stays
    periods = numpy.array([1.0, 2.0, 3.0, 4.0, 5.0, 4.0 * (1 + 2.0 ** -52), 7.0])
    assert peaks_spec.find_peaks(power, periods, 8, 0.0, (2.0,)).tolist() == [1, 5]


def test_descending_periods_select_the_mirrored_indices():
    power, periods = spectra(3, 500, smooth=False)
    power = power[:400]   # (distinct values: the mirrored row has the same candidates)
    assert len(numpy.unique(power)) == 400
    periods = periods[:400]
    up = peaks_spec.find_peaks(power, periods, 10, 0.02, peaks_spec.HARMONICS)
    down = peaks_spec.find_peaks(power[::-1], periods[::-1], 10, 0.02, peaks_spec.HARMONICS)
    assert (399 - down).tolist() == up.tolist()


T = numpy.linspace(0.0, 20.0, 480)
FLUX = numpy.ones((2, 480))
BAD = [dict(k=0), dict(k=33), dict(k=2.5), dict(k=True), dict(sep=-0.01), dict(sep=1.0), dict(sep=1.5), dict(sep=numpy.nan),
       dict(sep=numpy.inf), dict(ratios=tuple(1.0 + 0.1 * i for i in range(17))), dict(ratios=(0.5, 0.0)),
       dict(ratios=(-2.0,)), dict(ratios=(numpy.inf,)), dict(ratios=(numpy.nan,)), dict(min_power=numpy.nan)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "%s=%s" % (list(b)[0], str(list(b.values())[0])[:12]))
def test_bad_arguments_raise_on_the_host(bad, monkeypatch):
    """ValueError from both entry points before any context exists (creating one fails the test)."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    a = dict(k=4, sep=0.02, ratios=survey.HARMONICS, min_power=None)
    a.update(bad)
    with pytest.raises(ValueError):
        survey.power_batch(T, FLUX, peaks=a["k"], peak_separation=a["sep"], peak_ratios=a["ratios"], peak_min_power=a["min_power"])
    with pytest.raises(ValueError):
        survey.find_peaks(numpy.zeros(8), numpy.arange(1.0, 9.0), a["k"], separation=a["sep"], ratios=a["ratios"],
                          min_power=a["min_power"])


def test_peaks_with_models_raises(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    with pytest.raises(ValueError, match="models"):
        survey.power_batch(T, FLUX, peaks=4, models=True)


def test_find_peaks_shapes_are_checked_on_the_host(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    with pytest.raises(ValueError):
        survey.find_peaks(numpy.zeros(8), numpy.arange(1.0, 8.0), 3)
    with pytest.raises(ValueError):
        survey.find_peaks(numpy.zeros((2, 8)), numpy.arange(1.0, 9.0), 3, chi2=numpy.zeros(8))
    with pytest.raises(ValueError):
        survey.find_peaks(numpy.zeros(0), numpy.zeros(0), 3)


def test_good_arguments_pass_the_check():
    k, sep, ratios, low = _lib.peaks_arguments(32, 0.0, (), None)
    assert (k, sep, len(ratios), low) == (32, 0.0, 0, -numpy.inf)
    k, sep, ratios, low = _lib.peaks_arguments(numpy.int64(1), 0.999, [0.5] * 16, 3)
    assert (k, len(ratios), low) == (1, 16, 3.0) and ratios.dtype == numpy.float64
    assert survey.HARMONICS == (0.5, 2.0, 1 / 3, 3.0, 2 / 3, 1.5) == peaks_spec.HARMONICS


def test_header_and_binding_declare_both_entries():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("tls_find_peaks", "tls_power_batch_peaks"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS
        assert name in text.split("#define TLS_AMD_ABI_VERSION")[0]      # (the version comment lists the entries it gained)
    assert re.search(r"typedef struct tls_peak \{\s*double period, power, chi2, depth;\s*int64_t index, row;\s*\} tls_peak;", code)
    assert "#define TLS_AMD_ABI_VERSION 8" in text
    assert [n for n, _ in _lib.Peak._fields_] == list(_lib.PEAK_DTYPE.names) == ["period", "power", "chi2", "depth", "index", "row"]
    assert _lib.PEAK_DTYPE.itemsize == 48
    assert ("#define TLS_PEAKS_MAX_K %d" % _lib.PEAKS_MAX_K) in text and ("#define TLS_PEAKS_MAX_RATIOS %d" % _lib.PEAKS_MAX_RATIOS) in text
