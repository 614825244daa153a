"""The peak fits without a GPU: the host-side argument checks of survey.power_batch(peak_fits=True), the fields it adds to the
`peaks` array, tls_peak_fit in the header and its ctypes mirror, and the two entries in the header and the binding."""
import ctypes
import os
import re

import numpy
import pytest

from conftest import REPO
from tls_amd import _lib, survey

T = numpy.linspace(0.0, 20.0, 480)
FLUX = numpy.ones((2, 480))


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)


def test_peak_fits_without_peaks_raises(no_device):
    with pytest.raises(ValueError, match="peaks"):
        survey.power_batch(T, FLUX, peak_fits=True)
    with pytest.raises(ValueError, match="peaks"):
        survey.power_batch(T, FLUX, peak_fits=True, statistics=True)


def test_peak_fits_with_models_raises(no_device):
    with pytest.raises(ValueError, match="peak_fits cannot be combined"):
        survey.power_batch(T, FLUX, peaks=4, peak_fits=True, models=True)


def test_peak_fits_need_ascending_time_stamps(no_device):
    with pytest.raises(ValueError, match="ascending"):
        survey.power_batch(T[::-1], FLUX, peaks=4, peak_fits=True)
    with pytest.raises(ValueError, match="k must be"):
        survey.power_batch(T, FLUX, peaks=33, peak_fits=True)


def test_the_binding_refuses_fits_without_peaks():
    with pytest.raises(ValueError, match="peaks"):
        _lib.Context._power_batch(None, T, FLUX, FLUX, numpy.arange(1.0, 3.0), None, None, 3, peak_fits=(1.0, numpy.zeros(481), 5))


def test_fields_of_the_widened_peaks_array():
    added = ("T0", "status", "period_uncertainty", "duration_days", "depth_mean", "depth_mean_std", "depth_mean_even",
             "depth_mean_even_std", "depth_mean_odd", "depth_mean_odd_std", "snr", "odd_even_mismatch", "transit_count",
             "distinct_transit_count", "empty_transit_count", "in_transit_count", "after_transit_count",
             "before_transit_count", "rp_rs")
    assert survey.peak_fit_fields() == added
    assert added[2:-1] == _lib.TRANSIT_STATS_FIELDS == tuple(n for n, _ in _lib.TransitStats._fields_)
    peaks = numpy.zeros((2, 3), dtype=_lib.PEAK_DTYPE)
    peaks["row"] = [[0, 1, -1], [1, -1, -1]]
    peaks["depth"] = [[0.99, 0.9975, numpy.nan], [0.96, numpy.nan, numpy.nan]]
    fits = numpy.zeros((2, 3), dtype=_lib.PEAK_FIT_DTYPE)
    fits["status"] = [[0, 0, 1], [0, 2, 1]]
    fits["T0"] = [[3.5, 4.5, numpy.nan], [5.5, numpy.nan, numpy.nan]]
    fits["snr"] = 7.0
    out = survey._with_fits(survey._with_duration(peaks, numpy.array([0.01, 0.02])), fits, 1.0)
    assert out.dtype.names == ("period", "power", "chi2", "depth", "index", "row", "duration") + added
    assert all(out.dtype[k] == numpy.dtype("f8") for k in added)
    numpy.testing.assert_array_equal(out["T0"], fits["T0"])
    numpy.testing.assert_array_equal(out["snr"], fits["snr"])
    numpy.testing.assert_array_equal(out["duration"], [[0.01, 0.02, numpy.nan], [0.02, numpy.nan, numpy.nan]])
    # rp_rs from the candidate's own depth, as the summary forms it; NaN where nothing was fitted
    numpy.testing.assert_array_equal(out["rp_rs"], [[(1 - 0.99) ** 0.5, (1 - 0.9975) ** 0.5, numpy.nan], [(1 - 0.96) ** 0.5, numpy.nan, numpy.nan]])
    half = survey._with_fits(survey._with_duration(peaks, None), fits, 0.25)
    assert half["rp_rs"][0, 0] == ((1 - 0.99) * 0.25) ** 0.5


def test_tls_peak_fit_is_eighteen_doubles():
    assert ctypes.sizeof(_lib.PeakFit) == 18 * 8 == _lib.PEAK_FIT_DTYPE.itemsize
    assert [n for n, _ in _lib.PeakFit._fields_] == ["T0", "status", "stats"]
    assert _lib.PeakFit.stats.offset == 16 and ctypes.sizeof(_lib.TransitStats) == 16 * 8
    assert _lib.PEAK_FIT_DTYPE.names == ("T0", "status") + _lib.TRANSIT_STATS_FIELDS
    assert [_lib.PEAK_FIT_DTYPE.fields[k][1] for k in _lib.PEAK_FIT_DTYPE.names] == list(range(0, 144, 8))
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef struct tls_peak_fit \{\s*double T0;\s*double status;\s*tls_transit_stats stats;\s*\} tls_peak_fit;", code)
    assert (_lib.PEAK_FITTED, _lib.PEAK_NONE, _lib.PEAK_UNFITTED) == (0, 1, 2)


def test_header_binding_and_library_declare_both_entries():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("tls_power_batch_peak_fits", "tls_debug_peak_fits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
        assert name in text.split("#define TLS_AMD_ABI_VERSION")[0]      # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    # the arguments of tls_power_batch_peaks, then the fits
    peaks, fits = (re.search(r"\bint\s+%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
                   for n in ("tls_power_batch_peaks", "tls_power_batch_peak_fits"))
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    assert squeeze(fits) == squeeze(peaks) + ", tls_peak_fit *out_fits"
    assert lib.tls_power_batch_peak_fits.argtypes[:-1] == lib.tls_power_batch_peaks.argtypes
    assert len(lib.tls_debug_peak_fits.argtypes) == squeeze(re.search(r"\bint\s+tls_debug_peak_fits\s*\((.*?)\);", code,
                                                                      flags=re.S).group(1)).count(",") + 1
