"""The phase scan without a GPU: the host statement (tests/phase_scan_spec.py) tells an eclipsing binary found at its true
period from a planet; tls_phase_record in the header and its mirrors; the two entries in the header, the binding and the
library; the argument checks of survey.phase_scan and survey.power_batch(phase_scan=True) before any device work."""
import ctypes
import os
import re

import numpy
import pytest

import phase_scan_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, transit_model

T = numpy.linspace(3.0, 43.0, 1920)
FLUX = numpy.ones((2, 1920))
P, T0, D = 3.1, 4.0, 0.12


def transit(t0, rp):
    return transit_model.light_curve(T, t0, P, rp, 11, 89.8, 0, 90, [0.4, 0.3], "quadratic")


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


@pytest.mark.parametrize("seed", range(10))
def test_a_secondary_eclipse_stands_out_and_a_planet_does_not(seed):
    """A planet (rp 0.07) with white noise of 4e-4: no window away from the transit reaches 5 sigma of the windows' own
    scatter.  The same curve with a secondary eclipse (rp 0.035) at phase 0.5, and at 0.37 as on an eccentric orbit: at
    least 7 sigma, within one bin of the injected phase."""
    planet = transit(T0, 0.07) + numpy.random.RandomState(seed).normal(0, 4e-4, len(T))
    rec = spec.expected(T, planet, P, T0, D)
    assert rec["status"] == 0 and rec["n_bins"] == 51
    print("seed %d planet: secondary %.2f primary %.1f" % (seed, rec["secondary_significance"], rec["primary_significance"]))
    assert rec["secondary_significance"] < 5
    assert rec["primary_significance"] > 20
    for phase in (0.5, 0.37):
        binary = planet + transit(T0 + phase * P, 0.035) - 1
        rec = spec.expected(T, binary, P, T0, D)
        print("seed %d secondary at %.2f: %.2f at phase %.4f" % (seed, phase, rec["secondary_significance"], rec["secondary_phase"]))
        assert abs(rec["secondary_phase"] - phase) <= 1 / 51
        assert rec["secondary_significance"] >= 7


def test_statement_by_hand():
    """Sixteen bins of one point each, flux 1 but for two dips: every count and depth of the record by hand."""
    t = (numpy.arange(16) + 0.5) / 16                   # P = 1, T0 = 0: point i falls into bin i
    y = numpy.ones(16)
    y[0] = 0.5                                          # in the primary window (bins 15 and 0)
    y[7] = 0.75                                         # windows 6 and 7
    rec, delta = spec.scan(t, y, 1.0, 0.0, 0.125, min_count=2, with_delta=True)
    assert rec["status"] == 0 and rec["n_bins"] == 16
    assert rec["primary_count"] == 2 and rec["primary_depth"] == 11.75 / 12 - 1.5 / 2
    assert [j for j in range(16) if not numpy.isnan(delta[j])] == list(range(2, 13)) + [15]
    assert delta[6] == delta[7] == 10.0 / 10 - 1.75 / 2
    assert rec["secondary_depth"] == delta[6] and rec["secondary_phase"] == 7 / 16 and rec["secondary_count"] == 2
    assert rec["bump_depth"] == delta[2] == 9.75 / 10 - 1 and rec["bump_phase"] == 3 / 16
    assert rec["n_windows"] == 6 and numpy.isnan(rec["scan_mean"]) and numpy.isnan(rec["scan_std"])   # (2, 3 and 9 to 12: 8 are wanted)
    assert spec.scan(t, y, 1.0, 0.0, 0.125)["n_windows"] == 0       # min_count 3: no window of two points counts
    for bad in ((0.0, 0.0, 0.1), (-1.0, 0.0, 0.1), (1.0, numpy.nan, 0.1), (1.0, 0.0, 0.0), (numpy.inf, 0.0, 0.1), (1.0, 0.0, 0.126)):
        rec = spec.scan(t, y, *bad)
        assert rec["status"] == 1 and all(numpy.isnan(v) for k, v in rec.items() if k != "status"), bad
    assert spec.scan(t, y, 1.0, 0.0, 1e-9, max_bins=100)["n_bins"] == 100


def test_phase_scan_without_peak_fits_raises(no_device):
    with pytest.raises(ValueError, match="peak_fits"):
        survey.power_batch(T, FLUX, phase_scan=True)
    with pytest.raises(ValueError, match="peak_fits"):
        survey.power_batch(T, FLUX, peaks=4, phase_scan=True)
    with pytest.raises(ValueError, match="peaks"):
        survey.power_batch(T, FLUX, peak_fits=True, phase_scan=True)


@pytest.mark.parametrize("kw", [dict(max_bins=15), dict(max_bins=4097), dict(max_bins=64.0), dict(max_bins=True),
                                dict(min_count=0), dict(min_count=-3), dict(min_count=2.5)])
def test_bad_bins_and_counts_raise(no_device, kw):
    with pytest.raises(ValueError, match="phase scan"):
        survey.power_batch(T, FLUX, peaks=4, peak_fits=True, phase_scan=True, **{"phase_scan_" + k: v for k, v in kw.items()})
    with pytest.raises(ValueError, match="phase scan"):
        survey.phase_scan(T, FLUX, [3.0, 3.0], [4.0, 4.0], [0.1, 0.1], **kw)


def test_the_binding_refuses_bad_shapes():
    with pytest.raises(ValueError, match="peak_fits"):
        _lib.Context._power_batch(None, T, FLUX, FLUX, numpy.arange(1.0, 3.0), None, None, 3, peaks=(4, 0.02, (), None),
                                  phase_scan=(4096, 3))
    scan = lambda *a, **k: _lib.Context.phase_scan(None, *a, **k)
    with pytest.raises(ValueError, match="one fit a light curve"):
        scan(T, FLUX, [3.0], [4.0], [0.1])
    with pytest.raises(ValueError, match="curve out of range"):
        scan(T, FLUX, [3.0], [4.0], [0.1], curve=[2])
    with pytest.raises(ValueError, match="curve out of range"):
        scan(T, FLUX, [3.0], [4.0], [0.1], curve=[-1])
    with pytest.raises(ValueError, match=r"\[n_fits\]"):
        scan(T, FLUX, [3.0, 3.0], [4.0], [0.1], curve=[0])
    with pytest.raises(ValueError, match="finite"):
        scan(numpy.where(numpy.arange(len(T)) == 5, numpy.nan, T), FLUX, [3.0], [4.0], [0.1], curve=[0])
    with pytest.raises(ValueError, match="over the time stamps"):
        scan(T[:-1], FLUX, [3.0], [4.0], [0.1], curve=[0])


def test_fields_of_the_widened_peaks_array():
    names = survey.phase_scan_fields()
    assert names == ("scan_status",) + spec.FIELDS[1:] + ("secondary_significance", "primary_significance")
    assert spec.FIELDS == _lib.PHASE_SCAN_FIELDS == _lib.PHASE_SCAN_DTYPE.names
    scans = numpy.zeros((2, 3), dtype=_lib.PHASE_SCAN_DTYPE)
    for k in scans.dtype.names:
        scans[k] = numpy.nan
    scans["status"] = [[0, 0, 1], [0, 1, 1]]
    scans["secondary_depth"][:, 0], scans["primary_depth"][:, 0] = [3e-4, 5e-4], [5e-3, 6e-3]
    scans["scan_mean"][:, 0], scans["scan_std"][:, 0] = [1e-5, -2e-5], [1e-4, 0.0]
    fits = numpy.zeros((2, 3), dtype=_lib.PEAK_FIT_DTYPE)
    records = survey._with_fits(survey._with_duration(numpy.zeros((2, 3), dtype=_lib.PEAK_DTYPE), None), fits, 1.0)
    out = survey._with_scans(records, scans)
    assert out.dtype.names == records.dtype.names + names and out.dtype.names.count("status") == 1
    numpy.testing.assert_array_equal(out["scan_status"], scans["status"])
    numpy.testing.assert_array_equal(out["status"], fits["status"])
    assert out["secondary_significance"][0, 0] == (3e-4 - 1e-5) / 1e-4 and out["primary_significance"][0, 0] == (5e-3 - 1e-5) / 1e-4
    assert out["secondary_significance"][1, 0] == numpy.inf            # (no scatter at all: the quotient as it falls)
    assert numpy.isnan(out["secondary_significance"][:, 1:]).all()
    alone = survey._with_scans(None, scans[0])
    assert alone.dtype.names == names and alone.shape == (3,)
    one = spec.expected(T, FLUX[0], P, T0, D)
    assert set(one) == set(spec.FIELDS) | set(names[-2:])


def test_tls_phase_record_is_twelve_doubles():
    assert ctypes.sizeof(_lib.PhaseRecord) == 12 * 8 == _lib.PHASE_SCAN_DTYPE.itemsize
    assert tuple(n for n, _ in _lib.PhaseRecord._fields_) == _lib.PHASE_SCAN_FIELDS
    assert [_lib.PHASE_SCAN_DTYPE.fields[k][1] for k in _lib.PHASE_SCAN_DTYPE.names] == list(range(0, 96, 8))
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct tls_phase_record \{(.*?)\} tls_phase_record;", code, flags=re.S).group(1)
    declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
    assert tuple(declared) == _lib.PHASE_SCAN_FIELDS
    assert (_lib.PHASE_SCANNED, _lib.PHASE_NOTHING) == (spec.SCANNED, spec.NOTHING) == (0, 1)
    assert "#define TLS_PHASE_SCAN_MIN_BINS 16" in text and "#define TLS_PHASE_SCAN_MAX_BINS 4096" in text
    assert (_lib.PHASE_SCAN_MIN_BINS, _lib.PHASE_SCAN_MAX_BINS) == (16, 4096)
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_phase_scan.hip.h")).read()
    assert "constexpr int kPhaseChunk = %d;" % _lib.PHASE_SCAN_CHUNK in kernel
    assert "constexpr int kPhaseMinBins = 16, kPhaseMaxBins = 4096;" in kernel and "constexpr int kPhaseWords = 12;" in kernel


def test_header_binding_and_library_declare_both_entries():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in ("tls_phase_scan", "tls_power_batch_phase_scan", "tls_debug_peak_phase_scans"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
        assert name in text.split("#define TLS_AMD_ABI_VERSION")[0]      # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    # the arguments of tls_power_batch_peak_fits, then the scan's
    fits, scans = (re.search(r"\bint\s+%s\s*\((.*?)\);" % n, code, flags=re.S).group(1)
                   for n in ("tls_power_batch_peak_fits", "tls_power_batch_phase_scan"))
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    assert squeeze(scans) == squeeze(fits) + ", int64_t max_bins, int64_t min_count, tls_phase_record *out_scans"
    assert lib.tls_power_batch_phase_scan.argtypes[:-3] == lib.tls_power_batch_peak_fits.argtypes
    alone = squeeze(re.search(r"\bint\s+tls_phase_scan\s*\((.*?)\);", code, flags=re.S).group(1))
    assert len(lib.tls_phase_scan.argtypes) == alone.count(",") + 1 == 13
    debug, with_scans = (squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % n, code, flags=re.S).group(1))
                         for n in ("tls_debug_peak_fits", "tls_debug_peak_phase_scans"))
    assert with_scans == debug.split(", double *out_epochs")[0] + ", int64_t max_bins, int64_t min_count, tls_phase_record *out_scans"
    assert len(lib.tls_debug_peak_phase_scans.argtypes) == with_scans.count(",") + 1
