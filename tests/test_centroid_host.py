"""The centroid-shift test without a GPU: the loop statement of tests/centroid_spec.py equals the vectorised one bit for bit on
every case of tests/centroid_cases.py, each case shows what it is there to show, the scenario -- a planet on an isolated target
against the same dip from a source a few pixels away -- on the statement, the fields formed on the host against a hand
computation, the record of the header, the binding, and every argument check of survey.centroid_test,
power_batch(centroids=...) and _lib.centroid_arguments before any device work."""
import ctypes
import math
import os
import re
import warnings

import numpy
import pytest

import centroid_cases as cases
import centroid_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, template

T = 1.0 + numpy.arange(300) / 64.0


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64))


_CASES = cases.edge_cases() + [cases.over_a_slab()]


@pytest.mark.parametrize("c", _CASES, ids=[str(c["label"]) for c in _CASES])
def test_loops_equal_the_vectorised_statement(c):
    loops, vector = cases.expected(c, fit=spec.centroid_loops), cases.expected(c)
    for k in spec.FIELDS:
        assert same(loops[k], vector[k]), (c["label"], k)
    c["check"](vector)


def fields_of(record):
    r = dict(zip(spec.FIELDS, record))
    names = ("depth", "depth_err", "shift_x", "shift_x_err", "shift_y", "shift_y_err")
    r.update(zip(("shift", "significance", "offset_x", "offset_y", "offset", "offset_err"),
                 (float(v) for v in survey.centroid_offsets(*(r[k] for k in names)))))
    return r


@pytest.mark.parametrize("seed", range(5))
def test_scenario_which_star_dims(seed):
    """On an isolated target cen_significance <= 5: without a shift it is a chi variable of 2 degrees of freedom, and
    P(> 5) = exp(-12.5) = 4e-6.  With the dimming source at (4, -3) px cen_significance >= 20 and each offset lies within
    5 cen_offset_err of (4, -3).  Seeds 0 to 4 gave: isolated 0.3 to 2.0; the source 62 to 80, x offset 3.90 to 4.05, y offset
    -3.10 to -2.92, cen_offset_err 0.08 to 0.09; the depth 0.00498 to 0.00502 in both."""
    P, d = cases.SCENARIO["period"], cases.SCENARIO["duration"]
    t, y, cx, cy, T0, b = cases.scenario(seed, blended=False)
    loops, alone = spec.centroid_loops(t, y, cx, cy, P, T0, d, b), spec.centroid(t, y, cx, cy, P, T0, d, b)
    assert same(loops, alone)
    alone = fields_of(alone)
    print("isolated", seed, alone)
    assert alone["status"] == 0 and alone["n_epochs"] >= 11 and abs(alone["depth"] - 0.005) < 5 * alone["depth_err"]
    assert alone["significance"] <= 5
    t, y, cx, cy, T0, b = cases.scenario(seed, blended=True)
    blend = fields_of(spec.centroid(t, y, cx, cy, P, T0, d, b))
    print("source at (4, -3)", seed, blend)
    assert blend["status"] == 0 and blend["significance"] >= 20
    assert abs(blend["offset_x"] - 4.0) <= 5 * blend["offset_err"] and abs(blend["offset_y"] + 3.0) <= 5 * blend["offset_err"]
    assert abs(blend["offset"] - 5.0) <= 5 * blend["offset_err"]


def test_one_event_carries_the_shift():
    """A shift of 0.02 px put into ONE of the thirteen events: chi2_x says so.  With 12 degrees of freedom a chi^2 above
    5 * 12 = 60 has a chance of 2e-8; chi2_y, untouched, stays below it (seed 0 gave 137 and 15)."""
    P, d = cases.SCENARIO["period"], cases.SCENARIO["duration"]
    t, y, cx, cy, T0, b = cases.scenario(0, blended=False)
    cx = cx + numpy.where(numpy.abs(t - (T0 + 3 * P)) <= 0.4 * d, 0.02, 0.0)
    r = fields_of(spec.centroid(t, y, cx, cy, P, T0, d, b))
    assert r["n_epochs"] == 13 and r["chi2_x"] > 5 * (r["n_epochs"] - 1) > r["chi2_y"]


def test_the_host_formed_fields():
    """centroid_fields() against a hand computation: sx = 3e-3, sy = -4e-3, D = 0.01: shift 5e-3, lever 99, offset (-0.297,
    0.396), 0.495; ex = ey = 1e-3: significance 5, var_shift 1e-6; eD = 1e-3: (99 * 1e-3)^2 + (50 * 1e-3)^2."""
    raw = numpy.zeros(4, dtype=_lib.CENTROID_DTYPE)
    for k in _lib.CENTROID_FIELDS:
        raw[k] = numpy.nan
    raw["status"] = [0, 0, 0, 1]
    raw["depth"], raw["depth_err"] = [0.01, -0.01, 0.0, numpy.nan], 1e-3
    raw["shift_x"], raw["shift_y"], raw["shift_x_err"], raw["shift_y_err"] = 3e-3, -4e-3, 1e-3, 1e-3
    out = survey._with_centroids(None, raw)
    assert out.dtype.names == survey.centroid_fields() == tuple("cen_" + k for k in _lib.CENTROID_FIELDS) + (
        "cen_shift", "cen_significance", "cen_offset_x", "cen_offset_y", "cen_offset", "cen_offset_err")
    for k in _lib.CENTROID_FIELDS:
        assert same(out["cen_" + k], raw[k])
    want = dict(cen_shift=5e-3, cen_significance=5.0, cen_offset_x=-0.297, cen_offset_y=0.396, cen_offset=0.495,
                cen_offset_err=math.sqrt(0.099 ** 2 + 0.05 ** 2))
    for k, v in want.items():
        assert abs(out[k][0] - v) < 1e-12 * max(1.0, abs(v)), k
        assert numpy.isnan(out[k][1:]).all(), k      # (depth <= 0, and no depth at all)
    base = numpy.zeros(4, dtype=[("period", "f8"), ("status", "i4")])
    base["period"] = [1.0, 2.0, 3.0, 4.0]
    more = survey._with_centroids(base, raw)
    assert more.dtype.names == ("period", "status") + survey.centroid_fields() and more["period"].tolist() == [1.0, 2.0, 3.0, 4.0]


def test_constants_and_shape():
    assert ctypes.sizeof(_lib.CentroidRecord) == 128 == _lib.CENTROID_DTYPE.itemsize
    assert _lib.CENTROID_FIELDS == spec.FIELDS and _lib.CENTROID_SHAPE_SAMPLES == spec.SHAPE_SAMPLES == 1025
    assert _lib.CENTROID_MAX_EPOCHS == spec.MAX_EPOCHS == 65536
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, _, _ = survey._batch_inputs(T, numpy.ones((1, len(T))) + 1e-3 * numpy.sin(T)[None, :], None,
                                         dict(oversampling_factor=1))
    b = survey._centroid_shape(inp)
    assert same(b, 1.0 - template.reference_transit(1025, **inp["shape"]))
    # (the first and last samples are the first and last in-transit ones of the supersampled curve: a hair below the baseline)
    assert b.shape == (1025,) and b.max() == 1.0 and b.min() >= 0.0 and b[0] < 1e-3 and b[-1] < 1e-3 and b[512] == 1.0
    assert survey.centroid_epochs(T, [1.0, numpy.nan, -2.0, 0.5]) == math.ceil((T[-1] - T[0]) / 0.5) + 2
    assert survey.centroid_epochs(T, [numpy.nan]) == 1 and survey.centroid_epochs(T, [1e-9]) == 65536


def test_the_record_of_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct tls_centroid_record \{(.*?)\} tls_centroid_record;", code, flags=re.S).group(1)
    declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
    assert tuple(declared) == _lib.CENTROID_FIELDS
    assert "#define TLS_CENTROID_MAX_EPOCHS 65536" in text and "#define TLS_CENTROID_MAX_SHAPE 1048576" in text
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_centroid.hip.h")).read()
    assert "constexpr int kCentroidMaxEpochs = 65536;" in kernel and "constexpr int kCentroidWords = 16;" in kernel
    assert "constexpr int kCentroidLdsEpochs = %d;" % _lib.CENTROID_LDS_EPOCHS in kernel
    assert "constexpr int kCentroidThreads = %d;" % _lib.CENTROID_THREADS in kernel
    assert "constexpr int kCentroidMaxPoints = 1 << 22;" in kernel and _lib.CENTROID_MAX_POINTS == 1 << 22
    assert "constexpr int kCentroidMaxShape = 1 << 20;" in kernel and _lib.CENTROID_MAX_SHAPE == 1 << 20
    bare = re.sub(r"//[^\n]*", "", kernel)
    assert "__syncthreads" not in bare and "wg_sync();" in kernel and "atomic" not in bare
    assert "#pragma clang fp contract(off)" in kernel


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_centroid_test"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "(8: %s)" % name in text.split("#define TLS_AMD_ABI_VERSION")[0]     # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_centroid_test.argtypes) == declared.count(",") + 1 == 19
    assert declared.endswith("const double *shape, int64_t L, double window, int64_t min_in, int64_t min_out, "
                             "int64_t max_epochs, tls_centroid_record *out")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_centroid.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    assert '#include "tls_centroid.hip.h"' in open(os.path.join(REPO, "tls_amd", "csrc", "tls_kernels.hip.h")).read()
    assert hasattr(_lib.Context, "centroid_test") and callable(_lib.centroid_arguments)
    assert "tls_centroid_test" in open(os.path.join(REPO, "INTEGRATION.md")).read()


FLUX = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
CEN = numpy.random.RandomState(1).normal(0, 1e-3, (2, 2, len(T)))

BAD = [
    (dict(cx_batch=CEN[0][:, :-1]), "cx must have the shape"), (dict(cy_batch=CEN[1][:1]), "cy must have the shape"),
    (dict(cx_batch=CEN[0][0]), "cx must have the shape"), (dict(cy_batch="x"), "cy must hold numbers"),
    (dict(window=0.99), "window"), (dict(window=numpy.nan), "window"), (dict(window=numpy.inf), "window"),
    (dict(window="3"), "window"), (dict(window=True), "window"),
    (dict(min_in=0), "min_in"), (dict(min_in=1.5), "min_in"), (dict(min_in=True), "min_in"),
    (dict(min_out=0), "min_out"), (dict(min_out=2.0), "min_out"),
    (dict(max_epochs=0), "max_epochs"), (dict(max_epochs=65537), "max_epochs"), (dict(max_epochs=10.0), "max_epochs"),
    (dict(period=[1.0]), "n_fits"), (dict(period=[[1.0, 1.5]]), "n_fits"), (dict(T0=["a", "b"]), "numbers"),
    (dict(curve=[0, 2]), "curve"), (dict(curve=[0.0, 1.0]), "curve"), (dict(curve=[0]), "curve")]


@pytest.mark.parametrize("kw, match", BAD)
def test_survey_call_refuses_before_any_device_work(no_device, kw, match):
    args = dict(dict(cx_batch=CEN[0], cy_batch=CEN[1], period=[1.0, 1.5], T0=[1.2, 1.3], duration=[0.1, 0.1]), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.centroid_test(T, FLUX, **args)
        with pytest.raises(ValueError, match=match):              # (nor is anything detrended first)
            survey.centroid_test(T, FLUX, detrend=25, **args)


def test_survey_call_checks_the_rows_and_reaches_the_device(no_device):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="flux_batch must be"):
            survey.centroid_test(T, FLUX[:, :-1], CEN[0], CEN[1], [1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
        with pytest.raises(ValueError, match="one candidate a light curve"):
            survey.centroid_test(T, FLUX, CEN[0], CEN[1], [1.0], [1.2], [0.1])
        with pytest.raises(ValueError, match="non-decreasing"):
            survey.centroid_test(T[::-1], FLUX, CEN[0], CEN[1], [1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
        holes = CEN.copy()
        holes[0, 0, 5:9], holes[1, 1, 100] = numpy.nan, numpy.inf
        with pytest.raises(AssertionError, match="a context was created"):     # (a good call reaches the device, holes and all)
            survey.centroid_test(T, FLUX, holes[0], holes[1], [1.0, numpy.nan], [1.2, 1.3], [0.1, -1.0])
        with pytest.raises(AssertionError, match="a context was created"):     # (one row [n])
            survey.centroid_test(T, FLUX[0], CEN[0][0], CEN[1][0], [1.0], [1.2], [0.1], window=1.0, min_in=3, max_epochs=1)


@pytest.mark.parametrize("kw, match", [
    (dict(), "needs peak_fits"), (dict(peaks=3), "needs peak_fits"),
    (dict(peaks=3, peak_fits=True, centroid_window=0.5), "window"),
    (dict(peaks=3, peak_fits=True, centroid_window=numpy.nan), "window"),
    (dict(peaks=3, peak_fits=True, centroid_min_in=0), "min_in"),
    (dict(peaks=3, peak_fits=True, centroid_min_out=1.5), "min_out"),
    (dict(peaks=3, peak_fits=True, centroids=(CEN[0],)), "pair"),
    (dict(peaks=3, peak_fits=True, centroids=CEN[0][0][0]), "pair"),
    (dict(peaks=3, peak_fits=True, centroids=(CEN[0], CEN[1][:, :-1])), "cy must have the shape"),
    (dict(peaks=3, peak_fits=True, centroids=(CEN[0][:1], CEN[1])), "cx must have the shape")])
def test_power_batch_refuses_before_any_device_work(no_device, kw, match):
    kw = dict(dict(centroids=(CEN[0], CEN[1])), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, FLUX, **kw)
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, FLUX, detrend=25, **kw)


GOOD = dict(t=T, y=numpy.ones(300), cx=numpy.zeros(300), cy=numpy.zeros(300), period=[1.0, 2.0], T0=[1.1, 1.2],
            duration=[0.1, 0.2], shape=[0.0, 1.0, 0.0], curve=[0, 0])


@pytest.mark.parametrize("kw", [
    dict(curve=[0, 1]), dict(curve=[-1, 0]), dict(curve=None), dict(T0=[1.0]), dict(duration=[[0.1, 0.2]]), dict(t=T[::-1]),
    dict(t=numpy.where(numpy.arange(300) == 7, numpy.nan, T)), dict(y=numpy.full(300, numpy.nan)), dict(y=numpy.ones(299)),
    dict(cx=numpy.zeros(299)), dict(cy=numpy.zeros((2, 300))), dict(shape=[1.0]), dict(shape=[0.0, numpy.nan, 0.0]),
    dict(shape=[0.0, numpy.inf]), dict(shape=[[0.0, 1.0]]), dict(shape="b"), dict(window=0.5), dict(min_in=0), dict(min_out=0),
    dict(max_epochs=0), dict(max_epochs=65537)])
def test_centroid_arguments_refuses(kw):
    with pytest.raises(ValueError, match="^centroid test: "):
        _lib.centroid_arguments(**dict(GOOD, **kw))


def test_centroid_arguments_packs():
    cx = numpy.zeros(300)
    cx[3] = numpy.nan
    a = _lib.centroid_arguments(**dict(GOOD, period=[numpy.nan, -2.0], cx=cx))      # (any candidate value; holes stay)
    assert a["y"].shape == a["cx"].shape == a["cy"].shape == (1, 300) and numpy.isnan(a["cx"][0, 3])
    assert a["curve"].dtype == numpy.int64 and a["curve"].tolist() == [0, 0] and a["shape"].tolist() == [0.0, 1.0, 0.0]
    assert (a["window"], a["min_in"], a["min_out"], a["max_epochs"]) == (3.0, 1, 3, 65536)
    assert all(a[k].flags.c_contiguous and a[k].dtype == numpy.float64 for k in ("t", "y", "cx", "cy", "period", "T0", "duration"))
    one = _lib.centroid_arguments(T, numpy.ones((2, 300)), numpy.zeros((2, 300)), numpy.zeros((2, 300)), [1.0, 2.0], [1.1, 1.2],
                                  [0.1, 0.2], [0.0, 1.0])
    assert one["curve"].tolist() == [0, 1]
