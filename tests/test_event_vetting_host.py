"""Event vetting without a GPU: the statement (tests/event_vetting_spec.py) equals its own loops bit for bit, on random
candidates and on every edge the GPU test names (tests/event_vetting_cases.py); it passes the events of a planet and fails
those of three unrelated events lined up on an ephemeris; the argument checks of the Python layer, all raised before any
device work; the rows; the field lists; and the header, the binding and the version comment name tls_event_vetting."""
import ctypes
import os
import re
import warnings

import numpy
import pytest

import event_vetting_cases as cases
import event_vetting_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, transit_model

SHAPE = cases.SHAPE
T = 1.0 + numpy.arange(300) / 64.0


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


# ---- the two forms of the statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5, 12, 37])
def test_the_loops_equal_the_vectorised_form(L):
    """A series with a gap, per-point dy, odd and even widths, candidates whose first and last epochs hang over the ends,
    chase reaches beyond the series and inside the guard; and candidates of status 1 and 2."""
    rng = numpy.random.default_rng(L)
    t = numpy.delete(T, numpy.arange(140, 170))
    y = 1 + rng.normal(0, 1e-3, len(t))
    for at in range(3, len(t), 45):
        y[at: at + L] -= 4e-3
    dy = rng.uniform(5e-4, 2e-3, len(t))
    b = spec.shapes_of([L], **SHAPE)[0]
    span = (L - 1) / 64.0 * 1.5
    for P, T0, S, R, Gd, min_ses, epochs in ((45 / 64.0, T[3 + L // 2], L, 20, L, 3.0, 8), (0.61, 0.93, 2, 400, 0, 0.0, 9),
                                             (0.2, 1.0, 1, 9, 3, 3.0, 40), (0.61, 0.93, 2, 5, 5, 3.0, 9),
                                             (numpy.nan, 1.0, 1, 5, 1, 3.0, 4), (0.2, 1.0, 1, 5, 1, 3.0, 4),
                                             (-1.0, 1.0, 1, 5, 1, 3.0, 4), (50.0, 0.5, 1, 5, 1, 3.0, 4)):
        kw = dict(depth_min=1e-4, min_ses=min_ses, chase_fraction=0.5, chase_min=0.4, point_fraction=0.45, step_fraction=0.3,
                  max_epochs=epochs)
        fast = spec.event_vetting(t, y, dy, P, T0, b, span, S, R, Gd, 0.1 * abs(P), **kw)
        slow = spec.event_vetting_loops(t, y, dy, P, T0, b, span, S, R, Gd, 0.1 * abs(P), **kw)
        assert fast[0].tobytes() == slow[0].tobytes() and fast[1].tobytes() == slow[1].tobytes(), (L, P)
        assert fast[0].shape == (15,) and fast[1].shape == (epochs, 14)
    assert slow[0][0] == 2 and numpy.isnan(slow[1]).all()                # (no epoch of 0.5 + 50 e inside the series)
    assert spec.event_vetting(t, y, dy, 0.2, 1.0, b, span, 1, 5, 1, 0.1, max_epochs=4)[0][:2].tolist() == [2.0, 24.0]
    assert spec.event_vetting(t, y, dy, numpy.inf, 1.0, b, span, 1, 5, 1, 0.1)[0][0] == 1


_EDGES = cases.edge_cases()


@pytest.mark.parametrize("c", _EDGES, ids=[str(c["label"]) for c in _EDGES])
def test_the_loops_equal_the_vectorised_form_on_every_edge(c):
    """The cases the device is tested on: both forms agree, and each shows what it is there to show."""
    fast, slow = cases.expected(c), cases.expected(c, loops=True)
    assert fast[0].tobytes() == slow[0].tobytes() and fast[1].tobytes() == slow[1].tobytes()
    assert fast[0].dtype.names == spec.SUMMARY_FIELDS and fast[1].dtype.names == spec.EVENT_FIELDS
    c["check"](*slow)


def test_the_loops_equal_the_vectorised_form_on_a_sample_of_many_candidates():
    c = cases.many_candidates()
    which = numpy.arange(0, 1030, 41)
    fast, slow = cases.expected(c, which=which), cases.expected(c, loops=True, which=which)
    assert fast[0].tobytes() == slow[0].tobytes() and fast[1].tobytes() == slow[1].tobytes()
    assert (fast[0]["status"] == 0).all() and (fast[0]["n_held"] >= 2).sum() > 20


# ---- behaviour ------------------------------------------------------------------------------------------------------------------
SIGMA, WIDTH = 3e-4, 7
SERIES = numpy.delete(2 + numpy.arange(1920) / 48, numpy.arange(900, 960))


def vetted(flux, P, T0):
    """The statement on one light curve of SERIES: L = 7, reach L, dy = SIGMA, the defaults of survey.event_vetting otherwise."""
    t = SERIES
    dt = numpy.median(numpy.diff(t))
    widths, span_max, row, reach, chase_reach, guard, chase_span = survey.event_vetting_rows(t, [P], [WIDTH * dt])
    assert widths.tolist() == [WIDTH] and reach.tolist() == [WIDTH] and guard.tolist() == [10]
    b = spec.shapes_of([WIDTH], **SHAPE)[0]
    record, rows = spec.event_vetting(t, flux, numpy.full(len(t), SIGMA), P, T0, b, span_max[0], reach[0], chase_reach[0], guard[0],
                                      chase_span[0], max_epochs=16)
    record = dict(zip(spec.SUMMARY_FIELDS, record))
    rows = rows[:int(record["n_epochs"])]
    return record, {k: rows[:, i] for i, k in enumerate(spec.EVENT_FIELDS)}


@pytest.mark.parametrize("seed", range(5))
def test_the_events_of_a_planet_are_good(seed):
    """A planet of period 7.3 d and rp = 0.03 on white noise of 3e-4: six transits, all held, all good, none chased.  Seeds 0
    to 4 on the CPU: dominance 0.44 to 0.47, the largest point_share 0.28 to 0.33, the largest side 0.11 to 0.21, mes 17.4
    to 21.3 with mes_rest 15.4 to 18.9 (every figure is printed)."""
    t = SERIES
    T0 = t[0] + 3.1
    flux = transit_model.light_curve(t, T0, 7.3, 0.03, 17.0, 89.5, 0, 90, [0.4, 0.3], "quadratic") \
        + numpy.random.default_rng(seed).normal(0, SIGMA, len(t))
    record, rows = vetted(flux, 7.3, T0)
    sides = numpy.concatenate([rows["before"], rows["after"]])
    print("planet seed %d: dominance %.3f, largest point_share %.3f, largest side %.3f, mes %.2f, mes_good %.2f, mes_rest %.2f, "
          "chases_min %.2f" % (seed, record["dominance"], rows["point_share"].max(), numpy.nanmax(sides), record["mes"],
                               record["mes_good"], record["mes_rest"], record["chases_min"]))
    assert record["n_good"] == record["n_held"] == 6
    assert (rows["chases"] == 1.0).all()


@pytest.mark.parametrize("seed", range(5))
def test_three_unrelated_events_on_an_ephemeris_are_not(seed):
    """P = 11 d: two single-sample outliers of 12 sigma at epochs 0 and 1, a step of 2.5 sigma that decays over 40 samples at
    epoch 2, nothing at epoch 3; white noise of sigma with red noise on top, a 12-sample boxcar mean of unit white noise times
    sigma.  The stacked signal is strong, yet at most one event is good.  Seeds 0 to 4 on the CPU: mes 7.7 to 11.0,
    n_good 0 (four seeds) or 1 (seed 1, the decaying step), chases_min 0.21 to 0.23, the outliers' point_share 0.73 to 1.03,
    every outlier flagged 2, the empty epoch flagged 8 with other bits (every figure is printed)."""
    t = SERIES
    rng = numpy.random.default_rng(seed)
    P, T0 = 11.0, t[0] + 2.0
    flux = 1 + rng.normal(0, SIGMA, len(t))
    flux += SIGMA * numpy.convolve(rng.normal(0, 1, len(t) + 11), numpy.ones(12) / 12, mode="valid")
    centre = [int(numpy.argmin(numpy.abs(t - (T0 + e * P)))) for e in range(4)]
    flux[centre[0]] -= 12 * SIGMA
    flux[centre[1]] -= 12 * SIGMA
    flux[centre[2]: centre[2] + 40] -= 2.5 * SIGMA * numpy.exp(-numpy.arange(40) / 15.0)
    record, rows = vetted(flux, P, T0)
    print("fake seed %d: mes %.2f, n_held %d, n_good %d, chases_min %.2f, point_share %s, flags %s"
          % (seed, record["mes"], record["n_held"], record["n_good"], record["chases_min"],
             numpy.round(rows["point_share"], 2).tolist(), rows["flags"].tolist()))
    assert record["n_epochs"] == 4
    assert record["n_good"] <= 1


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_field_lists():
    assert spec.SUMMARY_FIELDS == _lib.EVENT_SUMMARY_FIELDS == _lib.EVENT_SUMMARY_DTYPE.names == survey.event_summary_fields()
    assert spec.EVENT_FIELDS == _lib.EVENT_RECORD_FIELDS == _lib.EVENT_RECORD_DTYPE.names == survey.event_fields()
    assert len(spec.SUMMARY_FIELDS) == 15 and len(spec.EVENT_FIELDS) == 14
    assert ctypes.sizeof(_lib.EventSummary) == 120 == _lib.EVENT_SUMMARY_DTYPE.itemsize
    assert ctypes.sizeof(_lib.EventRecord) == 112 == _lib.EVENT_RECORD_DTYPE.itemsize
    assert spec.MAX_CHASE == _lib.EVENTS_MAX_CHASE == 8192
    assert spec.DEFAULTS == dict(depth_min=0.0, min_ses=3.0, chase_fraction=0.6, chase_min=0.5, point_fraction=0.5,
                                 step_fraction=0.5, max_epochs=64)


def test_the_records_of_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, fields in (("tls_event_summary", _lib.EVENT_SUMMARY_FIELDS), ("tls_event_record", _lib.EVENT_RECORD_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
        declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
        assert tuple(declared) == fields, name
    assert "#define TLS_EVENTS_MAX_CHASE 8192" in text
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_events.hip.h")).read()
    assert "constexpr int kEventsMaxChase = 8192;" in kernel
    assert "constexpr int kEventsSummaryWords = 15;" in kernel and "constexpr int kEventsRecordWords = 14;" in kernel
    assert "__syncthreads" not in re.sub(r"//[^\n]*", "", kernel) and "wg_sync();" in kernel
    assert "#pragma clang fp contract(off)" in kernel and "asm" not in re.sub(r"//[^\n]*", "", kernel)


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_event_vetting"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "(8: tls_event_vetting)" in text.split("#define TLS_AMD_ABI_VERSION")[0]   # (the version comment lists the entry)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_event_vetting.argtypes) == declared.count(",") + 1 == 29
    assert declared.endswith("double chase_fraction, double chase_min, double point_fraction, double step_fraction, "
                             "int64_t max_epochs, tls_event_summary *out, tls_event_record *out_events")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_events.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    kernels = open(os.path.join(REPO, "tls_amd", "csrc", "tls_kernels.hip.h")).read()
    assert kernels.index('#include "tls_times.hip.h"') < kernels.index('#include "tls_events.hip.h"')
    assert hasattr(_lib.Context, "event_vetting")


def test_rows():
    """transit_time_rows' four arrays, then chase_reach = min(int(chase_window P / dt), 8192), guard = int(guard L) and
    chase_span = chase_window P -- also where the cap bites."""
    dt = 1 / 64.0
    period = [2.0, 2.0, 0.2, 1.0, numpy.nan, -1.0]
    duration = [5 * dt, 0.5 * dt, 8 * dt, 37.4 * dt, 5 * dt, 5 * dt]
    rows = survey.event_vetting_rows(T, period, duration)
    for got, want in zip(rows[:4], survey.transit_time_rows(T, period, duration)):
        assert numpy.array_equal(got, want)
    assert rows[4].tolist() == [12, 12, 1, 6, 0, 0] and rows[4].dtype == numpy.int64       # (0.1 * 2 d is 12.8 samples)
    assert rows[5].tolist() == [7, 4, 12, 55, 7, 7] and rows[5].dtype == numpy.int64        # (int(1.5 L))
    assert rows[6].tolist() == [0.1 * 2.0, 0.1 * 2.0, 0.1 * 0.2, 0.1 * 1.0, 1.0, 1.0]
    wide = survey.event_vetting_rows(T, [2.0], [5 * dt], 1.0, 0.5, 0.0)
    assert wide[4].tolist() == [64] and wide[5].tolist() == [0] and wide[6].tolist() == [1.0]
    long_t = numpy.arange(20000) * dt
    capped = survey.event_vetting_rows(long_t, [250.0, 1e300], [1.0, 1.0], 1.0, 0.9)
    assert capped[4].tolist() == [8192, 8192] and capped[6].tolist() == [0.9 * 250.0, 0.9 * 1e300]   # (the span stays)
    for bad in (dict(duration=[0.0]), dict(duration=[numpy.nan]), dict(t=T[:2]), dict(t=numpy.ones(10))):
        with pytest.raises(ValueError):
            survey.event_vetting_rows(**dict(dict(t=T, period=[2.0], duration=[0.1]), **bad))


@pytest.mark.parametrize("kw, match", [
    (dict(search=0), "search"), (dict(search=numpy.nan), "search"), (dict(search=True), "search"),
    (dict(min_ses=numpy.nan), "min_ses"), (dict(min_ses=None), "min_ses"),
    (dict(max_epochs=0), "max_epochs"), (dict(max_epochs=65537), "max_epochs"), (dict(max_epochs=2.0), "max_epochs"),
    (dict(gap_tolerance=-0.5), "gap_tolerance"), (dict(transit_depth_min=-1e-6), "depth_min"),
    (dict(chase_window=0), "chase_window"), (dict(chase_window=-0.1), "chase_window"), (dict(chase_window=numpy.nan), "chase_window"),
    (dict(chase_window=numpy.inf), "chase_window"), (dict(chase_window="0.1"), "chase_window"),
    (dict(guard=-1), "guard"), (dict(guard=numpy.nan), "guard"), (dict(guard=numpy.inf), "guard"), (dict(guard=None), "guard"),
    (dict(chase_fraction=0), "chase_fraction"), (dict(chase_fraction=1.01), "chase_fraction"),
    (dict(chase_fraction=numpy.nan), "chase_fraction"), (dict(chase_fraction=True), "chase_fraction"),
    (dict(chase_min=-0.01), "chase_min"), (dict(chase_min=1.01), "chase_min"), (dict(chase_min=numpy.nan), "chase_min"),
    (dict(point_fraction=0), "point_fraction"), (dict(point_fraction=numpy.nan), "point_fraction"),
    (dict(step_fraction=0), "step_fraction"), (dict(step_fraction=-1.0), "step_fraction"),
    (dict(step_fraction=numpy.nan), "step_fraction"), (dict(step_fraction="x"), "step_fraction"),
    (dict(duration=[0.1, 0.0]), "duration"), (dict(period=[1.0]), "n_fits"),
    (dict(curve=[0, 2]), "curve"), (dict(curve=[0.0, 1.0]), "curve"), (dict(curve=[0]), "curve")])
def test_survey_call_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    args = dict(dict(period=[1.0, 1.5], T0=[1.2, 1.3], duration=[0.1, 0.1]), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match) as raised:
            survey.event_vetting(T, flux, **args)
        assert "transit times" not in str(raised.value)
        with pytest.raises(ValueError, match=match):              # (nor is anything detrended first)
            survey.event_vetting(T, flux, detrend=25, **args)
        with pytest.raises(ValueError, match="flux_batch must be"):
            survey.event_vetting(T, flux[:, :-1], [1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
        with pytest.raises(ValueError, match="one candidate a light curve"):
            survey.event_vetting(T, flux, [1.0], [1.2], [0.1])
        with pytest.raises(AssertionError, match="a context was created"):     # (a good call reaches the device)
            survey.event_vetting(T, flux, [1.0, 1.5], [1.2, 1.3], [0.1, 0.001])


@pytest.mark.parametrize("kw, match", [
    (dict(event_vetting=True), "needs peak_fits"), (dict(event_vetting=True, peaks=3), "needs peak_fits"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_search=0), "search"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_chase_window=0), "chase_window"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_guard=-1), "guard"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_min_ses=numpy.nan), "min_ses"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_chase_fraction=1.5), "chase_fraction"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_chase_min=2), "chase_min"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_point_fraction=0), "point_fraction"),
    (dict(event_vetting=True, peaks=3, peak_fits=True, event_vetting_step_fraction=numpy.nan), "step_fraction")])
def test_power_batch_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, **kw)
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, detrend=25, **kw)


GOOD = dict(t=T, y=numpy.ones(300), dy=numpy.ones(300), period=[1.0, 2.0], T0=[1.1, 1.2], row=[0, 1], reach=[1, 5],
            chase_reach=[0, 8192], guard=[0, 10 ** 12], chase_span=[0.1, 0.2], widths=[3, 5], shapes=[numpy.ones(3), numpy.ones(5)],
            span_max=[0.1, 0.2], curve=[0, 0], max_epochs=8)


@pytest.mark.parametrize("kw", [
    dict(row=[0, 2]), dict(reach=[0, 1]), dict(reach=[1, 4097]), dict(curve=[0, 1]), dict(curve=None), dict(T0=[1.0]),
    dict(max_epochs=0), dict(min_ses=numpy.nan), dict(depth_min=-1.0), dict(widths=[2, 5]), dict(t=T[::-1]),
    dict(dy=numpy.zeros(300)), dict(chase_reach=[-1, 0]), dict(chase_reach=[0, 8193]), dict(chase_reach=[0.0, 1.0]),
    dict(chase_reach=[0]), dict(guard=[-1, 0]), dict(guard=[0.5, 1.0]), dict(guard=[1]), dict(chase_span=[0.0, 0.1]),
    dict(chase_span=[0.1, -0.1]), dict(chase_span=[numpy.nan, 0.1]), dict(chase_span=[numpy.inf, 0.1]), dict(chase_span=[0.1]),
    dict(chase_span=["a", "b"]), dict(chase_fraction=0.0), dict(chase_fraction=1.5), dict(chase_fraction=numpy.nan),
    dict(chase_min=-0.1), dict(chase_min=1.5), dict(chase_min=numpy.nan), dict(point_fraction=0.0),
    dict(point_fraction=numpy.nan), dict(step_fraction=0.0), dict(step_fraction=numpy.nan), dict(step_fraction=None)])
def test_event_vetting_arguments_refuses(kw):
    with pytest.raises(ValueError, match="^event vetting: "):
        _lib.event_vetting_arguments(**dict(GOOD, **kw))


def test_event_vetting_arguments_packs():
    a = _lib.event_vetting_arguments(**dict(GOOD, period=[numpy.nan, -1.0], chase_fraction=1, point_fraction=numpy.inf))
    assert a["y"].shape == a["dy"].shape == (1, 300) and a["max_epochs"] == 8 and a["min_ses"] == 3.0
    assert (a["chase_fraction"], a["chase_min"], a["point_fraction"], a["step_fraction"]) == (1.0, 0.5, numpy.inf, 0.5)
    for key in ("curve", "row", "reach", "chase_reach", "guard", "width", "shape_offset"):
        assert a[key].dtype == numpy.int64 and a[key].flags["C_CONTIGUOUS"], key
    for key in ("t", "y", "dy", "period", "T0", "chase_span", "shape_values", "span_max"):
        assert a[key].dtype == numpy.float64 and a[key].flags["C_CONTIGUOUS"], key
    assert a["guard"].tolist() == [0, 10 ** 12] and a["chase_reach"].tolist() == [0, 8192]
    assert _lib.event_vetting_options() == (0.6, 0.5, 0.5, 0.5)
