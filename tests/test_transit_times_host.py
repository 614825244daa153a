"""Transit times without a GPU: the statement (tests/transit_times_spec.py) equals its own loops bit for bit and finds what is
injected -- a linear ephemeris, a sinusoidal timing variation, even widths, a planet too shallow to time; the argument checks
of the Python layer, all raised before any device work; the rows and the reach cap; the field lists; and the header, the
binding and the version comment name tls_transit_times."""
import ctypes
import os
import re
import warnings

import numpy
import pytest

import transit_times_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, transit_model

SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")
T = 1.0 + numpy.arange(300) / 64.0


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


def injected(seed, A, L=5, P=3.7, T0=1.1, rp=0.07, points=1920, gap=(900, 1000), max_epochs=16):
    """(record, epoch rows, ttv of every epoch row) of the statement on one light curve: 30 min cadence with a gap,
    a planet of period P whose transits move by A sin(2 pi e / 6) days, white noise of 3e-4, dy = std(flux)."""
    t = numpy.delete(0.013 + numpy.arange(points) / 48, numpy.arange(*gap))
    e = numpy.round((t - T0) / P)
    ttv = A * numpy.sin(2 * numpy.pi * e / 6)
    flux = transit_model.light_curve(t - ttv, T0, P, rp, 12.0, 89.5, 0, 90, [0.48, 0.19], "quadratic") \
        + numpy.random.default_rng(seed).normal(0, 3e-4, len(t))
    widths, span_max, row, reach = survey.transit_time_rows(t, [P], [L * numpy.median(numpy.diff(t))], 1.0, 0.5)
    assert widths.tolist() == [L] and reach.tolist() == [L] and row.tolist() == [0]
    b = spec.shapes_of([L], **SHAPE)[0]
    eph, rows = spec.transit_times(t, flux, numpy.full(len(t), numpy.std(flux)), P, T0, b, span_max[0], reach[0], 0.0, 3.0,
                                   max_epochs)
    record = dict(zip(spec.EPHEMERIS_FIELDS, eph))
    rows = rows[:int(record["n_epochs"])]
    return record, rows, A * numpy.sin(2 * numpy.pi * rows[:, 0] / 6)


@pytest.mark.parametrize("L", [3, 5, 12, 37])
def test_the_loops_equal_the_vectorised_form(L):
    """A series with a gap, per-point dy, odd and even widths, a candidate whose first and last epochs hang over the ends;
    and candidates of status 1 and 2."""
    rng = numpy.random.default_rng(L)
    t = numpy.delete(T, numpy.arange(140, 170))
    y = 1 + rng.normal(0, 1e-3, len(t))
    for at in range(3, len(t), 45):
        y[at: at + L] -= 4e-3
    dy = rng.uniform(5e-4, 2e-3, len(t))
    b = spec.shapes_of([L], **SHAPE)[0]
    span = (L - 1) / 64.0 * 1.5
    for P, T0, S, min_ses, epochs in ((45 / 64.0, T[3 + L // 2], L, 3.0, 8), (0.61, 0.93, 2, 0.0, 9), (0.2, 1.0, 1, 3.0, 40),
                                      (numpy.nan, 1.0, 1, 3.0, 4), (0.2, 1.0, 1, 3.0, 4), (-1.0, 1.0, 1, 3.0, 4),
                                      (50.0, 0.5, 1, 3.0, 4)):
        fast = spec.transit_times(t, y, dy, P, T0, b, span, S, 1e-4, min_ses, epochs)
        slow = spec.transit_times_loops(t, y, dy, P, T0, b, span, S, 1e-4, min_ses, epochs)
        assert fast[0].tobytes() == slow[0].tobytes() and fast[1].tobytes() == slow[1].tobytes(), (L, P)
        assert fast[0].shape == (12,) and fast[1].shape == (epochs, 8)
    assert slow[0][0] == 2 and numpy.isnan(slow[1]).all()                # (no epoch of 0.5 + 50 e inside the series)
    assert spec.transit_times(t, y, dy, 0.2, 1.0, b, span, 1, max_epochs=4)[0][:2].tolist() == [2.0, 24.0]
    assert spec.transit_times(t, y, dy, numpy.inf, 1.0, b, span, 1)[0][0] == 1


@pytest.mark.parametrize("seed", range(5))
def test_a_linear_ephemeris_is_recovered(seed):
    """A = 0: ten of the eleven epochs are timed; the eleventh lies in the gap and is not: windows beside the gap lie within
    reach and hold noise dips, so the statement reports it as too weak, status 3 (seeds 0 to 4, here and with A = 0.02).  Seeds 0 to 4 on
    the CPU: ttv_chi2 1.3 to 4.8 (8 degrees of freedom), |period - 3.7| at most 1.1e-4 against period_err of 3.0e-4,
    |T0 - 1.1| at most 9.6e-4 against T0_err of 1.8e-3, |time - time_linear| / time_err at most 1.6."""
    record, rows, ttv = injected(seed, 0.0)
    assert record["status"] == 0 and record["n_epochs"] == 11 and record["n_timed"] == 10 and record["epoch_first"] == 0
    assert rows[5, 1] == 3.0 and (numpy.delete(rows[:, 1], 5) == 0).all()
    assert record["ttv_chi2"] < 15
    assert abs(record["period"] - 3.7) < 3 * record["period_err"]
    assert abs(record["T0"] - 1.1) < 3 * record["T0_err"]
    timed = rows[:, 1] == 0
    assert numpy.all(numpy.abs(rows[timed, 3] - rows[timed, 2]) / rows[timed, 4] < 4)
    assert numpy.isnan(rows[5, 3]) and numpy.isnan(rows[5, 4])


@pytest.mark.parametrize("seed", range(5))
def test_a_timing_variation_shows_in_the_table(seed):
    """A = 0.02 d: the line no longer fits -- ttv_chi2 136 to 188 on seeds 0 to 4 -- and every timed epoch follows the
    injected sine within 2.1 time_err."""
    record, rows, ttv = injected(seed, 0.02)
    assert record["n_timed"] == 10 and rows[5, 1] == 3.0 and record["ttv_chi2"] > 60
    timed = rows[:, 1] == 0
    assert numpy.all(numpy.abs(rows[timed, 3] - rows[timed, 2] - ttv[timed]) / rows[timed, 4] < 4)
    assert record["ttv_max_sigma"] > 4 and record["ttv_max_epoch"] in rows[timed, 0]
    assert 0.005 < record["ttv_rms"] < 0.03


@pytest.mark.parametrize("seed", range(5))
def test_an_even_width_reads_its_centre_between_two_samples(seed):
    """L = 12 (P = 9.1, T0 = 2.2, rp = 0.03, 4320 points, samples 2000..2099 removed): the window's centre lies half-way
    between two samples; read half a sample off (0.0104 d), the mean of time - time_linear would show it.  Seeds 0 to 4:
    the mean is at most 0.0047 d in absolute value, ttv_chi2 8.5 to 25.4."""
    record, rows, ttv = injected(seed, 0.0, L=12, P=9.1, T0=2.2, rp=0.03, points=4320, gap=(2000, 2100))
    timed = rows[:, 1] == 0
    assert record["n_timed"] == timed.sum() == 10
    assert abs(numpy.mean(rows[timed, 3] - rows[timed, 2])) < 0.008
    assert record["ttv_chi2"] < 40


@pytest.mark.parametrize("seed", [0, 1])
def test_a_planet_too_shallow_to_time(seed):
    """The same with rp = 0.012: single transits of ses below 3.  Nine of the ten epochs are status 3 and there is no
    ephemeris (seeds 0 and 1: one epoch timed each)."""
    record, rows, ttv = injected(seed, 0.0, L=12, P=9.1, T0=2.2, rp=0.012, points=4320, gap=(2000, 2100))
    assert (rows[:, 1] == 3).sum() >= 9 and record["n_timed"] < 2
    assert numpy.isnan(record["period"]) and numpy.isnan(record["T0"]) and numpy.isnan(record["ttv_chi2"])
    assert numpy.all(rows[rows[:, 1] == 3, 5] < 3.0)


def test_row_constants():
    b = spec.shapes_of([8], **SHAPE)[0]
    b_l, bb, g, gg, bg = spec.row_constants(b)
    assert g[0] == 0.5 * b[1] and g[7] == 0.5 * (0.0 - b[6]) and g[3] == 0.5 * (b[4] - b[2])
    assert gg[2] == g[2] * g[2] and bg[5] == b[5] * g[5] and bb[1] == b[1] * b[1]
    assert abs(sum(g)) < 1e-12                    # (the slopes of a shape that starts and ends at 0 cancel)


# ---- the Python layer -----------------------------------------------------------------------------------------------------
def test_field_lists():
    assert spec.EPHEMERIS_FIELDS == _lib.EPHEMERIS_FIELDS == _lib.EPHEMERIS_DTYPE.names == survey.ephemeris_fields()
    assert spec.TIME_FIELDS == _lib.TRANSIT_TIME_FIELDS == _lib.TRANSIT_TIME_DTYPE.names
    assert survey.transit_time_fields() == spec.TIME_FIELDS + ("oc",)
    assert len(spec.EPHEMERIS_FIELDS) == 12 and len(spec.TIME_FIELDS) == 8
    assert ctypes.sizeof(_lib.Ephemeris) == 96 == _lib.EPHEMERIS_DTYPE.itemsize
    assert ctypes.sizeof(_lib.TransitTime) == 64 == _lib.TRANSIT_TIME_DTYPE.itemsize
    assert (spec.MAX_REACH, spec.MAX_EPOCHS) == (_lib.TIMES_MAX_REACH, _lib.TIMES_MAX_EPOCHS) == (4096, 65536)
    assert [k for k, _ in survey.TRANSIT_TIMES_PEAK_FIELDS] == ["tt_status", "tt_n_timed", "tt_period", "tt_period_err", "tt_T0",
                                                               "tt_T0_err", "tt_chi2", "tt_rms", "tt_max_sigma"]
    assert all(source in spec.EPHEMERIS_FIELDS for _, source in survey.TRANSIT_TIMES_PEAK_FIELDS)


def test_the_records_of_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, fields in (("tls_ephemeris", _lib.EPHEMERIS_FIELDS), ("tls_transit_time", _lib.TRANSIT_TIME_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
        declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
        assert tuple(declared) == fields, name
    assert "#define TLS_TIMES_MAX_REACH 4096" in text and "#define TLS_TIMES_MAX_EPOCHS 65536" in text
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_times.hip.h")).read()
    assert "constexpr int kTimesMaxReach = 4096;" in kernel and "constexpr int kTimesMaxEpochs = 65536;" in kernel
    assert "constexpr int kTimesEphemerisWords = 12;" in kernel and "constexpr int kTimesTimeWords = 8;" in kernel
    assert "__syncthreads" not in re.sub(r"//[^\n]*", "", kernel) and "wg_sync();" in kernel
    assert "#pragma clang fp contract(off)" in kernel


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_transit_times"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert name in text.split("#define TLS_AMD_ABI_VERSION")[0]      # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_transit_times.argtypes) == declared.count(",") + 1 == 22
    assert declared.endswith("double depth_min, double min_ses, int64_t max_epochs, tls_ephemeris *out, tls_transit_time *out_times")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_times.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    assert hasattr(_lib.Context, "transit_times")


def test_rows_and_the_reach_cap():
    """L = clip(int(round(duration / dt)), 3, min(4096, n)); the table is the sorted distinct widths; reach = max(1,
    min(int(search L), (int(P / dt) - 1) // 2, 4096)): two epochs never share a centre."""
    dt = 1 / 64.0
    widths, span_max, row, reach = survey.transit_time_rows(
        T, period=[2.0, 2.0, 0.2, 1.0, 3 * dt, 1000.0, numpy.nan, -1.0], duration=[5 * dt, 0.5 * dt, 8 * dt, 37.4 * dt, 5 * dt,
                                                                                   900.0, 5 * dt, 5 * dt])
    assert widths.tolist() == [3, 5, 8, 37, 300] and widths.dtype == numpy.int64
    assert row.tolist() == [1, 0, 2, 3, 1, 4, 1, 1]                  # (a duration shorter than three samples clips to 3)
    assert reach.tolist() == [5, 3, min(8, (12 - 1) // 2), 31, 1, 300, 1, 1]   # (0.2 d is 12 samples; 1 d is 64: (64-1)//2)
    assert span_max == [(L - 1) * dt * 1.5 for L in (3, 5, 8, 37, 300)]
    assert survey.transit_time_rows(T, [2.0], [5 * dt], search=2.5)[3].tolist() == [12]
    assert survey.transit_time_rows(T, [2.0], [5 * dt], search=0.1)[3].tolist() == [1]
    long_t = numpy.arange(20000) * dt
    assert survey.transit_time_rows(long_t, [250.0], [70.0], search=3.0)[3].tolist() == [4096]      # (the entry's limit)
    assert survey.transit_time_rows(long_t, [250.0], [70.0])[0].tolist() == [4096]
    assert survey.transit_time_rows(T, [2.0], [5 * dt], gap_tolerance=0.0)[1] == [4 * dt]
    for bad in (dict(duration=[0.0]), dict(duration=[numpy.nan]), dict(duration=[numpy.inf]), dict(t=T[:2]),
                dict(t=numpy.ones(10))):
        with pytest.raises(ValueError, match="transit times"):
            survey.transit_time_rows(**dict(dict(t=T, period=[2.0], duration=[0.1]), **bad))


@pytest.mark.parametrize("kw, match", [
    (dict(search=0), "search"), (dict(search=-1.0), "search"), (dict(search=numpy.nan), "search"), (dict(search=numpy.inf), "search"),
    (dict(search="1"), "search"), (dict(search=True), "search"), (dict(min_ses=numpy.nan), "min_ses"), (dict(min_ses=None), "min_ses"),
    (dict(max_epochs=0), "max_epochs"), (dict(max_epochs=65537), "max_epochs"), (dict(max_epochs=2.0), "max_epochs"),
    (dict(gap_tolerance=-0.5), "gap_tolerance"), (dict(transit_depth_min=-1e-6), "depth_min"),
    (dict(transit_depth_min=numpy.inf), "depth_min"), (dict(duration=[0.1, 0.0]), "duration"), (dict(period=[1.0]), "n_fits"),
    (dict(curve=[0, 2]), "curve"), (dict(curve=[0.0, 1.0]), "curve"), (dict(curve=[0]), "curve")])
def test_survey_call_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    args = dict(dict(period=[1.0, 1.5], T0=[1.2, 1.3], duration=[0.1, 0.1]), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.transit_times(T, flux, **args)
        with pytest.raises(ValueError, match=match):              # (nor is anything detrended first)
            survey.transit_times(T, flux, detrend=25, **args)
        with pytest.raises(ValueError, match="flux_batch must be"):
            survey.transit_times(T, flux[:, :-1], [1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
        with pytest.raises(ValueError, match="one candidate a light curve"):
            survey.transit_times(T, flux, [1.0], [1.2], [0.1])
        with pytest.raises(AssertionError, match="a context was created"):     # (a good call reaches the device)
            survey.transit_times(T, flux, [1.0, 1.5], [1.2, 1.3], [0.1, 0.001])


@pytest.mark.parametrize("kw, match", [
    (dict(transit_times=True), "needs peak_fits"), (dict(transit_times=True, peaks=3), "needs peak_fits"),
    (dict(transit_times=True, peaks=3, peak_fits=True, transit_times_search=0), "search"),
    (dict(transit_times=True, peaks=3, peak_fits=True, transit_times_search=numpy.nan), "search"),
    (dict(transit_times=True, peaks=3, peak_fits=True, transit_times_min_ses=numpy.nan), "min_ses")])
def test_power_batch_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, **kw)
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, detrend=25, **kw)


GOOD = dict(t=T, y=numpy.ones(300), dy=numpy.ones(300), period=[1.0, 2.0], T0=[1.1, 1.2], row=[0, 1], reach=[1, 5],
            widths=[3, 5], shapes=[numpy.ones(3), numpy.ones(5)], span_max=[0.1, 0.2], curve=[0, 0], max_epochs=8)


@pytest.mark.parametrize("kw", [
    dict(row=[0, 2]), dict(row=[-1, 0]), dict(row=[0.0, 1.0]), dict(row=[0]), dict(reach=[0, 1]), dict(reach=[1, 4097]),
    dict(reach=[1.0, 2.0]), dict(curve=[0, 1]), dict(curve=[-1, 0]), dict(curve=None), dict(T0=[1.0]), dict(period=[[1.0, 2.0]]),
    dict(max_epochs=0), dict(max_epochs=65537), dict(max_epochs=True), dict(min_ses=numpy.nan), dict(depth_min=-1.0),
    dict(depth_min=numpy.nan), dict(widths=[5, 3], shapes=[numpy.ones(5), numpy.ones(3)]), dict(widths=[2, 5]),
    dict(shapes=[numpy.ones(3), numpy.ones(4)]), dict(span_max=[0.1, numpy.inf]), dict(t=T[::-1]),
    dict(dy=numpy.zeros(300)), dict(y=numpy.full(300, numpy.nan))])
def test_transit_times_arguments_refuses(kw):
    with pytest.raises(ValueError):
        _lib.transit_times_arguments(**dict(GOOD, **kw))


def test_transit_times_arguments_packs():
    a = _lib.transit_times_arguments(**dict(GOOD, period=[numpy.nan, -1.0], min_ses=numpy.int64(2)))
    assert a["y"].shape == a["dy"].shape == (1, 300) and a["max_epochs"] == 8 and a["min_ses"] == 2.0 and a["depth_min"] == 0.0
    assert a["width"].tolist() == [3, 5] and a["shape_offset"].tolist() == [0, 3]
    for key in ("curve", "row", "reach", "width", "shape_offset"):
        assert a[key].dtype == numpy.int64 and a[key].flags["C_CONTIGUOUS"], key
    for key in ("t", "y", "dy", "period", "T0", "shape_values", "span_max"):
        assert a[key].dtype == numpy.float64 and a[key].flags["C_CONTIGUOUS"], key
    assert numpy.isnan(a["period"][0]) and "k" not in a and "separation" not in a
    one = _lib.transit_times_arguments(**dict(GOOD, period=[1.0], T0=[1.0], row=[0], reach=[1], curve=None))
    assert one["curve"].tolist() == [0]


def test_oc_is_formed_on_the_host():
    eph = numpy.zeros(2, dtype=_lib.EPHEMERIS_DTYPE)
    times = numpy.zeros((2, 3), dtype=_lib.TRANSIT_TIME_DTYPE)
    eph["T0"], eph["period"] = [1.0, numpy.nan], [2.0, 3.0]
    times["epoch"], times["time"] = [[0, 1, numpy.nan]] * 2, [[1.5, 3.25, numpy.nan]] * 2
    out = survey._with_oc(eph, times)
    assert out.dtype.names == survey.transit_time_fields() and out.shape == (2, 3)
    assert out["oc"][0, :2].tolist() == [0.5, 0.25] and numpy.isnan(out["oc"][0, 2]) and numpy.isnan(out["oc"][1]).all()
    assert numpy.array_equal(out["time"], times["time"], equal_nan=True)


def test_the_shared_checks_speak_of_transit_times_and_take_the_entry_s_n():
    """t, y, dy and the rows go through single_arguments' checks under this entry's name and with its own limit of n."""
    for kw in (dict(t=T[::-1]), dict(widths=[2, 5]), dict(dy=numpy.zeros(300)), dict(shapes=[numpy.ones(3), numpy.ones(4)]),
               dict(y=numpy.ones(299)), dict(span_max=[0.1, numpy.inf]), dict(widths=[3.0, 5])):
        with pytest.raises(ValueError, match="^transit times: "):
            _lib.transit_times_arguments(**dict(GOOD, **kw))
    with pytest.raises(ValueError, match="^single transits: "):
        _lib.single_arguments(T[::-1], GOOD["y"], GOOD["dy"], GOOD["widths"], GOOD["shapes"], GOOD["span_max"])
    n = _lib.SINGLE_MAX_POINTS + 1
    assert _lib.TIMES_MAX_POINTS == 1 << 30
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_times.hip.h")).read()
    assert "constexpr int kTimesMaxPoints = 1 << 30;" in kernel
    long_t = numpy.arange(n) / 64.0
    a = _lib.transit_times_arguments(**dict(GOOD, t=long_t, y=numpy.ones(n), dy=numpy.ones(n)))
    assert a["y"].shape == (1, n)
    with pytest.raises(ValueError, match="^single transits: t must have shape"):
        _lib.single_arguments(long_t, numpy.ones(n), numpy.ones(n), GOOD["widths"], GOOD["shapes"], GOOD["span_max"])
