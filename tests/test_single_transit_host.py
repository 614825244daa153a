"""Single-transit events without a GPU: the host statement (tests/single_transit_spec.py) recovers injected single transits
and equals its own double loop bit for bit; the default width grid; the argument checks of _lib.single_arguments and
survey.single_transits before any device work; tls_single_event and the entry in the header, the binding and the library."""
import ctypes
import os
import re
import warnings

import numpy
import pytest

import single_transit_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, transit_model
from tls_amd.template import reference_transit

SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")


def gapped(n, gap_at, gap):
    """n time stamps at 30 min with `gap` cadences missing in front of index gap_at."""
    t = 1.0 + numpy.arange(n + gap) / 48.0
    return numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def rows_of(t, widths, gap_tolerance=0.5):
    dt = float(numpy.median(numpy.diff(t)))
    return spec.shapes_of(widths, **SHAPE), [(int(L) - 1) * dt * (1 + gap_tolerance) for L in widths]


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


@pytest.mark.parametrize("seed", range(5))
def test_the_statement_recovers_injected_single_transits(seed):
    """1920 points at 30 min with a 60-point gap, noise of 3e-4 and two single transits (rp 0.07 and 0.06, 15 and 19 samples
    in transit) shorter than the longest row (48): they are ranks 1 and 2, each within half its width of its time, and rank 3
    stays below a third of rank 2.  (Seeds 0 to 4 with the statement on the CPU, dy = std(y) with the transits in it: ses of
    rank 1 / 2 / 3 = 29.6-30.2 / 24.4-25.3 / 1.5-2.0, rank 3 / rank 2 = 0.06-0.08; all five seeds hold.)"""
    t = gapped(1920, 700, 60)
    t0 = (t[400], t[1400])
    y = numpy.ones(len(t))
    y += transit_model.light_curve(t, t0[0], 40.0, 0.07, 45.0, 89.9, 0, 90, [0.4, 0.3], "quadratic") - 1
    y += transit_model.light_curve(t, t0[1], 80.0, 0.06, 70.0, 89.95, 0, 90, [0.4, 0.3], "quadratic") - 1
    in_transit = [int(((y < 1) & (abs(t - c) < 1)).sum()) for c in t0]
    assert max(in_transit) < 48
    y += numpy.random.RandomState(seed).normal(0, 3e-4, len(t))
    widths = survey.single_transit_widths(t)
    shapes, span = rows_of(t, widths)
    events, n_events, ses, row, depth = spec.expected(t, y, numpy.full(len(t), numpy.std(y)), widths, shapes, span)
    ev = events[0]
    print("seed %d: in transit %s, ses %s, widths %s, depths %s" % (seed, in_transit, ev["ses"][:4], ev["width"][:4], ev["depth"][:4]))
    assert n_events[0] >= 3
    dt = 1 / 48.0
    for rank, c in enumerate(t0):
        assert abs(ev["time"][rank] - c) <= 0.5 * ev["width"][rank] * dt, rank
    assert ev["ses"][2] < ev["ses"][1] / 3
    assert numpy.all(numpy.diff(ev["ses"][:n_events[0]]) <= 0)
    # no window runs over the gap
    assert numpy.all((ev["t_last"] - ev["t_first"])[:n_events[0]] <= 1.5 * (ev["width"][:n_events[0]] - 1) * dt)


def test_the_double_loop_equals_the_vectorised_form():
    """One curve with a gap, per-point dy and an even and an odd row wider than an island: every plane bit for bit."""
    rng = numpy.random.RandomState(7)
    t = gapped(300, 120, 9)
    y = 1 + rng.normal(0, 1e-3, len(t))
    y[40:52] -= 3e-3
    dy = rng.uniform(0.5, 2.0, len(t)) * 1e-3
    widths = [3, 4, 5, 8, 37, 64, 200]
    shapes, span = rows_of(t, widths)
    fast = spec.statistic(t, y, dy, widths, shapes, span, 1e-4)
    slow = spec.statistic_loops(t, y, dy, widths, shapes, span, 1e-4)
    for a, b, name in zip(fast, slow, ("ses", "row", "depth")):
        numpy.testing.assert_array_equal(a, b, err_msg=name)
    assert (fast[1] >= 0).sum() > 100 and (fast[1] < 0).sum() > 10 and len(set(fast[1].tolist())) > 4
    both = spec.statistic(t, numpy.array([y, y[::-1]]), numpy.array([dy, dy]), widths, shapes, span, 1e-4)
    for a, b in zip(both, fast):
        numpy.testing.assert_array_equal(a[0], b)


def test_selection_by_hand():
    """Five centres with rows of width 3 and 5: ties go to the lowest index, the guard is int(separation * L), windows that
    only touch count as meeting."""
    t = numpy.arange(14.0)
    nan = numpy.nan
    # windows: 1 -> [0, 2], 4 -> [3, 5], 7 -> [5, 9] (width 5), 9 -> [8, 10], 12 -> [11, 13]
    ses = numpy.array([nan, 5.0, nan, nan, 5.0, nan, nan, 4.0, nan, 3.0, nan, nan, 6.0, nan])
    row = numpy.array([-1, 0, -1, -1, 0, -1, -1, 1, -1, 0, -1, -1, 0, -1])
    depth = numpy.where(row >= 0, 1e-3, nan)
    # no guard: 12; 1 before 4 (a tie); 4, whose window [3, 5] meets 7's at sample 5; 9
    ev, count = spec.select(t, ses, row, depth, [3, 5], k=8, separation=0.0)
    assert count == 4 and ev["index"][:4].tolist() == [12, 1, 4, 9] and ev["index"][4] == -1 and numpy.isnan(ev["ses"][4])
    assert ev["ses"][:4].tolist() == [6.0, 5.0, 5.0, 3.0] and ev["time"][:4].tolist() == [12.0, 1.0, 4.0, 9.0]
    # g = int(0.5 * 3) = 1: 12 clears [10, 14] and with it 9; 1 clears [-1, 3] and with it 4; 7 is left
    ev, count = spec.select(t, ses, row, depth, [3, 5], k=8, separation=0.5)
    assert ev["index"][:count].tolist() == [12, 1, 7]
    assert (ev["t_first"][2], ev["t_last"][2], ev["width"][2], ev["row"][2], ev["depth"][2]) == (5, 9, 5, 1, 1e-3)
    ev, count = spec.select(t, ses, row, depth, [3, 5], k=2, separation=0.0)
    assert count == 2 and ev["index"].tolist() == [12, 1]
    ev, count = spec.select(t, ses, row, depth, [3, 5], k=8, min_ses=4.5, separation=0.0)
    assert ev["index"][:count].tolist() == [12, 1, 4]
    ev, count = spec.select(t, ses, row, depth, [3, 5], k=8, separation=1e300)
    assert ev["index"][:count].tolist() == [12]


def test_known_width_grids():
    t30 = numpy.arange(4320) / 48.0
    grid = survey.single_transit_widths(t30)
    assert grid.tolist() == [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 17, 18, 20, 22, 24, 27, 30, 33, 36, 39, 43, 48]
    assert grid.dtype == numpy.int64
    assert survey.single_transit_widths(t30, duration_min=0.25, duration_max=0.5, log_step=1.5).tolist() == [12, 18]
    assert survey.single_transit_widths(t30, duration_min=0.5, duration_max=0.5).tolist() == [24]
    assert survey.single_transit_widths(t30, log_step=2.0, duration_max=0.3).tolist() == [3, 6, 12]
    # a gap does not move the median cadence
    assert survey.single_transit_widths(gapped(1920, 700, 60)).tolist() == grid.tolist()


def test_the_width_grid_is_capped():
    t2 = numpy.arange(20000) / 720.0                                   # 2 min: duration_max = 10 d is 7200 samples
    grid = survey.single_transit_widths(t2, duration_min=5.0, duration_max=10.0)
    assert grid[0] == 3600 and grid[-1] <= 4096 and grid[-1] == int(round(3600 * 1.1))
    assert survey.single_transit_widths(t2, duration_min=4096 / 720.0, duration_max=10.0).tolist() == [4096]
    short = numpy.arange(20) / 48.0                                    # 20 points: no row wider than the series
    assert survey.single_transit_widths(short).max() <= 20
    assert survey.single_transit_widths(short, log_step=20 / 3.0).tolist() == [3, 20]


def test_an_empty_width_grid_raises():
    t30 = numpy.arange(4320) / 48.0
    with pytest.raises(ValueError, match="no trial width"):
        survey.single_transit_widths(t30, duration_max=0.05)           # 2.4 samples
    with pytest.raises(ValueError, match="no trial width"):
        survey.single_transit_widths(t30, duration_min=2.0, duration_max=1.0)
    with pytest.raises(ValueError, match="no trial width"):
        survey.single_transit_widths(numpy.arange(20000) / 720.0, duration_min=6.0, duration_max=10.0)    # beyond 4096
    with pytest.raises(ValueError, match="no trial width"):
        survey.single_transit_widths(numpy.arange(2) / 48.0)
    with pytest.raises(ValueError, match="log_step"):
        survey.single_transit_widths(t30, log_step=1.0)
    with pytest.raises(ValueError, match="cadence"):
        survey.single_transit_widths(numpy.zeros(10))


T = 1.0 + numpy.arange(200) / 48.0             # (t > 0: the cleaning of a search drops a time stamp of 0)
Y = numpy.ones((2, 200))
DY = numpy.full((2, 200), 1e-3)
GOOD = dict(widths=[3, 5], shapes=[numpy.ones(3), numpy.ones(5)], span_max=[0.1, 0.2])


@pytest.mark.parametrize("kw", [
    dict(widths=[5, 3], shapes=[numpy.ones(5), numpy.ones(3)]), dict(widths=[3, 3], shapes=[numpy.ones(3), numpy.ones(3)]),
    dict(widths=[2, 5], shapes=[numpy.ones(2), numpy.ones(5)]), dict(widths=[3, 4097], shapes=[numpy.ones(3), numpy.ones(4097)]),
    dict(widths=[3.0, 5]), dict(widths=[True, 5]), dict(widths=[], shapes=[], span_max=[]),
    dict(shapes=[numpy.ones(3)]), dict(shapes=[numpy.ones(3), numpy.ones(4)]),
    dict(shapes=[numpy.ones(3), numpy.array([1, 1, numpy.nan, 1, 1])]),
    dict(span_max=[0.1]), dict(span_max=[0.1, -0.2]), dict(span_max=[0.1, numpy.inf]), dict(span_max=[numpy.nan, 0.2]),
    dict(k=0), dict(k=33), dict(k=2.0), dict(k=True),
    dict(depth_min=-1e-9), dict(depth_min=numpy.inf), dict(depth_min=numpy.nan), dict(depth_min="0"),
    dict(separation=-0.1), dict(separation=numpy.inf), dict(separation=numpy.nan),
    dict(min_ses=numpy.nan), dict(min_ses="3"),
    dict(t=T[::-1]), dict(t=numpy.where(numpy.arange(200) == 7, numpy.nan, T)), dict(t=T[:-1]), dict(t=T[None, :]),
    dict(dy=numpy.where(numpy.arange(200) == 7, 0.0, DY)), dict(dy=DY[:1]), dict(y=numpy.where(numpy.arange(200) == 7, numpy.inf, Y)),
])
def test_single_arguments_refuses(kw):
    args = dict(GOOD, t=T, y=Y, dy=DY)
    args.update(kw)
    with pytest.raises(ValueError, match="single transits"):
        _lib.single_arguments(**args)


def test_single_arguments_packs():
    b = [numpy.array([0.0, 1.0, 0.0]), numpy.array([0.0, 0.5, 1.0, 0.5, 0.0])]
    a = _lib.single_arguments(T, Y[0], DY[0], [3, 5], b, [0.1, 0.2], k=numpy.int64(4), min_ses=None)
    assert a["y"].shape == a["dy"].shape == (1, 200) and a["k"] == 4 and a["min_ses"] == -numpy.inf
    assert a["width"].tolist() == [3, 5] and a["shape_offset"].tolist() == [0, 3] and a["width"].dtype == numpy.int64
    numpy.testing.assert_array_equal(a["shape_values"], numpy.concatenate(b))
    assert (a["depth_min"], a["separation"]) == (0.0, 0.5)
    for key in ("t", "y", "dy", "shape_values", "span_max"):
        assert a[key].dtype == numpy.float64 and a[key].flags["C_CONTIGUOUS"], key


@pytest.mark.parametrize("kw, match", [
    (dict(widths=[5, 3]), "strictly ascending"), (dict(widths=[2, 3]), "every width"), (dict(k=0), "k must be"),
    (dict(k=33), "k must be"), (dict(separation=-1), "separation"), (dict(transit_depth_min=-1e-6), "depth_min"),
    (dict(gap_tolerance=-0.5), "gap_tolerance"), (dict(gap_tolerance=numpy.inf), "gap_tolerance"),
    (dict(min_ses=numpy.nan), "min_ses"), (dict(widths=[3, 201]), None)])
def test_survey_call_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, 200))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if match is None:                       # (a row wider than the series is no error: it has no valid centre)
            with pytest.raises(AssertionError, match="a context was created"):
                survey.single_transits(T, flux, **kw)
        else:
            with pytest.raises(ValueError, match=match):
                survey.single_transits(T, flux, **kw)
            with pytest.raises(ValueError, match=match):          # (nor is anything detrended first)
                survey.single_transits(T, flux, detrend=25, **kw)
        with pytest.raises(ValueError, match="flux_batch must have shape"):
            survey.single_transits(T, flux[:, :-1])


def test_event_fields():
    assert spec.FIELDS == _lib.SINGLE_EVENT_FIELDS == _lib.SINGLE_EVENT_DTYPE.names
    assert survey.single_event_fields() == spec.FIELDS + ("duration_days",)
    assert (spec.MAX_WIDTH, spec.MAX_K) == (_lib.SINGLE_MAX_WIDTH, _lib.SINGLE_MAX_K) == (4096, 32)
    b = spec.shapes_of([9], **SHAPE)[0]
    numpy.testing.assert_array_equal(b, 1.0 - reference_transit(9, **SHAPE))
    assert b.max() == 1.0 and b[4] == 1.0 and 0.0 <= b[0] < 1e-3         # (1 at the bottom, 0 out of transit)


def test_tls_single_event_is_eight_doubles():
    assert ctypes.sizeof(_lib.SingleEvent) == 8 * 8 == _lib.SINGLE_EVENT_DTYPE.itemsize
    assert tuple(n for n, _ in _lib.SingleEvent._fields_) == _lib.SINGLE_EVENT_FIELDS
    assert [_lib.SINGLE_EVENT_DTYPE.fields[k][1] for k in _lib.SINGLE_EVENT_DTYPE.names] == list(range(0, 64, 8))
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct tls_single_event \{(.*?)\} tls_single_event;", code, flags=re.S).group(1)
    declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
    assert tuple(declared) == _lib.SINGLE_EVENT_FIELDS
    assert "#define TLS_SINGLE_MAX_WIDTH 4096" in text and "#define TLS_SINGLE_MAX_K 32" in text
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_single.hip.h")).read()
    assert "constexpr int kSingleTile = %d;" % _lib.SINGLE_TILE in kernel
    assert "constexpr int kSingleMinWidth = %d, kSingleMaxWidth = %d;" % (_lib.SINGLE_MIN_WIDTH, _lib.SINGLE_MAX_WIDTH) in kernel
    assert "constexpr int kSingleMaxPoints = 1 << 20;" in kernel and _lib.SINGLE_MAX_POINTS == 1 << 20
    assert "constexpr int kSingleEventWords = 8;" in kernel and "constexpr int kSingleMaxK = 32;" in kernel


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_single_transits"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert name in text.split("#define TLS_AMD_ABI_VERSION")[0]      # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_single_transits.argtypes) == declared.count(",") + 1 == 20
    assert declared.endswith("tls_single_event *out_events, int64_t *out_n_events, double *out_ses, int64_t *out_row, double *out_depth")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_single.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
