"""The host layer's argument checks as a table of cases, GPU-free: per checked function one valid call at the smallest
shapes and one mutation per refusal -- a bool, a string, a NaN, an infinity, one past a bound, a wrong rank, length or dtype,
curve=None with a mismatched count, two bad arguments at once (the order of refusal).  tools/record_host_refusals.py ran the
table once, at the commit named in tests/golden/host_refusals.json, and tests/test_host_refusals.py replays it: what is
refused, with which message, and what an accepted call returns, stays as recorded.

A case is (id, function, keyword arguments); describe() is the record of one call."""
import types

import numpy

from tls_amd import _lib, survey

NAN, INF = float("nan"), float("inf")
T = numpy.arange(4.0)
Y = numpy.array([[1.0, 0.9, 1.0, 1.1], [1.0, 1.0, 0.8, 1.2]])
DY = numpy.full((2, 4), 0.1)
WIDTHS, SHAPES, SPANS = [3, 4], [[0.1, 0.2, 0.1], [0.1, 0.2, 0.2, 0.1]], [3.0, 4.0]
K_ROWS, PROFILE, SUB = [0.05, 0.1], [[0.0, 0.5, 1.0], [0.0, 0.6, 1.2]], [-0.01, 0.01]
# the series checks: the short lists go to every stage, the long ones to the stages that own a kind of check
BAD_T = [("t 2-D", dict(t=[[0.0, 1.0]])), ("t NaN", dict(t=[0.0, 1.0, NAN, 3.0]))]
BAD_Y = [("y short", dict(y=Y[:, :3])), ("y NaN", dict(y=numpy.where(Y > 1.1, NAN, Y)))]
BAD_DY = [("dy shape", dict(dy=DY[:1])), ("dy zero", dict(dy=numpy.where(Y > 1.1, 0.0, DY)))]
NO_DY = [("dy None", dict(dy=None))]
MORE_SERIES = [("t descending", dict(t=[0.0, 1.0, 3.0, 2.0])), ("y 3-D", dict(y=Y[None])),
               ("y inf", dict(y=numpy.where(Y > 1.1, INF, Y))), ("dy inf", dict(dy=numpy.where(Y > 1.1, INF, DY))),
               ("dy NaN", dict(dy=numpy.where(Y > 1.1, NAN, DY)))]
ONE_ROW = [("one row", dict(y=Y[0], dy=DY[0], curve=[0, 0]))]
BAD_CANDIDATES = [("period string", dict(period=["a", "b"])), ("T0 short", dict(T0=[0.5])),
                  ("period 2-D", dict(period=[[2.0, 3.0]], T0=[[0.5, 1.0]], duration=[[0.2, 0.3]])),
                  ("curve None, 1 candidate", dict(period=[2.0], T0=[0.5], duration=[0.2], curve=None)),
                  ("curve short", dict(curve=[0])), ("curve float", dict(curve=[0.0, 1.0])),
                  ("curve negative", dict(curve=[-1, 0])), ("curve past", dict(curve=[0, 2])),
                  ("curve given", dict(curve=numpy.array([1, 0], dtype=numpy.int32)))]
SOME_CANDIDATES = [BAD_CANDIDATES[i] for i in (0, 1, 3, 7)]
ROWS = [("widths float", dict(widths=[3.0, 4.0])), ("widths bool", dict(widths=[True, 4])), ("widths none", dict(widths=[], shapes=[], span_max=[])),
        ("widths small", dict(widths=[2, 4])), ("widths large", dict(widths=[3, 4097])), ("widths equal", dict(widths=[3, 3], shapes=[SHAPES[0]] * 2)),
        ("shapes short", dict(shapes=SHAPES[:1])), ("shape length", dict(shapes=[SHAPES[0], SHAPES[0]])),
        ("shape NaN", dict(shapes=[[0.1, NAN, 0.1], SHAPES[1]])), ("span short", dict(span_max=[3.0])),
        ("span inf", dict(span_max=[3.0, INF])), ("span negative", dict(span_max=[-1.0, 4.0]))]


def number(name, *more):
    """The usual bad scalars of `name`, and `more` of its own."""
    return [("%s %r" % (name, v), {name: v}) for v in (True,) + more]


def integer(name, *more):
    return [("%s %r" % (name, v), {name: v}) for v in (True,) + more]


def column(name, *more):
    """The usual bad per-candidate integer columns of `name` [2], and `more` of its own."""
    return [("%s %r" % (name, v), {name: v}) for v in ([0],) + more]


def _context_phase_scan(**kw):
    """Context.phase_scan on a stand-in for the library: its checks, and the packed record array of an accepted call."""
    fake = types.SimpleNamespace(_h=None, _check=lambda rc: None, _lib=types.SimpleNamespace(tls_phase_scan=lambda *a: 0))
    return _lib.Context.phase_scan(fake, **kw)


def _refused_only(call, **more):
    """A survey entry whose accepted call goes on to the device or takes long: the table holds its refusals only."""
    def run(**kw):
        call(**more, **kw)
    return run


NO_DEVICE = dict(context=types.SimpleNamespace())
PLANETS = numpy.zeros(3, dtype=[(k, "f8") for k in _lib.REMOVE_TRANSITS_FIELDS])
EVENTS = numpy.zeros(2, dtype=[(k, "f8") for k in ("index", "ses", "depth", "width", "row")])


SERIES = dict(t=T, y=Y, dy=DY)
CANDIDATES = dict(period=[2.0, 3.0], T0=[0.5, 1.0], duration=[0.2, 0.3], curve=None)
SINGLE = dict(SERIES, widths=WIDTHS, shapes=SHAPES, span_max=SPANS)
TIMES = dict(SINGLE, period=[2.0, 3.0], T0=[0.5, 1.0], row=[0, 1], reach=[1, 2])
VETTING = dict(TIMES, chase_reach=[4, 5], guard=[1, 2], chase_span=[1.0, 1.5])
PERIODS = dict(SINGLE, curve=[0, 1], index_a=[0, 1], index_b=[2, 3], row=[0, 1], reach=[1, 2], offset=[0.0, 0.5], period_min=1.0)
SHAPE_TABLES = dict(ratios=[0.5, 1.0], ingress=[0.0, 0.5], shifts=[-0.1, 0.1])
FIT_TABLES = dict(k_rows=K_ROWS, profile=PROFILE, impacts=[0.0, 0.5], ratios=[0.5, 1.0], shifts=[-0.1, 0.1], sub=SUB)
REMOVE = dict(t=T, y=Y, period=[2.0, 3.0], T0=[0.5, 1.0], row=[0, 1], amplitude=[1.0, 1.0], b=[0.1, 0.2], duration=[0.2, 0.3],
              shift=[0.0, 0.0], k_rows=K_ROWS, profile=PROFILE, sub=SUB)
MATCH = dict(star=[0, 1], period=[2.0, 3.0], T0=[0.5, 1.0], duration=[0.2, 0.3], strength=[9.0, 8.0], span=30.0)
SURVEY_CANDIDATES = dict(t=T, flux_batch=Y, period=[2.0, 3.0], T0=[0.5, 1.0], duration=[0.2, 0.3])
VETTING_OPTIONS = dict(search=1.0, chase_window=0.1, guard=1.0, min_ses=3.0, chase_fraction=0.6, chase_min=0.5,
                       point_fraction=0.5, step_fraction=0.5)
SURVEY_ROWS = [("flux 3-D", dict(flux_batch=Y[None])), ("flux short", dict(flux_batch=Y[:, :3])), ("t 2-D", dict(t=[T])),
               ("t NaN", dict(t=[0.0, 1.0, NAN, 3.0])), ("t descending", dict(t=T[::-1]))]
TABLE = [("ratios string", dict(ratios=["a"])), ("ratios 2-D", dict(ratios=[[0.5, 1.0]])), ("shifts empty", dict(shifts=[])),
         ("ratios NaN", dict(ratios=[0.5, NAN])), ("shifts descending", dict(shifts=[0.1, -0.1])), ("ratio zero", dict(ratios=[0.0, 1.0]))]
WINDOW = number("window", INF, 0.5) + integer("min_count", 0)

# (name, function, the valid call, [(label, the arguments that differ)])
STAGES = [
    ("phase_scan_arguments", _lib.phase_scan_arguments, dict(max_bins=16, min_count=1),
     [("max_bins True", dict(max_bins=True)), ("max_bins 16.0", dict(max_bins=16.0)), ("min_count '1'", dict(min_count="1")),
      ("max_bins 15", dict(max_bins=15)), ("max_bins 4097", dict(max_bins=4097)), ("min_count 0", dict(min_count=0)),
      ("min_count 2^31", dict(min_count=2 ** 31)), ("numpy integers", dict(max_bins=numpy.int64(4096), min_count=numpy.int32(3))),
      ("both", dict(max_bins=15, min_count=0))]),
    ("Context.phase_scan", _context_phase_scan, dict(t=T, y=Y, **CANDIDATES),
     [("max_bins 15", dict(max_bins=15)), ("y short", dict(y=Y[:, :3])), ("t empty", dict(t=[], y=[])), ("t 2-D", dict(t=[T])),
      ("t inf", dict(t=[0.0, 1.0, 2.0, INF])), ("one row", dict(y=Y[0], curve=[0, 0])), ("T0 short", dict(T0=[0.5])),
      ("period string", dict(period=["a", "b"])), ("period 2-D", dict(period=[[2.0, 3.0]], T0=[[0.5, 1.0]], duration=[[0.2, 0.3]])),
      ("curve None, 1 fit", dict(period=[2.0], T0=[0.5], duration=[0.2])), ("curve short", dict(curve=[0])),
      ("curve negative", dict(curve=[-1, 0])), ("curve past", dict(curve=[0, 2])), ("y short, t inf", dict(y=Y[:, :3], t=numpy.full(4, INF)))]),
    ("ephemeris_match_arguments", _lib.ephemeris_match_arguments, MATCH,
     number("span", 0.0, INF) + number("drift_tolerance", -1.0, INF) + number("epoch_tolerance", -1.0, INF)
     + integer("max_ratio", 0, 65) + [("star float", dict(star=[0.0, 1.0])), ("star huge", dict(star=numpy.array([2 ** 63, 1], dtype=numpy.uint64))),
                                      ("period string", dict(period=["a", "b"])), ("star 2-D", dict(star=[[0, 1]])),
                                      ("T0 short", dict(T0=[0.5])), ("none", dict(star=[], period=[], T0=[], duration=[], strength=[])),
                                      ("too many", dict({k: numpy.zeros((1 << 20) + 1) for k in ("period", "T0", "duration", "strength")},
                                                        star=numpy.zeros((1 << 20) + 1, dtype=numpy.int64))),
                                      ("span and max_ratio", dict(span=0.0, max_ratio=0)), ("scalars", dict(star=1, period=2.0, T0=0.5, duration=0.2, strength=9.0))]),
    ("noise_arguments", _lib.noise_arguments, dict(t=T, y=Y, widths=[1, 3], span_max=[0.0, 2.5], pair_span=1.5),
     [("t None", dict(t=None)), ("one row", dict(y=Y[0])), ("y string", dict(y=["a"])), ("y 3-D", dict(y=Y[None])),
      ("t 2-D", dict(t=[T])), ("y short", dict(y=Y[:, :3])), ("n 2", dict(t=T[:2], y=Y[:, :2])), ("t NaN", dict(t=[0.0, 1.0, NAN, 3.0])),
      ("t descending", dict(t=T[::-1])), ("y NaN", dict(y=numpy.where(Y > 1.1, NAN, Y))), ("widths 2-D", dict(widths=[[1, 3]])),
      ("widths none", dict(widths=[], span_max=[])), ("widths whole floats", dict(widths=[1.0, 3.0])), ("widths 1.5", dict(widths=[1.5, 3.0])),
      ("widths bool", dict(widths=[True, False])), ("width 0", dict(widths=[0, 3])), ("width 5", dict(widths=[1, 5])),
      ("widths equal", dict(widths=[3, 3])), ("span string", dict(span_max=["a", "b"])), ("span short", dict(span_max=[1.0])),
      ("span negative", dict(span_max=[-1.0, 1.0])), ("span NaN", dict(span_max=[NAN, 1.0])), ("span inf", dict(span_max=[INF, INF]))]
     + number("pair_span", -1.0, INF) + number("clip_upper", -1.0) + number("clip_lower", -1.0) + integer("min_count", 0, 2 ** 31)
     + [("y NaN and min_count", dict(y=numpy.where(Y > 1.1, NAN, Y), min_count=0))]),
    ("single_widths", _lib.single_widths, dict(widths=[3, 4]), [(k, v) for k, v in ROWS if list(v) == ["widths"]] + [("heading", dict(what="x"))]),
    ("single_options", _lib.single_options, dict(),
     integer("k", 0, 33, 2.0, numpy.True_, "1") + number("depth_min", -1.0, INF, NAN, numpy.True_, "1") + number("separation", -1.0, INF)
     + number("min_ses", -INF, numpy.True_, "1")
     + [("min_ses None", dict(min_ses=None)), ("k and depth_min", dict(k=0, depth_min=-1.0))]),
    ("single_arguments", _lib.single_arguments, SINGLE,
     BAD_T + BAD_Y + BAD_DY + NO_DY + MORE_SERIES + ROWS + [("one row", dict(y=Y[0], dy=DY[0])), ("one row 2-D, dy 1-D", dict(y=Y[:1], dy=DY[0])), ("one row, dy 2-D", dict(y=Y[0], dy=DY[:1])),
                                      ("t empty", dict(t=[], y=[], dy=[])), ("max_points 5", dict(max_points=5)),
                                      ("heading", dict(what="x", t=[[0.0]])), ("k 0", dict(k=0)), ("depth_min -1", dict(depth_min=-1.0)),
                                      ("t NaN and k", dict(t=T * NAN, k=0)), ("y NaN and dy zero", dict(y=Y * NAN, dy=DY * 0.0))]),
    ("transit_times_options", _lib.transit_times_options, dict(),
     number("depth_min", -1.0, INF) + number("min_ses", NAN) + integer("max_epochs", 0, 65537) + [("all three", dict(depth_min=-1.0, min_ses=NAN, max_epochs=0))]),
    ("transit_times_arguments", _lib.transit_times_arguments, TIMES,
     BAD_T[:1] + BAD_DY[1:] + NO_DY + ROWS[:1] + column("row", [0, 2], [-1, 0], [1.0, 1.0], [[0, 1]]) + column("reach", [0, 1], [1, 4097])
     + [(k, {a: b for a, b in v.items() if a != "duration"}) for k, v in SOME_CANDIDATES]
     + [("one row", dict(y=Y[0], dy=DY[0], curve=[0, 0])), ("none", dict(period=[], T0=[], row=[], reach=[], curve=[])),
        ("depth_min -1", dict(depth_min=-1.0)), ("max_epochs 0", dict(max_epochs=0)), ("min_ses NaN and t", dict(min_ses=NAN, t=[[0.0]])),
        ("row and reach", dict(row=[0, 2], reach=[0, 1])), ("t and period", dict(t=T[::-1], period=["a", "b"]))]),
    ("event_periods_options", _lib.event_periods_options, dict(period_min=1.0),
     number("period_min", 0.0, INF, NAN, numpy.True_, "1") + integer("max_aliases", 0, 4097) + number("min_ses", NAN) + number("veto_sigma", NAN)
     + [("veto_sigma inf", dict(veto_sigma=INF)), ("both", dict(period_min=0.0, max_aliases=0))]),
    ("event_periods_arguments", _lib.event_periods_arguments, PERIODS,
     BAD_T[:1] + BAD_DY[1:] + NO_DY + ROWS[:1] + column("curve", [0, 2], [-1, 0], [[1, 1]]) + column("index_a", [0, 4]) + column("index_b", [3, 4])
     + column("row", [0, 2]) + column("reach", [0, 1], [1, 4097])
     + [("period_min tiny", dict(period_min=1e-5)), ("period_min 0", dict(period_min=0.0)), ("max_points", dict(t=numpy.zeros((1 << 20) + 1))),
        ("index order", dict(index_a=[2, 1], index_b=[2, 3])), ("offset string", dict(offset=["a", "b"])), ("offset short", dict(offset=[0.0])),
        ("offset negative", dict(offset=[-1.0, 0.0])), ("offset inf", dict(offset=[INF, 0.0])), ("none", dict(curve=[], index_a=[], index_b=[], row=[], reach=[], offset=[])),
        ("scalars", dict(curve=0, index_a=0, index_b=3, row=0, reach=1, offset=0.0)), ("curve 2-D", dict(curve=[[0, 1]], index_a=[[0, 1]])),
        ("t and curve", dict(t=T[::-1], curve=[0, 2])), ("min_ses NaN and t", dict(min_ses=NAN, t=[[0.0]]))]),
    ("event_vetting_options", _lib.event_vetting_options, dict(),
     number("chase_fraction", 0.0, 1.5, NAN, numpy.True_, "1") + number("chase_min", -0.5, 1.5) + number("point_fraction", 0.0, NAN, "1")
     + number("step_fraction", 0.0)
     + [("inf", dict(point_fraction=INF, step_fraction=INF)), ("both", dict(chase_fraction=0.0, chase_min=2.0))]),
    ("event_vetting_arguments", _lib.event_vetting_arguments, VETTING,
     BAD_T[:1] + BAD_DY[1:] + NO_DY + ROWS[:1] + column("row", [0, 2]) + column("reach", [0, 1]) + column("chase_reach", [-1, 0], [0, 8193])
     + column("guard", [-1, 0]) + [(k, {a: b for a, b in v.items() if a != "duration"}) for k, v in SOME_CANDIDATES]
     + [("chase_span string", dict(chase_span=["a", "b"])), ("chase_span short", dict(chase_span=[1.0])), ("chase_span 0", dict(chase_span=[0.0, 1.0])),
        ("chase_span inf", dict(chase_span=[INF, 1.0])), ("depth_min -1", dict(depth_min=-1.0)), ("min_ses NaN", dict(min_ses=NAN)),
        ("max_epochs 0", dict(max_epochs=0)), ("chase_fraction 0 and t", dict(chase_fraction=0.0, t=[[0.0]])),
        ("none", dict(period=[], T0=[], row=[], reach=[], curve=[], chase_reach=[], guard=[], chase_span=[])),
        ("reach and guard", dict(reach=[0, 1], guard=[-1, 0]))]),
    ("shape_fit_tables", _lib.shape_fit_tables, SHAPE_TABLES,
     TABLE + WINDOW + number("depth_min", -1.0, INF)
     + [("ingress string", dict(ingress=["a"])), ("ingress from 0.1", dict(ingress=[0.1, 0.5])), ("ingress to 0.4", dict(ingress=[0.0, 0.4])),
        ("units", dict(ratios=numpy.linspace(0.5, 1.0, 257), shifts=numpy.linspace(-0.1, 0.1, 128))), ("ratios and window", dict(ratios=[], window=NAN))]),
    ("shape_fit_candidates", _lib.shape_fit_candidates, dict(CANDIDATES, n_curves=2), BAD_CANDIDATES + [("heading", dict(what="x", curve=[0]))]),
    ("shape_fit_arguments", _lib.shape_fit_arguments, dict(SERIES, **CANDIDATES, **SHAPE_TABLES),
     BAD_T + BAD_Y + BAD_DY + NO_DY + SOME_CANDIDATES + ONE_ROW
     + [("t empty", dict(t=[], y=[], dy=[])), ("ratios and t", dict(ratios=[], t=[[0.0]])), ("t and period", dict(t=T[::-1], period=["a", "b"])),
        ("window 0.5", dict(window=0.5))]),
    ("transit_fit_tables", _lib.transit_fit_tables, FIT_TABLES,
     TABLE + WINDOW + number("delta", -1.0, INF)
     + [("k_rows descending", dict(k_rows=[0.1, 0.05])), ("k_rows zero", dict(k_rows=[0.0, 0.1])), ("k_rows many", dict(k_rows=numpy.linspace(0.01, 0.1, 4097))),
        ("sub unordered", dict(sub=[0.01, -0.01])), ("sub NaN", dict(sub=[NAN])), ("sub many", dict(sub=numpy.zeros(17))), ("sub empty", dict(sub=[])),
        ("profile string", dict(profile=[["a"]])), ("profile 1-D", dict(profile=[0.0, 1.0])), ("profile rows", dict(profile=PROFILE[:1])),
        ("profile M 0", dict(profile=[[0.0], [0.0]])), ("profile NaN", dict(profile=[[0.0, NAN, 1.0], [0.0, 0.6, 1.2]])),
        ("impact 1", dict(impacts=[0.0, 1.0])), ("impact negative", dict(impacts=[-0.1, 0.5])),
        ("units", dict(ratios=numpy.linspace(0.5, 1.0, 257), impacts=numpy.linspace(0.0, 0.9, 128), shifts=[-0.1, 0.0, 0.1])),
        ("k_rows and delta", dict(k_rows=[], delta=-1.0))]),
    ("transit_fit_arguments", _lib.transit_fit_arguments, dict(SERIES, **CANDIDATES, row_first=[0, 1], **FIT_TABLES),
     BAD_T[:1] + BAD_Y[1:] + BAD_DY[1:] + NO_DY + SOME_CANDIDATES[1:3] + ONE_ROW + column("row_first", [0, 2], [-1, 0])
     + [("sub NaN and t", dict(sub=[NAN], t=[[0.0]])), ("window tight", dict(window=0.7, duration=[0.01, 0.3])),
        ("duration NaN", dict(duration=[NAN, -1.0], window=0.7)),
        ("t and row_first", dict(t=T[::-1], row_first=[0, 2]))]),
    ("centroid_options", _lib.centroid_options, dict(),
     number("window", 0.5, INF) + integer("min_in", 0, 2.0, numpy.True_, "1") + integer("min_out", 0) + integer("max_epochs", 0, 65537)
     + [("window and min_in", dict(window=0.5, min_in=0))]),
    ("centroid_rows", _lib.centroid_rows, dict(cx=Y, cy=Y + 1.0, shape=(2, 4)),
     [("cx string", dict(cx=["a"])), ("cy short", dict(cy=Y[:, :3])), ("one row", dict(cx=Y[0], cy=Y[1], shape=(1, 4))),
      ("NaN", dict(cx=Y * NAN)), ("both", dict(cx=Y[:1], cy=["a"]))]),
    ("centroid_arguments", _lib.centroid_arguments, dict(t=T, y=Y, cx=Y, cy=Y + 1.0, shape=[0.0, 1.0, 0.0], **CANDIDATES),
     BAD_T + BAD_Y + SOME_CANDIDATES
     + [("one row", dict(y=Y[0], cx=Y[0], cy=Y[1], curve=[0, 0])), ("t empty", dict(t=[], y=[])), ("shape string", dict(shape=["a"])),
        ("shape 2-D", dict(shape=[[0.0, 1.0]])), ("shape one sample", dict(shape=[1.0])), ("shape NaN", dict(shape=[0.0, NAN])),
        ("cx short", dict(cx=Y[:1])), ("window 0.5 and shape", dict(window=0.5, shape=[1.0])), ("shape and t", dict(shape=[1.0], t=[[0.0]])),
        ("cx and period", dict(cx=Y[:1], period=["a", "b"]))]),
    ("folded_views_tables", _lib.folded_views_tables, dict(),
     integer("n_global", 1, 65537) + integer("n_local", 1, 65537) + number("local_durations", 0.0, INF) + number("local_width", 0.0, INF, 8.5)
     + [("n_global and local_width", dict(n_global=1, local_width=0.0))]),
    ("folded_views_arguments", _lib.folded_views_arguments, dict(t=T, y=Y, **CANDIDATES),
     BAD_T + BAD_Y + SOME_CANDIDATES
     + [("one row", dict(y=Y[0], curve=[0, 0])), ("t empty", dict(t=[], y=[])), ("secondary", dict(secondary_phase=[0.5, 0.4])),
        ("secondary string", dict(secondary_phase=["a", "b"])), ("secondary short", dict(secondary_phase=[0.5])), ("secondary scalar", dict(secondary_phase=0.5)),
        ("n_local 1 and t", dict(n_local=1, t=[[0.0]])), ("y and period", dict(y=Y * NAN, period=["a", "b"]))]),
    ("gls_axes", _lib.gls_axes, dict(t=T, frequencies=[0.1, 0.2]),
     [("t string", dict(t=["a"])), ("frequencies string", dict(frequencies=["a"])), ("t 2-D", dict(t=[T])), ("n 2", dict(t=T[:2])),
      ("n_min 1", dict(t=T[:1], n_min=1)), ("t NaN", dict(t=T * NAN)), ("t descending", dict(t=T[::-1])), ("frequencies 2-D", dict(frequencies=[[0.1]])),
      ("frequencies none", dict(frequencies=[])), ("frequency scalar", dict(frequencies=0.1)), ("frequency 0", dict(frequencies=[0.0])),
      ("frequency inf", dict(frequencies=[INF])), ("t and frequencies", dict(t=T[:2], frequencies=[]))]),
    ("gls_rows", _lib.gls_rows, SERIES,
     BAD_Y + BAD_DY + MORE_SERIES[1:] + [("y string", dict(y=["a"])), ("dy None", dict(dy=None)), ("one row", dict(y=Y[0], dy=DY[0])),
                       ("one row, dy 2-D", dict(y=Y[0], dy=DY[:1])), ("one row 2-D, dy 1-D", dict(y=Y[:1], dy=DY[0])), ("heading", dict(what="x", y=Y * NAN)), ("y NaN and dy zero", dict(y=Y * NAN, dy=DY * 0.0))]),
    ("lomb_scargle_arguments", _lib.lomb_scargle_arguments, dict(SERIES, frequencies=[0.1, 0.2]),
     [("n 2", dict(t=T[:2])), ("y NaN", dict(y=Y * NAN)), ("dy None", dict(dy=None)), ("peaks 3", dict(peaks=3)), ("peaks 0", dict(peaks=0)),
      ("peaks 33", dict(peaks=33)), ("separation 1", dict(peaks=3, separation=1.0)), ("separation unused", dict(separation=0.5)),
      ("separation string", dict(peaks=3, separation="a"))]),
    ("prewhiten_arguments", _lib.prewhiten_arguments, dict(SERIES, frequencies=[0.1, 0.2]),
     integer("n_terms", 0, 33) + integer("harmonics", 0, 9) + number("min_power", -0.1, 1.1)
     + [("n 2", dict(t=T[:2])), ("y NaN", dict(y=Y * NAN)), ("dy zero", dict(dy=DY * 0.0)), ("dy None", dict(dy=None)),
        ("y and n_terms", dict(y=Y * NAN, n_terms=0)), ("n_terms and min_power", dict(n_terms=0, min_power=2.0))]),
    ("sine_test_arguments", _lib.sine_test_arguments,
     dict(SERIES, period=[2.0, 3.0], T0=[0.5, 1.0], duration=[0.2, 0.3], curve=None, mask=1.5, harmonics=(0.5, 1.0, 2.0)),
     [("t string", dict(t=["a"])), ("t 2-D", dict(t=[T])), ("t empty", dict(t=[], y=[], dy=[])), ("t NaN", dict(t=T * NAN)), ("t descending", dict(t=T[::-1])),
      ("y NaN", dict(y=Y * NAN)), ("dy None", dict(dy=None)), ("T0 alone", dict(duration=None)), ("no T0", dict(T0=None, duration=None)),
      ("harmonics string", dict(harmonics=["a"])), ("harmonics 2-D", dict(harmonics=[[1.0]])), ("harmonics none", dict(harmonics=[])),
      ("harmonics nine", dict(harmonics=numpy.arange(1.0, 10.0))), ("harmonic 0", dict(harmonics=[0.0])), ("harmonic scalar", dict(harmonics=1.0)),
      ("period no T0 2-D", dict(period=[[2.0, 3.0]], T0=None, duration=None))]
     + number("mask", -1.0, INF) + SOME_CANDIDATES + BAD_CANDIDATES[4:7] + ONE_ROW + [("harmonics and mask", dict(harmonics=[], mask=-1.0)), ("mask and curve", dict(mask=-1.0, curve=[0]))]),
    ("peaks_arguments", _lib.peaks_arguments, dict(k=3, separation=0.02, ratios=(0.5, 2.0), min_power=None),
     [("k True", dict(k=True)), ("k 2.0", dict(k=2.0)), ("k 0", dict(k=0)), ("k 33", dict(k=33)), ("separation string", dict(separation="a")),
      ("separation None", dict(separation=None)), ("ratios string", dict(ratios=["a"])), ("separation NaN", dict(separation=NAN)),
      ("separation 1", dict(separation=1.0)), ("separation -0.1", dict(separation=-0.1)), ("ratios None", dict(ratios=None)),
      ("ratios many", dict(ratios=numpy.ones(17))), ("ratio 0", dict(ratios=[0.0])), ("ratio inf", dict(ratios=[INF])),
      ("min_power NaN", dict(min_power=NAN)), ("min_power 0.5", dict(min_power=0.5)), ("k and separation", dict(k=0, separation=1.0))]),
    ("medfilt_arguments", _lib.medfilt_arguments, dict(y=Y, kernel=3),
     [("one row", dict(y=Y[0])), ("y 3-D", dict(y=Y[None])), ("y empty", dict(y=[])), ("kernel True", dict(kernel=True)), ("kernel 3.0", dict(kernel=3.0)),
      ("kernel 0", dict(kernel=0)), ("kernel 4", dict(kernel=4)), ("kernel 5", dict(kernel=5)), ("kernel 4097", dict(y=numpy.ones(5000), kernel=4097)),
      ("y zero", dict(y=Y * 0.0)), ("y NaN", dict(y=Y * NAN)), ("kernel and y", dict(kernel=4, y=Y * 0.0))]),
    ("biweight_arguments", _lib.biweight_arguments, dict(t=T, y=Y, window_length=2.0, break_tolerance=1.5),
     BAD_T + number("window_length", 0.0, INF) + number("break_tolerance", 0.0, INF)
     + [("t empty", dict(t=[])), ("window too long", dict(t=numpy.arange(5000.0), window_length=5000.0)), ("one row", dict(y=Y[0])),
        ("y short", dict(y=Y[:, :3])), ("y 3-D", dict(y=Y[None])), ("y zero", dict(y=Y * 0.0)), ("y inf", dict(y=Y * INF)),
        ("window_length and t", dict(window_length=0.0, t=[[0.0]]))]),
    ("biweight_masked_arguments", _lib.biweight_masked_arguments,
     dict(t=T, y=Y, mask=numpy.zeros((2, 4), dtype=bool), window_length=2.0, break_tolerance=1.5),
     integer("min_points", 0, 2 ** 31)
     + [("mask uint8", dict(mask=numpy.ones((2, 4), dtype=numpy.uint8))), ("mask float", dict(mask=numpy.zeros((2, 4)))),
        ("mask 1-D of 2 rows", dict(mask=numpy.zeros(4, dtype=bool))), ("one row", dict(y=Y[0], mask=numpy.zeros(4, dtype=bool))),
        ("y zero and mask", dict(y=Y * 0.0, mask=numpy.zeros(4))), ("mask and min_points", dict(mask=numpy.zeros(4), min_points=0))]),
    ("transit_mask_arguments", _lib.transit_mask_arguments, dict(t=T, period=[2.0, 3.0], T0=[0.5, 1.0], duration=[0.2, 0.3]),
     number("factor", 0.0, INF) + [("n_curves %r" % (v,), dict(n_curves=v)) for v in (True, 2.0, -1, 1, 3)]
     + [("t string", dict(t=["a"])), ("t 2-D", dict(t=[T])), ("t empty", dict(t=[])), ("t NaN", dict(t=T * NAN)), ("t descending", dict(t=T[::-1])),
        ("T0 short", dict(T0=[0.5])), ("curve", dict(curve=[1, 1])), ("curve short", dict(curve=[1])), ("curve float", dict(curve=[0.0, 1.0])),
        ("curve past", dict(curve=[0, 2], n_curves=2)), ("curve negative", dict(curve=[-1, 0])), ("none", dict(period=[], T0=[], duration=[], curve=[])),
        ("t and factor", dict(t=T * NAN, factor=0.0))]),
    ("remove_transits_arguments", _lib.remove_transits_arguments, REMOVE,
     BAD_T + BAD_Y[:1] + column("row", [0, 2], [-1, 0], [0.0, 1.0], [0.5, 1.0], [NAN, 1.0], [3e9, 1.0], ["a", "b"])
     + [("k_rows zero", dict(k_rows=[0.0, 0.1])), ("sub NaN", dict(sub=[NAN])), ("profile NaN", dict(profile=[[0.0, NAN, 1.0], [0.0, 0.6, 1.2]])),
        ("y string", dict(y=["a"])), ("one row", dict(y=Y[0], curve=[0, 0])),
        ("t empty", dict(t=[], y=[])), ("b short", dict(b=[0.1])), ("period 2-D", dict(period=[[2.0, 3.0]])), ("three, no curve", dict({k: [1.0] * 3 for k in ("period", "T0", "amplitude", "b", "duration", "shift")}, row=[0, 0, 0])),
        ("one, no curve", dict({k: [1.0] for k in ("period", "T0", "amplitude", "b", "duration", "shift")}, row=[0])),
        ("curve", dict(curve=[1, 0])), ("curve short", dict(curve=[0])), ("curve float", dict(curve=[0.0, 1.0])), ("curve past", dict(curve=[0, 2])),
        ("none", dict({k: [] for k in ("period", "T0", "amplitude", "b", "duration", "shift", "row")})), ("sub and t", dict(sub=[NAN], t=[[0.0]])),
        ("t and row", dict(t=T[::-1], row=[0, 2]))]),
    ("sysrem_arguments", _lib.sysrem_arguments, dict(y=Y),
     [("one row", dict(y=Y[:1])), ("y 1-D", dict(y=Y[0])), ("y empty", dict(y=numpy.zeros((2, 0)))), ("dy", dict(dy=DY)), ("dy shape", dict(dy=DY[:1])),
      ("dy zero", dict(dy=DY * 0.0)), ("y zero", dict(y=Y * 0.0)), ("y NaN", dict(y=Y * NAN)), ("three rows, two components", dict(y=numpy.ones((3, 4)), n_components=2)),
      ("tol and y", dict(tol=-1.0, y=Y * 0.0))]
     + [("n_components %r" % (v,), dict(n_components=v)) for v in (True, 1.5, "1", 0, 2, numpy.int64(1))]
     + [("max_iter %r" % (v,), dict(max_iter=v)) for v in (numpy.True_, 1.5, 0, 1001)] + number("tol", -1.0, INF)),
    ("survey._candidate_rows", survey._candidate_rows, dict(what="x", t=T, flux_batch=Y, dy_batch=DY),
     SURVEY_ROWS + [("one row", dict(flux_batch=Y[0], dy_batch=DY[0])), ("one row, no dy", dict(flux_batch=Y[0], dy_batch=None)),
                    ("lists", dict(t=list(T), flux_batch=Y.tolist(), dy_batch=None)), ("flux NaN", dict(flux_batch=Y * NAN))]),
    ("survey._transit_times_options", survey._transit_times_options, dict(search=1.0, min_ses=3.0),
     number("search", 0.0, INF) + number("gap_tolerance", -1.0, INF)
     + [("transit_depth_min -1", dict(transit_depth_min=-1.0)), ("min_ses NaN", dict(min_ses=NAN)), ("max_epochs 0", dict(max_epochs=0))] + [("max_epochs 5", dict(max_epochs=5)), ("search and min_ses", dict(search=0.0, min_ses=NAN))]),
    ("survey._event_vetting_options", survey._event_vetting_options, VETTING_OPTIONS,
     number("search", 0.0) + number("chase_window", 0.0, INF) + number("guard", -1.0, INF)
     + [("gap_tolerance -1", dict(gap_tolerance=-1.0)), ("transit_depth_min -1", dict(transit_depth_min=-1.0)), ("min_ses NaN", dict(min_ses=NAN)),
        ("max_epochs 0", dict(max_epochs=0)), ("chase_fraction 0", dict(chase_fraction=0.0)), ("step_fraction 0", dict(step_fraction=0.0))]
     + [("max_epochs 5", dict(max_epochs=5)), ("guard and search", dict(guard=-1.0, search=0.0)), ("chase_min and guard", dict(chase_min=2.0, guard=-1.0))]),
    ("survey.phase_scan", _refused_only(survey.phase_scan, **NO_DEVICE), None,
     [("max_bins 15", dict(SURVEY_CANDIDATES, max_bins=15)), ("min_count 0", dict(SURVEY_CANDIDATES, min_count=0))]
     + [(k, dict(SURVEY_CANDIDATES, **v)) for k, v in SURVEY_ROWS[:3]]),
    ("survey.transit_times", _refused_only(survey.transit_times, **NO_DEVICE), None,
     [(k, dict(SURVEY_CANDIDATES, **v)) for k, v in SURVEY_ROWS[1:4] + SOME_CANDIDATES + number("search", 0.0) + integer("max_epochs", 0)
      + [("two stamps", dict(t=T[:2], flux_batch=Y[:, :2])), ("no cadence", dict(t=numpy.zeros(4))), ("duration 0", dict(duration=[0.0, 0.3])), ("duration NaN", dict(duration=[NAN, 0.3])), ("search and t", dict(search=0.0, t=T[::-1])),
         ("t and period", dict(t=T[::-1], period=["a", "b"])), ("one row", dict(flux_batch=Y[0], period=[2.0]))]]),
    ("survey.event_vetting", _refused_only(survey.event_vetting, **NO_DEVICE), None,
     [(k, dict(SURVEY_CANDIDATES, **v)) for k, v in SURVEY_ROWS[1:4] + SOME_CANDIDATES + number("search", 0.0) + number("chase_window", 0.0)
      + integer("max_epochs", 0) + [("two stamps", dict(t=T[:2], flux_batch=Y[:, :2])), ("no cadence", dict(t=numpy.zeros(4))), ("duration 0", dict(duration=[0.0, 0.3])), ("duration NaN", dict(duration=[NAN, 0.3])),
                                    ("guard and t", dict(guard=-1.0, t=T[::-1])), ("t and period", dict(t=T[::-1], period=["a", "b"])),
                                    ("one row", dict(flux_batch=Y[0], period=[2.0]))]]),
    ("survey.transit_time_rows", survey.transit_time_rows, dict(t=T, period=[2.0, NAN], duration=[0.2, 3.0]),
     [("two stamps", dict(t=T[:2])), ("t 2-D", dict(t=[T])), ("no cadence", dict(t=numpy.zeros(4))), ("duration 0", dict(duration=[0.0, 0.3])),
      ("duration inf", dict(duration=[INF, 0.3])), ("scalars", dict(period=2.0, duration=0.2)), ("none", dict(period=[], duration=[]))]),
    ("survey.event_vetting_rows", survey.event_vetting_rows, dict(t=T, period=[2.0, NAN], duration=[0.2, 3.0]),
     [("two stamps", dict(t=T[:2])), ("duration 0", dict(duration=[0.0, 0.3]))]),
    ("survey.remove_transits", _refused_only(survey.remove_transits, **NO_DEVICE), None,
     [(k, dict(dict(t=T, flux_batch=Y, planets=None, profile=(K_ROWS, PROFILE), exposure=0.02), **v)) for k, v in SURVEY_ROWS[1:4:2] + integer("n_sub", 0, 17)
      + number("exposure", -1.0, INF) + [("M 0", dict(profile=None, M=0)), ("k_rows zero", dict(profile=([0.0, 0.1], PROFILE))),
                                         ("profile no pair", dict(profile=1.0)), ("profile NaN", dict(profile=(K_ROWS, numpy.full((2, 3), NAN)))),
                                         ("planets plain", dict(planets=numpy.zeros(2))),
                                         ("three planets, two curves", dict(planets=PLANETS)), ("curve short", dict(planets=PLANETS, curve=[0, 1])), ("n_sub and flux", dict(n_sub=0, flux_batch=Y[None]))]]),
    ("survey._transit_fit_setup", survey._transit_fit_setup,
     dict(t=T, impacts=None, ratios=None, shifts=None, exposure=0.02, n_sub=2, window=1.0, min_count=3, delta=1.0, profile=(K_ROWS, PROFILE),
          template_kwargs={}),
     integer("n_sub", 0, 17) + number("exposure", -1.0, INF)
     + [("window inf", dict(window=INF)), ("min_count 0", dict(min_count=0)), ("delta -1", dict(delta=-1.0))]
     + [("exposure None", dict(exposure=None)), ("exposure 0", dict(exposure=0.0)), ("profile no pair", dict(profile=1.0)),
        ("M 0", dict(profile=None, template_kwargs=dict(M=0))), ("impacts", dict(impacts=[0.0, 1.0])), ("n_sub and window", dict(n_sub=0, window=NAN))]),
    ("survey.transit_profile", _refused_only(survey.transit_profile), None,
     [(k, v) for k, v in integer("M", 0, 4097)] + [("k_rows zero", dict(k_rows=[0.0])), ("k_rows and M", dict(k_rows=[0.0], M=0))]),
    ("survey._ratio", survey._ratio, dict(name="depth_ratio", value=2.0), number("value", 0.5, INF) + [("heading", dict(what="x", value=0.5))]),
    ("survey.event_pairs", _refused_only(survey.event_pairs), None,
     [(k, dict(dict(events=None, n_events=None), **v)) for k, v in number("depth_ratio", 0.5) + number("width_ratio", 0.5) + number("min_ses", NAN)
      + integer("max_pairs", 0) + [("events None", dict()), ("n_events 3 of 2", dict(events=EVENTS, n_events=[3])), ("width_ratio and max_pairs", dict(width_ratio=0.5, max_pairs=0))]]),
    ("survey._noise_spans", survey._noise_spans, dict(t=None, widths=[1, 3], gap_tolerance=0.5),
     number("gap_tolerance", -1.0, INF) + [("t", dict(t=T)), ("widths string", dict(widths=["a"])), ("gap_tolerance and widths", dict(gap_tolerance=-1.0, widths=["a"]))]),
    ("survey.power_batch_protected", _refused_only(survey.power_batch_protected, **NO_DEVICE), None,
     [(k, dict(dict(t=T, flux_batch=Y, detrend=None, sde_min=7.0), **v)) for k, v in number("factor", 0.0, INF) + number("sde_min", NAN)
      + [("detrend_mask", dict(detrend_mask=None)), ("median filter", dict(detrend=25)), ("factor and sde_min", dict(factor=0.0, sde_min=NAN))]]),
    ("survey.power_batch_multi", _refused_only(survey.power_batch_multi, **NO_DEVICE), None,
     [(k, dict(dict(t=T, flux_batch=Y, sde_min=7.0), **v)) for k, v in number("sde_min", NAN) + integer("n_planets", 0, 9) + number("protect_factor", 0.0, INF)
      + [("transit_fit None", dict(transit_fit=None)), ("median filter", dict(protect_factor=1.5, detrend=25)),
         ("statistics", dict(statistics=True)), ("flux 3-D", dict(flux_batch=Y[None])), ("dy shape", dict(dy_batch=DY[:1])), ("sde_min and n_planets", dict(sde_min=NAN, n_planets=0))]]),
]


def cases():
    """Every (id, function, keyword arguments) of the table, the valid call of a stage first."""
    for name, function, base, mutations in STAGES:
        if base is not None:
            yield name + ": valid", function, dict(base)
        for label, changed in mutations:
            yield "%s: %s" % (name, label), function, dict(base or {}, **changed)


def _item(v):
    if isinstance(v, numpy.ndarray):
        return "%s%s%s %r" % (v.dtype.str.lstrip("<|="), list(v.shape), "C" if v.flags.c_contiguous else "-", v.tolist())
    return "%s %r" % (type(v).__name__, v)


def describe(function, kwargs):
    """The record of one call: "Type: message" of the exception, or per returned item its key and a string of its dtype,
    shape, C-contiguity and values (of a scalar: its type and value)."""
    try:
        out = function(**kwargs)
    except Exception as e:
        return "%s: %s" % (type(e).__name__, e)
    if isinstance(out, dict):
        return {k: _item(v) for k, v in out.items()}
    return {str(i): _item(v) for i, v in enumerate(out if isinstance(out, tuple) else (out,))}


# the functions whose `raise ValueError` lines tools/record_host_refusals.py expects the table to reach
IN_SCOPE = {
    "_lib": ("phase_scan_arguments", "ephemeris_match_arguments", "noise_arguments", "_single_number", "single_widths",
             "single_options", "single_arguments", "transit_times_options", "transit_times_arguments", "event_periods_options",
             "event_periods_arguments", "event_vetting_options", "event_vetting_arguments", "shape_fit_tables",
             "shape_fit_candidates", "shape_fit_arguments", "transit_fit_tables", "transit_fit_arguments", "centroid_options",
             "centroid_rows", "centroid_arguments", "folded_views_tables", "folded_views_arguments", "gls_axes", "gls_rows",
             "lomb_scargle_arguments", "prewhiten_arguments", "sine_test_arguments", "peaks_arguments", "medfilt_kernel",
             "medfilt_arguments", "_days", "biweight_windows", "biweight_arguments", "detrend_mask_rows", "_min_points",
             "biweight_masked_arguments", "transit_mask_arguments", "remove_transits_arguments", "_sysrem_integer",
             "sysrem_arguments", "phase_scan"),
    "survey": ("_candidate_rows", "_transit_times_options", "_event_vetting_options", "phase_scan", "transit_times",
               "event_vetting", "_transit_fit_setup", "_ratio", "_noise_spans", "transit_time_rows", "event_vetting_rows",
               "transit_profile", "remove_transits", "power_batch_protected", "power_batch_multi", "event_pairs"),
}
