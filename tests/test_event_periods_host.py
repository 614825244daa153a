"""Event periods without a GPU: the statement (tests/event_periods_spec.py) equals its own loops bit for bit; it keeps the true
period of two sectors a year apart and of three transits in a window with a gap, and vetoes what the data rule out; event_pairs;
the argument checks of the Python layer, all raised before any device work; and the header, the binding and the version comment
name tls_event_periods."""
import ctypes
import os
import re

import numpy
import pytest

import event_periods_spec as spec
from conftest import REPO
from tls_amd import _lib, survey

SHAPE = spec.DEFAULT_SHAPE


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


def _same(fast, slow):
    return fast[0].tobytes() == slow[0].tobytes() and fast[1].tobytes() == slow[1].tobytes()


@pytest.mark.parametrize("L", [3, 4, 9, 16])
def test_the_loops_equal_the_vectorised_form(L):
    """Random small cases: a gap, equal time stamps, per-point dy, odd and even widths, events at the ends, every status."""
    rng = numpy.random.default_rng(L)
    t = numpy.delete(1.0 + numpy.arange(260) / 64.0, numpy.arange(120, 170))
    t[40] = t[39]                                                     # (two samples share a time stamp)
    y = 1 + rng.normal(0, 1e-3, len(t))
    dips = (20, 70, 95, 150, 190)
    for at in dips:
        y[at - (L - 1) // 2: at - (L - 1) // 2 + L] -= 5e-3
    for at in (110, 180):                                             # (two bumps: a pair without a dip)
        y[at - (L - 1) // 2: at - (L - 1) // 2 + L] += 8e-3
    dy = rng.uniform(5e-4, 2e-3, len(t))
    b = spec.shapes_of([L], **SHAPE)[0]
    span = (L - 1) / 64.0 * 1.5
    statuses = set()
    for ca, cb, S, offset, pmin, amax, min_ses, veto in (
            (20, 70, 2, 2.5 / 64, 0.1, 16, 3.0, 3.0), (20, 190, 1, 1.5 / 64, 0.05, 64, 3.0, 3.0), (70, 95, 3, 3.5 / 64, 0.02, 8, 0.0, numpy.inf),
            (95, 150, 2, 2.5 / 64, 0.3, 16, 3.0, -1.0), (39, 40, 2, 2.5 / 64, 0.1, 16, 3.0, 3.0), (0, 209, 2, 2.5 / 64, 0.1, 16, 3.0, 3.0),
            (110, 180, 1, 0.0, 0.1, 16, 3.0, 3.0), (20, 70, 2, 2.5 / 64, 5.0, 16, 3.0, 3.0), (20, 70, 2, 0.0, 0.1, 16, 3.0, 3.0)):
        fast = spec.event_periods(t, y, dy, ca, cb, b, span, S, offset, pmin, amax, min_ses, veto)
        slow = spec.event_periods_loops(t, y, dy, ca, cb, b, span, S, offset, pmin, amax, min_ses, veto)
        assert _same(fast, slow), (L, ca, cb)
        assert fast[0].shape == (16,) and fast[1].shape == (amax, 8)
        statuses.add(int(fast[0][0]))
    assert statuses == {0, 1, 2, 3}
    # constant flux, NaN-free: every q is 0, the first shift and the smallest k win the ties
    flat = numpy.ones(len(t))
    fast = spec.event_periods(t, flat, dy, 20, 70, b, span, 2, 2.5 / 64, 0.1, 16)
    slow = spec.event_periods_loops(t, flat, dy, 20, 70, b, span, 2, 2.5 / 64, 0.1, 16)
    assert _same(fast, slow) and fast[0][0] == 2                      # (pN == 0 is no dip)


def _pair(record):
    return dict(zip(spec.PAIR_FIELDS, record))


def _table(table, n):
    return {f: table[:n, i] for i, f in enumerate(spec.ALIAS_FIELDS)}


@pytest.mark.parametrize("seed", range(5))
def test_two_sectors_a_year_apart(seed, capsys):
    """Scenario A of DESIGN.md "Event periods": the true alias k = 10 is allowed, an allowed alias has no covered epoch but the
    pair's own two unless another one shows a dip, and a vetoed alias exceeds veto_sigma by definition -- the smallest
    worst_sigma among them is printed, not asserted."""
    s = spec.scenario_two_sectors(seed)
    pair, table = spec.event_periods(s["t"], s["flux"], s["dy"], s["ca"], s["cb"], s["b"], s["span_max"], s["S"], s["offset"],
                                     2.0, 256, 3.0, 3.0)
    pair = _pair(pair)
    assert pair["status"] == 0 and pair["n_aliases"] == 178 and pair["n_evaluated"] == 178
    a = _table(table, 178)
    with numpy.errstate(invalid="ignore"):
        vetoed = a["worst_sigma"] > 3.0
    allowed = ~vetoed
    assert allowed[s["true_k"] - 1] and abs(a["period"][s["true_k"] - 1] - s["period"]) <= s["cadence"]
    assert pair["n_allowed"] == allowed.sum() and pair["longest_k"] == numpy.flatnonzero(allowed)[0] + 1
    no_other_dip = allowed & ~(a["n_seen"] > 2)
    assert numpy.all(a["n_covered"][no_other_dip] == 2), a["n_covered"][no_other_dip]
    assert numpy.all(a["worst_sigma"][vetoed] > 3.0) and vetoed.any()
    with capsys.disabled():
        print("\nscenario A seed %d: %d of 178 aliases allowed, smallest vetoed worst_sigma %.1f, pair_mes %.1f"
              % (seed, allowed.sum(), a["worst_sigma"][vetoed].min(), pair["pair_mes"]))


@pytest.mark.parametrize("seed", range(5))
def test_three_transits_in_a_window_with_a_gap(seed, capsys):
    """Scenario B: over the three pairs the allowed alias of the largest mes is the true period with three covered epochs, and
    half the period is vetoed."""
    s = spec.scenario_three_transits(seed)
    c = s["centres"]
    best = None
    for ca, cb in ((c[0], c[1]), (c[1], c[2]), (c[0], c[2])):
        pair, table = spec.event_periods(s["t"], s["flux"], s["dy"], ca, cb, s["b"], s["span_max"], s["S"], s["offset"], 2.0,
                                         64, 3.0, 3.0)
        pair = _pair(pair)
        assert pair["status"] == 0
        a = _table(table, int(pair["n_evaluated"]))
        with numpy.errstate(invalid="ignore"):
            allowed = ~(a["worst_sigma"] > 3.0)
        half = numpy.flatnonzero(numpy.abs(a["period"] - s["period"] / 2) <= s["cadence"])
        assert len(half) == 1 and not allowed[half[0]]
        if best is None or pair["best_mes"] > best["best_mes"]:
            best = pair
        if (ca, cb) == (c[0], c[2]):
            longest = pair, a, allowed
    assert abs(best["best_period"] - s["period"]) <= s["cadence"] and best["best_n_covered"] == 3
    pair, a, allowed = longest
    assert allowed[0] and a["n_covered"][0] == 2 and a["mes"][0] < best["best_mes"]          # 22 d: allowed, and behind 11 d
    with capsys.disabled():
        print("\nscenario B seed %d: best %.3f d, mes %.1f, %d covered; 22 d mes %.1f"
              % (seed, best["best_period"], best["best_mes"], best["best_n_covered"], a["mes"][0]))


def _events(rows, k=6):
    """Records of single_transits for one curve from (index, ses, depth, width, row) tuples."""
    ev = numpy.zeros(k, dtype=[(f, "f8") for f in survey.single_event_fields()])
    ev["index"] = -1
    for i, (index, ses, depth, width, row) in enumerate(rows):
        ev[i] = (index, 0.0, ses, depth, row, width, 0.0, 0.0, 0.0)
    return ev, len(rows)


def test_event_pairs():
    one, n_one = _events([(500, 12.0, 2e-3, 9, 2), (100, 10.0, 2.5e-3, 9, 2), (900, 8.0, 1.9e-3, 12, 3), (300, 9.0, 6e-3, 9, 2),
                          (700, 5.0, 2e-3, 9, 2), (800, 11.0, 2e-3, 30, 5)])
    none, n_none = _events([])
    lone, n_lone = _events([(10, 20.0, 1e-3, 5, 0)])
    events, n_events = numpy.stack([none, one, lone]), numpy.array([n_none, n_one, n_lone])
    curve, ia, ib, row = survey.event_pairs(events, n_events)
    # 300 is three times as deep, 700 too weak, 800 more than twice as wide: the pairs among 100, 500, 900 by strength
    assert curve.tolist() == [1, 1, 1] and list(zip(ia.tolist(), ib.tolist())) == [(100, 500), (500, 900), (100, 900)]
    assert row.tolist() == [2, 2, 2] and all(v.dtype == numpy.int64 for v in (curve, ia, ib, row))
    assert survey.event_pairs(events, n_events, max_pairs=1)[1].tolist() == [100]
    assert len(survey.event_pairs(events, n_events, depth_ratio=1.0)[0]) == 0
    wide = survey.event_pairs(events, n_events, min_ses=5.0, depth_ratio=4.0, width_ratio=4.0, max_pairs=100)
    assert len(wide[0]) == 15 and numpy.all(wide[1] < wide[2])
    stronger = survey.event_pairs(events, n_events, min_ses=8.0, width_ratio=4.0)
    assert (800, 900, 5) in zip(stronger[1].tolist(), stronger[2].tolist(), stronger[3].tolist())
    assert len(survey.event_pairs(events[:1], n_events[:1])[0]) == 0
    for bad in (dict(depth_ratio=0.5), dict(width_ratio=numpy.nan), dict(min_ses=numpy.nan), dict(max_pairs=0), dict(max_pairs=2.0)):
        with pytest.raises(ValueError, match="event pairs"):
            survey.event_pairs(events, n_events, **bad)
    with pytest.raises(ValueError, match="event pairs"):
        survey.event_pairs(numpy.zeros((3, 6)), n_events)


def test_event_period_reach():
    reach, offset = survey.event_period_reach([3, 9, 48, 4096], [0, 1, 2, 3, 1], 0.5)
    assert reach.tolist() == [1, 2, 12, 1024, 2] and offset.tolist() == [0.75, 1.25, 6.25, 512.25, 1.25]


T = 1.0 + numpy.arange(300) / 64.0
ROWS = dict(widths=[3, 5], shapes=spec.shapes_of([3, 5], **SHAPE), span_max=[0.05, 0.1])


def _arguments(**over):
    a = dict(t=T, y=numpy.ones((2, 300)), dy=numpy.full((2, 300), 1e-3), curve=[0, 1], index_a=[10, 20], index_b=[100, 200],
             row=[0, 1], reach=[1, 2], offset=[0.03, 0.04], period_min=0.5)
    a.update(ROWS)
    a.update(over)
    return a


@pytest.mark.parametrize("bad", [
    dict(period_min=0.0), dict(period_min=numpy.inf), dict(period_min=numpy.nan), dict(period_min=True), dict(period_min=1e-6),
    dict(max_aliases=0), dict(max_aliases=4097), dict(max_aliases=2.0), dict(min_ses=numpy.nan), dict(veto_sigma=numpy.nan),
    dict(veto_sigma=None), dict(curve=[0, 2]), dict(curve=[0.0, 1.0]), dict(index_a=[-1, 20]), dict(index_b=[100, 300]),
    dict(index_a=[100, 20], index_b=[100, 200]), dict(index_a=[10]), dict(row=[0, 2]), dict(reach=[0, 2]), dict(reach=[1, 4097]),
    dict(offset=[0.03, -1e-9]), dict(offset=[0.03, numpy.inf]), dict(offset=[0.03]), dict(offset=["a", "b"]),
    dict(t=T[::-1]), dict(t=numpy.zeros((1 << 20) + 1)), dict(widths=[5, 3]), dict(span_max=[0.05, -1.0]),
    dict(dy=numpy.zeros((2, 300))), dict(y=numpy.full((2, 300), numpy.nan)),
])
def test_argument_errors_raise_before_any_device_work(bad, no_device):
    with pytest.raises(ValueError, match="event periods"):
        _lib.event_periods_arguments(**_arguments(**bad))


def test_the_arguments_are_packed(no_device):
    a = _lib.event_periods_arguments(**_arguments(veto_sigma=numpy.inf))
    assert a["veto_sigma"] == numpy.inf and a["max_aliases"] == 256 and a["min_ses"] == 3.0
    assert all(a[k].dtype == numpy.int64 for k in ("curve", "index_a", "index_b", "row", "reach", "width", "shape_offset"))
    assert a["offset"].dtype == numpy.float64 and a["shape_offset"].tolist() == [0, 3]
    assert "depth_min" not in a and "k" not in a
    # the epoch bound: (t[n-1] - t[0]) / period_min + 2 <= TIMES_MAX_EPOCHS
    span = T[-1] - T[0]
    _lib.event_periods_arguments(**_arguments(period_min=span / (_lib.TIMES_MAX_EPOCHS - 2)))
    with pytest.raises(ValueError, match="epochs"):
        _lib.event_periods_arguments(**_arguments(period_min=span / (_lib.TIMES_MAX_EPOCHS - 1.9)))


@pytest.mark.parametrize("bad", [
    dict(period_min=-1.0), dict(max_aliases=0), dict(min_ses=numpy.nan), dict(veto_sigma=numpy.nan), dict(gap_tolerance=-0.1),
    dict(widths=[5, 3]), dict(reach=0), dict(reach=1.5), dict(reach=[1, 2, 3]), dict(pairs=([0], [5], [2], [0])),
    dict(pairs=([1], [5], [20], [0])), dict(pairs=([0], [5], [20], [7])), dict(pairs=([0], [5], [20])),
    dict(pairs=([0], [5], [20], [0]), events=numpy.zeros(1), n_events=[0]), dict(events=numpy.zeros(1)),
])
def test_the_survey_call_checks_before_any_device_work(bad, no_device):
    kw = dict(pairs=([0], [5], [20], [0]), widths=[3, 5])
    kw.update(bad)
    with pytest.raises(ValueError):
        survey.event_periods(T, numpy.ones((1, 300)), detrend=25, **kw)


def test_the_header_the_binding_and_the_records_agree():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    assert "(8: tls_event_periods)" in text and "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8
    assert "tls_event_periods" in _lib.SYMBOLS
    assert int(re.search(r"#define TLS_ALIAS_MAX (\d+)", text).group(1)) == _lib.ALIAS_MAX == spec.ALIAS_MAX == 4096
    for name, fields, struct, dtype, size in (("tls_event_pair", _lib.EVENT_PAIR_FIELDS, _lib.EventPair, _lib.EVENT_PAIR_DTYPE, 128),
                                              ("tls_event_alias", _lib.EVENT_ALIAS_FIELDS, _lib.EventAlias, _lib.EVENT_ALIAS_DTYPE, 64)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [w.strip() for part in re.findall(r"double ([^;]+);", body) for w in part.split(",")]
        assert tuple(declared) == tuple(fields), name
        assert ctypes.sizeof(struct) == dtype.itemsize == size == 8 * len(fields)
    assert tuple(_lib.EVENT_PAIR_FIELDS) == spec.PAIR_FIELDS == survey.event_pair_fields()
    assert tuple(_lib.EVENT_ALIAS_FIELDS) == spec.ALIAS_FIELDS == survey.event_alias_fields()
    kernels = open(os.path.join(REPO, "tls_amd", "csrc", "tls_aliases.hip.h")).read()
    assert int(re.search(r"kAliasLdsPoints = (\d+)", kernels).group(1)) == _lib.ALIAS_LDS_POINTS
    assert int(re.search(r"kAliasTile = (\d+)", kernels).group(1)) == _lib.ALIAS_TILE
    assert 24 * _lib.ALIAS_LDS_POINTS + 8192 <= 160 * 1024
    names = [n for n in dir(_lib.Context) if not n.startswith("_")]
    assert "event_periods" in names
