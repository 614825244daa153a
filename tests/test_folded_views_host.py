"""The folded views without a GPU: the statement (tests/folded_views_spec.py) equals an independent brute force (numpy.median
over a boolean mask per bin) on overlapping, disjoint and gapped tables; a constant curve, an injected box transit and
alternating depths come out as they must, and the even view is power()'s even; normalize_views on rows with empty bins at the
edges and inside, an all-empty row and a zero-minimum row; the argument checks of the Python layer, all raised before any
device work; the field lists; and the header, the binding and the version comment name tls_folded_views."""
import ctypes
import os
import re
import warnings

import numpy
import pytest

import folded_views_spec as spec
from conftest import REPO
from tls_amd import _lib, stats, survey

T = 1.0 + numpy.arange(1200) / 64.0


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


def brute(t, y, P, T0, phi_c, x_min, x_max, w, B, parity=None):
    """One view by a loop over the bins: a mask, numpy.median of what it selects."""
    median, count, any_bin = numpy.full(B, numpy.nan), numpy.zeros(B, dtype=numpy.int32), numpy.zeros(len(t), dtype=bool)
    u = (t - T0) / P - phi_c
    e = numpy.floor(u + 0.5)
    tau = (u - e) * P
    s = ((x_max - x_min) - w) / (B - 1)
    for b in range(B):
        lo = b * s + x_min
        mask = (lo <= tau) & (tau < lo + w)
        if parity is not None:
            mask &= (e % 2 == parity)
        count[b] = mask.sum()
        any_bin |= mask
        if count[b]:
            median[b] = numpy.median(y[mask])
    return median, count, int(any_bin.sum())


# ---- the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, kind", [(0.16, "w > s"), (0.5, "w == s"), (0.3, "w < s")])
@pytest.mark.parametrize("seed", [0, 1])
def test_the_statement_equals_a_brute_force(seed, width, kind):
    rng = numpy.random.RandomState(seed)
    t = numpy.delete(T, numpy.r_[300:380, 900:931])
    y = 1.0 + 1e-3 * rng.normal(size=len(t))
    y[::7] = y[3]                                                           # (equal values)
    P, T0, d, phi_s = 2.75 + 0.1 * seed, 1.4, 0.25, 0.37
    table = dict(n_global=41, n_local=201 if kind == "w > s" else 16, local_durations=4.0, local_width=width)
    record, views = spec.candidate_views(t, y, P, T0, d, phi_s, **table)
    kd, w = 4.0 * d, width * d
    s = (2 * kd - w) / (table["n_local"] - 1)
    assert {"w > s": w > s, "w == s": w == s, "w < s": w < s}[kind]
    want = dict(zip(spec.NAMES, (brute(t, y, P, T0, 0.0, -0.5 * P, 0.5 * P, P / 41, 41),
                                 brute(t, y, P, T0, 0.0, -kd, kd, w, table["n_local"]),
                                 brute(t, y, P, T0, 0.0, -kd, kd, w, table["n_local"], 0),
                                 brute(t, y, P, T0, 0.0, -kd, kd, w, table["n_local"], 1),
                                 brute(t, y, P, T0, phi_s, -kd, kd, w, table["n_local"]))))
    assert record[:2].tolist() == [0.0, 0.0]
    for i, name in enumerate(spec.NAMES):
        assert same(views[name], want[name][0]), name
        assert views[name + "_count"].dtype == numpy.int32 and (views[name + "_count"] == want[name][1]).all(), name
        assert record[2 + i] == want[name][2], name
    assert record[2] > 0.9 * len(t) and 0 < record[4] < record[3] and record[4] + record[5] == record[3]
    if kind == "w > s":
        assert views["local_count"].sum() > 3 * record[3]
    elif kind == "w == s":
        assert views["local_count"].sum() == record[3]
    else:
        assert views["local_count"].sum() == record[3] < (numpy.fabs(spec.fold(t, P, T0, 0.0)[0]) < kd).sum()


def test_medians():
    assert numpy.isnan(spec.median_of([]))
    assert spec.median_of([3.0]) == 3.0 and spec.median_of([3.0, 1.0]) == 2.0 and spec.median_of([3.0, 1.0, 9.0]) == 3.0
    assert spec.median_of([4.0, 1.0, 9.0, 2.0]) == 3.0 and spec.median_of([1e308, 1e308, 1e308]) == 1e308
    rng = numpy.random.RandomState(2)
    for c in (5, 6, 63, 64, 65):
        v = rng.normal(size=c).round(1)
        assert spec.median_of(v) == numpy.median(v)


def test_constant_curve():
    record, views = spec.candidate_views(T, numpy.ones(len(T)), 2.75, 1.4, 0.25, 0.5)
    for name in spec.NAMES:
        full = views[name + "_count"] > 0
        assert full.any() and (views[name][full] == 1.0).all() and numpy.isnan(views[name][~full]).all()
    assert (~(views["global_count"] > 0)).any()                              # (2001 bins, 1200 points)


def test_an_injected_box():
    """A box of depth 1/64 at (P, T0): the local view's centre bin is 1 - depth, the global view is 1 away from phase 0."""
    P, T0, d, depth = 2.75, 1.4 + 1 / 256.0, 0.25, 1 / 64.0
    tau = spec.fold(T, P, T0, 0.0)[0]
    y = 1.0 - depth * (numpy.fabs(tau) < 0.5 * d)
    record, views = spec.candidate_views(T, y, P, T0, d)
    assert views["local"][100] == 1.0 - depth and views["local_even"][100] == 1.0 - depth == views["local_odd"][100]
    assert (views["local"][:70] == 1.0).all() and (views["local"][131:] == 1.0).all()
    lo, hi = spec.edges(-0.5 * P, 0.5 * P, P / 2001, 2001)
    away = (hi < -0.6 * d) | (lo > 0.6 * d)
    held = views["global_count"] > 0
    near = (lo > -0.4 * d) & (hi < 0.4 * d)
    assert (away & held).sum() > 100 and (views["global"][away & held] == 1.0).all()
    assert (near & held).sum() > 5 and (views["global"][near & held] == 1.0 - depth).all()
    assert record[1] == 1.0 and numpy.isnan(views["secondary"]).all() and (views["secondary_count"] == 0).all()
    normal = spec.normalize_views(views)
    assert normal["local"].min() == -1.0 == normal["local"][100] and normal["local"][0] == 0.0
    assert normal["global"].min() == -1.0 and numpy.isnan(normal["secondary"]).all()


def test_alternating_depths_and_which_is_even():
    """Transits of depth 1/64 and 1/32 in turn, the first one -- at T0 -- the shallow one: local_even shows 1/64, local_odd
    1/32, and power()'s even transits (stats.intransit_stats: transit_depths[::2], depth_mean_even) are the same ones."""
    P, T0, d = 2.75, 1.4 + 1 / 256.0, 0.25
    tau, e = spec.fold(T, P, T0, 0.0)
    assert e.min() == 0.0                                                   # (T0 is the first transit, as power()'s is)
    y = 1.0 - numpy.where(e % 2 == 0, 1 / 64.0, 1 / 32.0) * (numpy.fabs(tau) < 0.5 * d)
    record, views = spec.candidate_views(T, y, P, T0, d)
    assert views["local_even"][100] == 1.0 - 1 / 64.0 and views["local_odd"][100] == 1.0 - 1 / 32.0
    assert views["local_even_count"][100] + views["local_odd_count"][100] == views["local_count"][100]
    times = T0 + P * numpy.arange(int(e.max()) + 1)
    mean_odd, mean_even = stats.intransit_stats(T, y, times, d)[:2]
    depths = stats.intransit_stats(T, y, times, d)[7]
    assert mean_even == 1.0 - 1 / 64.0 and mean_odd == 1.0 - 1 / 32.0
    timed = ~numpy.isnan(depths)                                            # (the last epoch lies behind the series)
    assert timed.sum() >= 6 and (depths[::2][timed[::2]] == views["local_even"][100]).all()
    assert (depths[1::2][timed[1::2]] == views["local_odd"][100]).all()
    # counted from the second transit the parities change places
    moved = spec.candidate_views(T, y, P, T0 + P, d)[1]
    assert same(moved["local_even"], views["local_odd"]) and same(moved["local_odd"], views["local_even"])


@pytest.mark.parametrize("P, T0, d", [(numpy.nan, 1.5, 0.1), (2.0, numpy.inf, 0.1), (2.0, 1.5, numpy.nan), (0.0, 1.5, 0.1),
                                      (-2.0, 1.5, 0.1), (2.0, 1.5, 0.0), (2.0, 1.5, -0.1), (numpy.inf, 1.5, 0.1), (2.0, 1.5, numpy.inf)])
def test_no_such_candidate(P, T0, d):
    record, views = spec.candidate_views(T, numpy.ones(len(T)), P, T0, d, 0.5, n_global=9, n_local=5)
    assert record.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert all(numpy.isnan(views[k]).all() and (views[k + "_count"] == 0).all() for k in spec.NAMES)


def test_the_batch_form():
    y = numpy.array([numpy.ones(len(T)), numpy.full(len(T), 2.0)])
    records, views = spec.folded_views(T, y, [2.0, numpy.nan, 3.0], [1.5, 1.5, 1.25], [0.1, 0.1, 0.2], curve=[1, 0, 0],
                                       secondary_phase=[0.5, 0.5, numpy.nan], n_global=9, n_local=5)
    assert records[:, 0].tolist() == [0.0, 1.0, 0.0] and records[:, 1].tolist() == [0.0, 1.0, 1.0]
    assert (views["global"][0] == 2.0).all() and numpy.isnan(views["global"][1]).all() and (views["global"][2] == 1.0).all()
    assert views["secondary"].shape == (3, 5) and numpy.isnan(views["secondary"][1:]).all()
    none = spec.folded_views(T, y, [2.0, 3.0], [1.5, 1.5], [0.1, 0.1], n_global=9, n_local=5)
    assert none[0][:, 1].tolist() == [1.0, 1.0] and (none[1]["global"][1] == 2.0).all()


# ---- normalize_views --------------------------------------------------------------------------------------------------------
def test_normalize_views():
    nan = numpy.nan
    rows = numpy.array([[nan, nan, 1.0, nan, nan, 0.5, 1.0, 1.0, nan],          # empty at both edges and inside
                        [nan] * 9,                                            # all empty
                        [2.0] * 9,                                            # the minimum is 0 behind the median
                        [1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]])
    views = {"local": rows, "local_count": numpy.where(numpy.isnan(rows), 0, 3).astype(numpy.int32)}
    for out in (survey.normalize_views(views), spec.normalize_views(views)):
        filled = numpy.array([1.0, 1.0, 1.0, 1.0 - 0.5 / 3, 1.0 - 1.0 / 3, 0.5, 1.0, 1.0, 1.0]) - 1.0
        assert same(out["local"][0], filled / 0.5) and out["local"][0].min() == -1.0
        assert numpy.isnan(out["local"][1]).all() and (out["local"][2] == 0.0).all()
        assert out["local"][3].tolist() == [0.0] * 4 + [-1.0] + [0.0] * 4
        assert out["local_count"].dtype == numpy.int32 and (out["local_count"] == views["local_count"]).all()
    assert numpy.isnan(rows[0, 0])                                           # (the input is not written)
    record, views = spec.candidate_views(T, 1.0 + 1e-3 * numpy.random.RandomState(3).normal(size=len(T)), 2.75, 1.4, 0.25, 0.3)
    batch = {k: numpy.array([[v, v]]) for k, v in views.items()}               # [1, 2, bins], as power_batch shapes them
    mine, theirs = survey.normalize_views(batch), spec.normalize_views(batch)
    assert set(mine) == set(theirs) == set(batch)
    for k in batch:
        assert mine[k].shape == batch[k].shape and same(mine[k], theirs[k]), k
    assert not numpy.isnan(mine["global"]).any() and (mine["global"].min(axis=-1) == -1.0).all()


# ---- the layers -------------------------------------------------------------------------------------------------------------
def test_field_lists_and_constants():
    assert survey.folded_view_fields() == _lib.VIEWS_FIELDS == spec.FIELDS
    assert _lib.VIEWS_LOCAL == spec.LOCAL and _lib.VIEWS_DTYPE.names == spec.FIELDS
    assert ctypes.sizeof(_lib.ViewsRecord) == 56 == _lib.VIEWS_DTYPE.itemsize
    assert [n for n, _ in _lib.ViewsRecord._fields_] == list(spec.FIELDS)
    assert spec.DEFAULTS == dict(n_global=2001, n_local=201, local_durations=4.0, local_width=0.16)
    assert _lib.folded_views_tables() == (2001, 201, 4.0, 0.16)


def test_the_record_of_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct tls_views_record \{(.*?)\} tls_views_record;", code, flags=re.S).group(1)
    declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
    assert tuple(declared) == _lib.VIEWS_FIELDS
    assert "#define TLS_VIEWS_MAX_BINS %d" % _lib.VIEWS_MAX_BINS in text
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_views.hip.h")).read()
    for name, value in (("kViewsWords", 7), ("kViewsLdsPoints", _lib.VIEWS_LDS_POINTS), ("kViewsLaneMembers", _lib.VIEWS_LANE_MEMBERS),
                        ("kViewsSlab", _lib.VIEWS_SLAB), ("kViewsMaxBins", "1 << 16"), ("kViewsMaxPoints", "1 << 20")):
        assert "constexpr int %s = %s;" % (name, value) in kernel, name
    assert _lib.VIEWS_MAX_BINS == 1 << 16 and _lib.VIEWS_MAX_POINTS == 1 << 20
    assert "__syncthreads" not in re.sub(r"//[^\n]*", "", kernel) and "wg_sync();" in kernel
    assert "#pragma clang fp contract(off)" in kernel and "kChkViews" in kernel
    assert "atomicAdd(members, held)" in kernel and "double* members" not in kernel      # (the only atomics are on LDS ints)


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_folded_views"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "(8: %s)" % name in text.split("#define TLS_AMD_ABI_VERSION")[0]     # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_folded_views.argtypes) == declared.count(",") + 1 == 20
    assert declared.endswith("double *global_median, int32_t *global_count, double *local_median, int32_t *local_count")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_views.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    assert hasattr(_lib.Context, "folded_views") and callable(_lib.folded_views_arguments)
    assert '#include "tls_views.hip.h"' in open(os.path.join(REPO, "tls_amd", "csrc", "tls_kernels.hip.h")).read()


BAD = [
    (dict(n_global=1), "n_global"), (dict(n_global=0), "n_global"), (dict(n_global=2.5), "n_global"), (dict(n_global=True), "n_global"),
    (dict(n_global=_lib.VIEWS_MAX_BINS + 1), "n_global"), (dict(n_local=1), "n_local"), (dict(n_local=-4), "n_local"),
    (dict(n_local="201"), "n_local"), (dict(local_durations=0.0), "local_durations"), (dict(local_durations=-1.0), "local_durations"),
    (dict(local_durations=numpy.nan), "local_durations"), (dict(local_durations=numpy.inf), "local_durations"),
    (dict(local_width=0.0), "local_width"), (dict(local_width=-0.16), "local_width"), (dict(local_width=numpy.nan), "local_width"),
    (dict(local_width=8.5), "wider than the view"), (dict(local_durations=0.05), "wider than the view"),
    (dict(period=[1.0]), "n_fits"), (dict(period=[[1.0, 1.5]]), "n_fits"), (dict(T0=["a", "b"]), "numbers"),
    (dict(curve=[0, 2]), "curve"), (dict(curve=[-1, 0]), "curve"), (dict(curve=[0.0, 1.0]), "curve"), (dict(curve=[0]), "curve"),
    (dict(secondary_phase=[0.5]), "secondary_phase"), (dict(secondary_phase="x"), "secondary_phase")]


@pytest.mark.parametrize("kw, match", BAD)
def test_survey_call_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    args = dict(dict(period=[1.0, 1.5], T0=[1.2, 1.3], duration=[0.1, 0.1]), **kw)
    with pytest.raises(ValueError, match=match):
        survey.folded_views(T, flux, **args)


def test_survey_call_checks_the_rows_and_reaches_the_device(no_device):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    good = ([1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
    with pytest.raises(ValueError, match="over the time stamps"):
        survey.folded_views(T, flux[:, :-1], *good)
    with pytest.raises(ValueError, match="one candidate a light curve"):
        survey.folded_views(T, flux, [1.0], [1.2], [0.1])
    with pytest.raises(ValueError, match="non-decreasing"):
        survey.folded_views(T[::-1], flux, *good)
    with pytest.raises(ValueError, match="non-decreasing"):
        survey.folded_views(numpy.where(numpy.arange(len(T)) == 7, numpy.nan, T), flux, *good)
    with pytest.raises(ValueError, match="NaN or an infinite"):
        survey.folded_views(T, numpy.where(flux > 1.003, numpy.inf, flux), *good)
    with pytest.raises(AssertionError, match="a context was created"):     # (a good call reaches the device)
        survey.folded_views(T, flux, [1.0, numpy.nan], [1.2, 1.3], [0.1, -1.0], secondary_phase=[numpy.nan, 0.5])
    with pytest.raises(AssertionError, match="a context was created"):     # (a bin as wide as the view)
        survey.folded_views(T, flux[0], [1.0], [1.2], [0.1], n_global=2, n_local=2, local_width=8.0)


@pytest.mark.parametrize("kw, match", [
    (dict(views=True), "needs peak_fits"), (dict(views=True, peaks=3), "needs peak_fits"),
    (dict(views=True, peaks=3, peak_fits=True, views_global_bins=1), "n_global"),
    (dict(views=True, peaks=3, peak_fits=True, views_local_bins=1), "n_local"),
    (dict(views=True, peaks=3, peak_fits=True, views_local_durations=0.0), "local_durations"),
    (dict(views=True, peaks=3, peak_fits=True, views_local_width=-1.0), "local_width"),
    (dict(views=True, peaks=3, peak_fits=True, views_local_width=9.0), "wider than the view")])
def test_power_batch_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, **kw)
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, detrend=25, **kw)


def test_folded_views_arguments_packs():
    a = _lib.folded_views_arguments(T, numpy.ones(len(T)), [numpy.nan, -2.0], [1.1, 1.2], [0.1, 0.2], curve=[0, 0],
                                    secondary_phase=[0.5, numpy.nan], n_global=numpy.int64(9))
    assert a["y"].shape == (1, len(T)) and a["curve"].dtype == numpy.int64 and a["curve"].tolist() == [0, 0]
    assert (a["n_global"], a["n_local"], a["local_durations"], a["local_width"]) == (9, 201, 4.0, 0.16)
    assert all(a[k].flags.c_contiguous and a[k].dtype == numpy.float64 for k in ("t", "y", "period", "T0", "duration", "secondary_phase"))
    one = _lib.folded_views_arguments(T, numpy.ones((2, len(T))), [1.0, 2.0], [1.1, 1.2], [0.1, 0.2])
    assert one["curve"].tolist() == [0, 1] and one["secondary_phase"] is None


def test_the_host_formed_fields():
    base = numpy.zeros((2, 2), dtype=[("period", "f8"), ("status", "f8")])
    raw = numpy.zeros((2, 2), dtype=_lib.VIEWS_DTYPE)
    raw["status"], raw["n_local_odd"], raw["secondary_status"] = [[0, 1], [0, 0]], 7.0, 1.0
    out = survey._with_views(base, raw)
    assert out.dtype.names == ("period", "status", "views_status", "views_n_global", "views_n_local", "views_n_local_even",
                               "views_n_local_odd", "views_n_secondary")
    assert out["views_status"].tolist() == [[0, 1], [0, 0]] and (out["views_n_local_odd"] == 7.0).all()
    g, gc = numpy.arange(12.0).reshape(4, 3), numpy.arange(12, dtype=numpy.int32).reshape(4, 3)
    l, lc = numpy.arange(32.0).reshape(4, 4, 2), numpy.arange(32, dtype=numpy.int32).reshape(4, 4, 2)
    views = survey._views_dict(g, gc, l, lc, lead=(2, 2))
    assert set(views) == set(spec.NAMES) | {k + "_count" for k in spec.NAMES}
    assert views["global"].shape == (2, 2, 3) and views["local_odd"].shape == (2, 2, 2) and views["secondary_count"].dtype == numpy.int32
    assert views["local_odd"][1, 0].tolist() == l[2, 2].tolist() and views["secondary"][0, 1].tolist() == l[1, 3].tolist()
