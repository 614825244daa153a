"""Biweight detrending without a GPU: the tls_biweight_detrend declaration and constants against the binding, hand-worked
cases of the restatement (biweight_spec), the binding's windows against the restatement's, a numpy restatement of the kernel's
per-lane walk (sorted span, median scan, MAD walk, ordered sums) and of its tile plan and LDS, the argument errors (raised
before any device work), and the order of calls behind detrend=Biweight(...) in the survey functions, with stand-in contexts
that record what they are asked to do."""
import ctypes
import os
import re
import warnings

import numpy
import pytest

from tls_amd import _lib, survey
from conftest import REPO
import biweight_spec as spec


def _header():
    return open(os.path.join(REPO, "include", "tls_amd.h")).read()


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


# ---- header and binding

def test_declaration_matches_argtypes():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"int\s+tls_biweight_detrend\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "tls_biweight_detrend is not declared"
    c_types = {"tls_ctx *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "const double *": _lib._c_double_p,
               "double *": _lib._c_double_p, "double": ctypes.c_double}
    want = []
    for p in m.group(1).split(","):
        words = p.replace("*", " * ").split()[:-1]   # (the type without the parameter's name)
        want.append(c_types[" ".join(words).replace(" *", " *")])
    got = _lib.load().tls_biweight_detrend.argtypes
    assert len(got) == len(want) == 9
    assert list(got) == want
    assert _lib.load().tls_biweight_detrend.restype == ctypes.c_int
    assert "tls_biweight_detrend" in _lib.SYMBOLS
    assert re.search(r"Entries added without changing a layout.*tls_biweight_detrend\)", _header(), flags=re.S)


def test_constants_mirrored_and_abi_8():
    h = _header()
    m = re.search(r"#define TLS_BIWEIGHT_MAX_WINDOW (\d+)\b", h)
    assert m and int(m.group(1)) == _lib.BIWEIGHT_MAX_WINDOW == spec.MAX_WINDOW >= 4095
    assert float(re.search(r"#define TLS_BIWEIGHT_C (\S+)", h).group(1)) == _lib.BIWEIGHT_C == spec.C == 5.0
    assert float(re.search(r"#define TLS_BIWEIGHT_FTOL (\S+)", h).group(1)) == _lib.BIWEIGHT_FTOL == spec.FTOL == 1e-6
    assert int(re.search(r"#define TLS_BIWEIGHT_MAX_ITER (\d+)", h).group(1)) == _lib.BIWEIGHT_MAX_ITER == spec.MAX_ITER == 50
    assert _lib.ABI_VERSION == 8
    assert _lib.load().tls_abi_version() == 8
    assert re.search(r"#define TLS_AMD_ABI_VERSION 8\b", h)


# ---- hand-worked cases of the restatement

def test_one_point_window_is_the_identity():
    t = numpy.arange(6.0)
    y = numpy.array([1.0, 3.0, 0.5, 7.0, 1e-300, 1e300])
    flat, trend = spec.detrend(t, y, 0.5, 0.5)
    assert numpy.array_equal(_bits(trend), _bits(y)) and numpy.all(flat == 1.0)


def test_mad_zero_keeps_the_median():
    assert spec.location([1.0, 1.0, 1.0, 1.0, 10.0]) == 1.0
    assert spec.location([2.0, 2.0, 2.0, 5.0, 9.0]) == 2.0


def test_single_outlier_gets_weight_zero():
    v = numpy.array([1.0, 1.01, 0.99, 1.02, 0.98, 50.0])
    loc = spec.location(v)
    loc0 = spec.median(v)
    mad = spec.median(numpy.abs(v - loc0))
    assert abs((50.0 - loc0) / (spec.C * mad)) >= 1.0
    # its weight is 0 in every step, and it stays the largest value: any larger outlier gives the same bits
    w = numpy.array(v)
    w[-1] = 5e10
    assert spec.location(w) == loc and 0.98 < loc < 1.02


def test_split_at_break_tolerance_is_strict():
    t = numpy.array([0.0, 0.25, 0.75, 1.0])       # a step of exactly 0.5 in the middle
    lo, hi = spec.windows(t, 10.0, 0.5)
    assert lo.tolist() == [0] * 4 and hi.tolist() == [4] * 4
    lo, hi = spec.windows(t, 10.0, 0.4999)
    assert lo.tolist() == [0, 0, 2, 2] and hi.tolist() == [2, 2, 4, 4]
    for args in ((10.0, 0.5), (10.0, 0.4999), (0.6, numpy.inf)):
        assert [a.tolist() for a in _lib.biweight_windows(t, *args)[3:]] == [a.tolist() for a in spec.windows(t, *args)]


def test_even_window_takes_the_mean_of_the_middle_two():
    assert spec.median(numpy.array([4.0, 1.0, 3.0, 2.0])) == 2.5
    assert spec.median(numpy.array([1.0, 1.0 + 2 ** -52])) == (1.0 + (1.0 + 2 ** -52)) / 2.0
    v = numpy.array([1.0, 2.0])
    # loc = 1.5, |d| = 0.5, 0.5 -> mad = 0.5, u = +-0.2: equal weights w, new = fl(w + 2 w) / fl(2 w), 1.5 up to rounding
    w = (1.0 - 0.2 * 0.2) * (1.0 - 0.2 * 0.2)
    assert spec.location(v) == (w * 1.0 + w * 2.0) / (w + w) and abs(spec.location(v) - 1.5) <= 2.3e-16
    rng = numpy.random.default_rng(3)
    for m in (2, 4, 10, 64):
        v = 1.0 + 1e-3 * rng.standard_normal(m)
        assert spec.median(v) == numpy.median(v)


def test_windows_equal_the_binding():
    rng = numpy.random.default_rng(11)
    for n in (1, 2, 5, 300):
        for t in (numpy.cumsum(rng.uniform(0.0, 0.05, n)), numpy.round(numpy.cumsum(rng.uniform(0.0, 0.3, n)), 1),
                  numpy.sort(rng.choice([0.0, 0.5, 1.0, 1.5, 3.0], n))):
            for wl, bt in ((0.01, 0.5), (0.5, 0.5), (1.0, 0.25), (2.0, numpy.inf), (100.0, 0.5)):
                got = _lib.biweight_windows(t, wl, bt)[3:]
                want = spec.windows(t, wl, bt)
                assert numpy.array_equal(got[0], want[0]) and numpy.array_equal(got[1], want[1]), (n, wl, bt)


# ---- a numpy restatement of the kernel (tls_biweight.hip.h) and of its tile plan (tls_amd.hip biweight_plan)

def kernel_location(keys, slots, vals, S, wa, wb):
    """One output lane: the sorted span (keys ascending, slot numbers), the index-ordered copy vals, the window [wa, wb)."""
    m = wb - wa
    need1, need2 = (m + 1) // 2, m // 2 + 1
    inwin = (slots[:S] >= wa) & (slots[:S] < wb)
    order = numpy.flatnonzero(inwin)                      # the scan: the window's sorted slots in order
    f1, f2 = order[need1 - 1], order[need2 - 1]
    kv = keys.view(numpy.float64)
    loc = kv[f2] if m % 2 else (kv[f1] + kv[f2]) / 2.0
    for _ in range(spec.MAX_ITER):
        p = int(numpy.searchsorted(keys[:S], numpy.float64(loc).view(numpy.uint64), side="right"))
        l, r, c = p - 1, p, 0
        d1 = d2 = 0.0
        while True:
            while l >= 0 and not inwin[l]:
                l -= 1
            while r < S and not inwin[r]:
                r += 1
            assert l >= 0 or r < S
            if r >= S or (l >= 0 and loc - kv[l] <= kv[r] - loc):
                d = loc - kv[l]
                l -= 1
            else:
                d = kv[r] - loc
                r += 1
            c += 1
            if c == need1:
                d1 = d
            if c == need2:
                d2 = d
                break
        mad = d2 if m % 2 else (d1 + d2) / 2.0
        if mad == 0.0:
            break
        s = spec.C * mad
        sw = swv = 0.0
        for v in vals[wa:wb]:
            u = (v - loc) / s
            q = 1.0 - u * u
            w = q * q if abs(u) < 1.0 else 0.0
            sw = sw + w
            swv = swv + w * v
        new = swv / sw
        done = abs(new - loc) <= spec.FTOL * abs(new)
        loc = new
        if done:
            break
    return loc


def plan_of(lo, hi):
    """biweight_plan: (T, P, smax) -- P0 = pow2(max(4 (wmax - 1), 256)) capped at 8192, one tile for n <= P0, otherwise
    T = P0 - 2 (wmax - 1); smax the largest span [lo_first, hi_last) of the tiles, P the power of two (>= 64) above it."""
    def pow2(v):
        p = 64
        while p < v:
            p <<= 1
        return p
    n, wmax = len(lo), int((hi - lo).max())
    P0 = min(pow2(max(4 * (wmax - 1), 256)), 8192)
    T = n if n <= P0 else P0 - 2 * (wmax - 1)
    smax = max(int(hi[min(f + T, n) - 1] - lo[f]) for f in range(0, n, T))
    return T, pow2(smax), smax


def mirror_detrend(t, y, wl, bt):
    """(flat, trend) of one row as the kernel forms it, tile by tile (the bitonic network is a sort: numpy's stable one)."""
    lo, hi = spec.windows(t, wl, bt)
    T, P, smax = plan_of(lo, hi)
    n = len(y)
    trend = numpy.empty(n)
    for first in range(0, n, T):
        last = min(first + T, n) - 1
        base, S = lo[first], hi[last] - lo[first]
        assert 1 <= S <= smax <= P
        vals = y[base: base + S]
        keys = numpy.full(P, 2 ** 64 - 1, dtype=numpy.uint64)
        keys[:S] = vals.view(numpy.uint64)
        slots = numpy.full(P, 2 ** 32 - 1, dtype=numpy.int64)
        slots[:S] = numpy.arange(S)
        o = numpy.argsort(keys, kind="stable")
        keys, slots = keys[o], slots[o]
        for g in range(first, last + 1):
            trend[g] = kernel_location(keys, slots, vals, S, lo[g] - base, hi[g] - base)
    return y / trend, trend


def _times(n, rng):
    t = 10.0 + numpy.cumsum(rng.uniform(0.0, 0.04, n))
    t[n // 2:] += 0.6
    return t


@pytest.mark.parametrize("n", [1, 2, 7, 90, 400])
def test_kernel_mirror_equals_the_restatement(n):
    rng = numpy.random.default_rng(n)
    t = _times(n, rng)
    rows = [1.0 + 1e-3 * rng.standard_normal(n), numpy.round(1.0 + 0.01 * rng.standard_normal(n), 2), numpy.full(n, 0.5),
            1e-300 * (1.0 + rng.random(n)), 1e300 * (1.0 + rng.random(n))]
    spikes = numpy.ones(n)
    spikes[::13] = 4.0
    rows.append(spikes)
    for y in rows:
        for wl, bt in ((0.3, 0.5), (0.01, 0.5), (3.0, 0.5), (3.0, numpy.inf)):
            flat, trend = mirror_detrend(t, y, wl, bt)
            want_flat, want_trend = spec.detrend(t, y, wl, bt)
            assert numpy.array_equal(_bits(trend), _bits(want_trend)), (n, wl, bt)
            assert numpy.array_equal(_bits(flat), _bits(want_flat))


def test_plan_fits_the_lds():
    """The largest span of every plan fits its sort (P) and the LDS it asks for, 12 P + 8 smax <= 160 KiB, and a tile has
    at least 4 outputs, up to windows of BIWEIGHT_MAX_WINDOW points."""
    rng = numpy.random.default_rng(2)
    for n, cadence in ((5000, 1.0), (20000, 1.0), (9000, None)):
        t = numpy.arange(float(n)) if cadence else numpy.cumsum(rng.uniform(0.0, 2.0, n))
        for w in (1, 2, 25, 361, 1000, 2049, _lib.BIWEIGHT_MAX_WINDOW):
            try:
                lo, hi = _lib.biweight_windows(t, max(w - 1.0, 0.5) if cadence else float(w), numpy.inf)[3:]
            except ValueError:   # (irregular stamps: a window over the cap)
                continue
            T, P, smax = plan_of(lo, hi)
            assert P & (P - 1) == 0 and 64 <= P <= 8192 and smax <= P
            assert 12 * P + 8 * smax <= 160 * 1024
            assert T >= min(4, n)
    lo, hi = _lib.biweight_windows(numpy.arange(9000.0), _lib.BIWEIGHT_MAX_WINDOW - 1.0, numpy.inf)[3:]
    assert (hi - lo).max() == _lib.BIWEIGHT_MAX_WINDOW and plan_of(lo, hi) == (4, 8192, 4 + 2 * 2047)


# ---- stand-in contexts: what the survey functions ask a device to do, in order

class Recorder(object):
    """A context stand-in: records every call, forms rows on the host (detrend with the restatement), searches nothing."""

    def __init__(self):
        self.calls = []
        self.searched = []

    def inject_transits(self, t, flux, constants, u1, u2):
        m = len(constants)
        self.calls.append(("inject", m))
        rows = numpy.array(numpy.broadcast_to(flux, (m, len(t))))
        rows[:, ::50] *= 0.999
        return rows, numpy.arange(m, dtype=numpy.int64)

    def null_rows(self, n, n_rows, seed, first_trial=0, sigma=None, source=None, block=None):
        self.calls.append(("null", int(first_trial), int(n_rows)))
        return numpy.array([1.0 + 1e-3 * numpy.random.default_rng(first_trial + r).standard_normal(n) for r in range(n_rows)])

    def biweight_detrend(self, t, y, window_length, break_tolerance, return_trend=False):
        t, rows, wl, bt = _lib.biweight_arguments(t, y, window_length, break_tolerance)
        self.calls.append(("biweight", len(rows), wl, bt))
        flat, trend = spec.detrend(t, rows, wl, bt)
        if numpy.ndim(y) == 1:
            flat, trend = flat[0], trend[0]
        return (flat, trend) if return_trend else flat

    def medfilt_detrend(self, y, kernel, return_trend=False):
        raise AssertionError("a Biweight must not reach the median filter")

    def _power_batch(self, t, y_rows, dy_rows, periods, table, params, kernel, **kw):
        self.calls.append(("search", len(y_rows)))
        self.searched.append(numpy.array(y_rows))
        summary = numpy.zeros(len(y_rows), dtype=_lib.POWER_SUMMARY_DTYPE)
        summary["no_fit"] = 1
        return dict(summary=summary)

    def search_batch(self, t, y_rows, dy_rows, periods, table, params):
        self.calls.append(("search", len(y_rows)))
        self.searched.append(numpy.array(y_rows))
        z = numpy.zeros((len(y_rows), len(periods)))
        return z, z.astype(numpy.int64), z


T = numpy.linspace(1.0, 21.0, 400)
KW = dict(period_min=2.0, period_max=3.0, oversampling_factor=2)
BW = survey.Biweight(0.5, 0.25)


def _flux(m, seed=1):
    rng = numpy.random.default_rng(seed)
    return (1.0 + 0.01 * numpy.sin(T / 3.0)) * (1.0 + 1e-3 * rng.standard_normal((m, len(T))))


INJ = dict(T0=[1.0, 1.5, 2.0, 2.5, 3.0], period=[2.5] * 5, rp_rs=[0.05] * 5, a=[10.0] * 5, inc=[90.0] * 5)


def test_biweight_value():
    assert survey.Biweight(0.7) == (0.7, 0.5) and survey.Biweight(0.7).break_tolerance == 0.5
    assert survey.Biweight(1.0, 2.0).window_length == 1.0
    with pytest.raises(AttributeError):
        survey.Biweight(1.0).window_length = 2.0


def test_biweight_batch_records_one_call_and_keeps_the_shape():
    f = _flux(3)
    ctx = Recorder()
    flat, trend = survey.biweight_batch(T, f, 0.5, 0.25, return_trend=True, context=ctx)
    assert ctx.calls == [("biweight", 3, 0.5, 0.25)]
    want_flat, want_trend = spec.detrend(T, f, 0.5, 0.25)
    assert numpy.array_equal(trend, want_trend) and numpy.array_equal(flat, want_flat) and flat.shape == f.shape
    one = survey.biweight_batch(T, f[0], context=ctx)
    assert one.shape == (len(T),) and numpy.array_equal(one, spec.detrend(T, f[0], 0.5, 0.5)[0])


@pytest.mark.parametrize("call", ["search_batch", "power_batch", "power_results"])
def test_batch_search_detrends_first(call):
    f = _flux(3)
    ctx = Recorder()
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # (no "Ignoring unknown parameter": detrend is the call's own keyword)
        try:
            getattr(survey, call)(T, f, context=ctx, detrend=BW, **KW)
        except Exception:
            if call != "power_results":   # (the stand-in's summary has no statistics: power_results stops behind the search)
                raise
    assert ctx.calls == [("biweight", 3, 0.5, 0.25), ("search", 3)]
    assert numpy.array_equal(ctx.searched[0], spec.detrend(T, f, 0.5, 0.25)[0])


def test_injection_recovery_detrends_each_chunk_after_injecting():
    f = _flux(1)[0]
    ctx = Recorder()
    rec, summary, rows = survey.injection_recovery(T, f, INJ, chunk=2, return_rows=True, context=ctx, detrend=BW, **KW)
    b = ("biweight", 2, 0.5, 0.25)
    assert ctx.calls == [("inject", 2), b, ("search", 2), ("inject", 2), b, ("search", 2),
                         ("inject", 1), ("biweight", 1, 0.5, 0.25), ("search", 1)]
    raw = numpy.array(numpy.broadcast_to(f, (5, len(T))))
    raw[:, ::50] *= 0.999
    want = spec.detrend(T, raw, 0.5, 0.25)[0]
    assert numpy.array_equal(rows, want) and numpy.array_equal(numpy.concatenate(ctx.searched), want)
    assert rec["n_in_transit"].tolist() == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("mode", ["white", "bootstrap"])
def test_null_sde_detrends_each_chunk_after_forming(mode):
    kw = dict(sigma=1e-3) if mode == "white" else dict(source=_flux(2), block=20)
    ctx = Recorder()
    summary, rows = survey.null_sde(T, 5, chunk=3, first_trial=4, return_rows=True, context=ctx, detrend=BW, **kw, **KW)
    assert ctx.calls == [("null", 4, 3), ("biweight", 3, 0.5, 0.25), ("search", 3), ("null", 7, 2),
                         ("biweight", 2, 0.5, 0.25), ("search", 2)]
    raw = numpy.array([1.0 + 1e-3 * numpy.random.default_rng(4 + r).standard_normal(len(T)) for r in range(5)])
    want = spec.detrend(T, raw, 0.5, 0.25)[0]
    assert numpy.array_equal(rows, want) and numpy.array_equal(numpy.concatenate(ctx.searched), want)


# ---- argument errors: ValueError before any device work

BAD = [survey.Biweight(0.0), survey.Biweight(-1.0), survey.Biweight(numpy.inf), survey.Biweight(numpy.nan),
       survey.Biweight(0.5, 0.0), survey.Biweight(0.5, -0.5), survey.Biweight(0.5, numpy.nan), survey.Biweight("0.5"),
       survey.Biweight(True), survey.Biweight(0.5, None), survey.Biweight(1e6)]   # (the last: one window of 400 points > ...)


def _calls(f, detrend, t=T):
    yield lambda ctx: survey.biweight_batch(t, f, detrend.window_length, detrend.break_tolerance, context=ctx)
    for call in (survey.search_batch, survey.power_batch, survey.power_results):
        yield lambda ctx, call=call: call(t, f, context=ctx, detrend=detrend, **KW)
    yield lambda ctx: survey.injection_recovery(t, f[0], INJ, context=ctx, detrend=detrend, **KW)
    yield lambda ctx: survey.null_sde(t, 3, sigma=1e-3, context=ctx, detrend=detrend, **KW)


def _refused(fn, match=None):
    ctx = Recorder()
    with pytest.raises(ValueError, match=match):
        fn(ctx)
    assert ctx.calls == []


def test_argument_errors(monkeypatch):
    monkeypatch.setattr(_lib, "BIWEIGHT_MAX_WINDOW", 399)     # (a window over the cap at 400 points)
    f = _flux(2)
    for bw in BAD:
        for fn in _calls(f, bw):
            _refused(fn)
    for fn in _calls(f, survey.Biweight(1e6)):
        _refused(fn, "BIWEIGHT_MAX_WINDOW")
    for bad_t in (T[::-1], numpy.where(numpy.arange(len(T)) == 7, numpy.nan, T), T[None, :], T[:-1]):
        fns = list(_calls(f, survey.Biweight(0.5), t=bad_t))
        for fn in [fns[0], fns[4]] + ([fns[5]] if len(bad_t) == len(T) else []):   # (null_sde takes any n)
            _refused(fn)
    for bad in (numpy.nan, numpy.inf, -numpy.inf, 0.0, -1.0):
        g = f.copy()
        g[1, 17] = bad
        for fn in list(_calls(g, survey.Biweight(0.5)))[:3]:
            _refused(fn, "non-positive")
        g[0, 17] = bad
        _refused(list(_calls(g, survey.Biweight(0.5)))[4], "non-positive")
    for shape in ((2, 3, len(T)), (2, 0), (), (2, len(T) + 1)):
        _refused(lambda ctx: survey.biweight_batch(T, numpy.ones(shape), context=ctx), "shape")
    _refused(lambda ctx: survey.power_batch(T, f[0], context=ctx, detrend=survey.Biweight(0.5), **KW), "shape")


def test_medfilt_detrend_unchanged():
    """detrend=k still takes the median filter (test_detrend_host.py pins its calls and errors)."""
    calls = []

    class Med(Recorder):
        def medfilt_detrend(self, y, kernel, return_trend=False):
            calls.append(kernel)
            return numpy.asarray(y)

    survey.search_batch(T, _flux(2), context=Med(), detrend=25, **KW)
    assert calls == [25]
