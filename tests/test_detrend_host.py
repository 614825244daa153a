"""Median-filter detrending without a GPU: the tls_medfilt_detrend declaration against its binding, a numpy restatement of
the kernel's selection (tiles, zero-padded span, bitonic sort, scan) against scipy.signal.medfilt bit for bit, the argument
errors (raised before any device work), and the order of calls behind detrend= in the survey functions, with stand-in
contexts that record what they are asked to do."""
import ctypes
import os
import re
import warnings

import numpy
import pytest
from scipy.signal import medfilt

from tls_amd import _lib, survey
from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "tls_amd.h")).read()


# ---- header and binding

def test_declaration_matches_argtypes():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"int\s+tls_medfilt_detrend\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "tls_medfilt_detrend is not declared"
    c_types = {"tls_ctx *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "const double *": _lib._c_double_p,
               "double *": _lib._c_double_p}
    want = []
    for p in m.group(1).split(","):
        words = p.replace("*", " * ").split()[:-1]   # (the type without the parameter's name)
        want.append(c_types[" ".join(words).replace(" *", " *")])
    got = _lib.load().tls_medfilt_detrend.argtypes
    assert len(got) == len(want) == 7
    assert list(got) == want
    assert _lib.load().tls_medfilt_detrend.restype == ctypes.c_int
    assert "tls_medfilt_detrend" in _lib.SYMBOLS


def test_max_kernel_mirrored_and_abi_8():
    m = re.search(r"#define TLS_MEDFILT_MAX_KERNEL (\d+)\b", _header())
    assert m and int(m.group(1)) == _lib.MEDFILT_MAX_KERNEL >= 4095
    assert _lib.ABI_VERSION == 8
    assert _lib.load().tls_abi_version() == 8
    assert re.search(r"#define TLS_AMD_ABI_VERSION 8\b", _header())


# ---- a numpy restatement of the kernel's selection (tls_detrend.hip.h, tls_medfilt_detrend's span choice)

def span_of(n, k):
    """detrend_span: P = a power of two >= 64, about 2 (k - 1) and at least 256, capped by the whole row's span."""
    assert 1 <= k <= min(n, _lib.MEDFILT_MAX_KERNEL) and k % 2 == 1
    def pow2(v):
        p = 64
        while p < v:
            p <<= 1
        return p
    return min(pow2(max(2 * (k - 1), 256)), pow2(n + k - 1))


def bitonic(keys, slots):
    """The kernel's bitonic network over P pairs, ascending by key, compare-exchange by compare-exchange."""
    P = len(keys)
    t = numpy.arange(P // 2)
    size = 2
    while size <= P:
        stride = size // 2
        while stride > 0:
            i = 2 * t - (t & (stride - 1))
            j = i + stride
            ki, kj = keys[i], keys[j]
            up = (i & size) == 0
            swap = numpy.where(up, ki > kj, ki < kj)
            a, b = i[swap], j[swap]
            keys[a], keys[b] = kj[swap], ki[swap]
            slots[a], slots[b] = slots[b].copy(), slots[a].copy()
            stride //= 2
        size *= 2
    return keys, slots


def mirror_medfilt(y, k):
    """(flat, trend) of one row as the kernel forms them: per tile, the zero-padded span staged, sorted once, then each output
    counts the sorted slots inside its window four at a time and finishes inside the group that reaches k // 2 + 1."""
    n, h = len(y), k // 2
    P = span_of(n, k)
    T = P - (k - 1)
    S = T + k - 1
    bits = y.view(numpy.uint64)
    trend = numpy.empty(n)
    need = h + 1
    for lo in range(0, n, T):
        g = lo - h + numpy.arange(P)
        inside = (g >= 0) & (g < n) & (numpy.arange(P) < S)
        keys = numpy.where(numpy.arange(P) < S, numpy.uint64(0), numpy.uint64(2 ** 64 - 1)).astype(numpy.uint64)
        keys[inside] = bits[g[inside]]
        slots = numpy.where(numpy.arange(P) < S, numpy.arange(P), 2 ** 32 - 1).astype(numpy.uint32)
        keys, slots = bitonic(keys, slots)
        i = numpy.arange(min(T, n - lo), dtype=numpy.uint32)
        hit = ((slots[None, :] - i[:, None]) < numpy.uint32(k)).astype(numpy.int64)   # (uint32 wrap-around, as on the device)
        c = numpy.cumsum(hit, axis=1)
        group = numpy.argmax(c[:, 3::4] >= need, axis=1)           # the first group of four that reaches need
        assert numpy.all(c[numpy.arange(len(i)), 4 * group + 3] >= need)
        j = 4 * group
        f = j + sum((c[numpy.arange(len(i)), j + u] < need).astype(numpy.int64) for u in range(3))
        assert numpy.all(f < S)
        trend[lo: lo + len(i)] = keys[f].view(numpy.float64)
    return y / trend, trend


def _rows(rng):
    """Random, tie-heavy, constant and monotone rows, spikes and extreme magnitudes."""
    out = [1.0 + 1e-3 * rng.standard_normal(500),
           numpy.round(1.0 + 0.01 * rng.standard_normal(500), 2),            # a few levels: heavy ties
           numpy.full(300, 1.25),
           numpy.linspace(0.5, 2.0, 333), numpy.linspace(2.0, 0.5, 333),
           1e-300 * (1.0 + rng.random(257)), 1e300 * (1.0 + rng.random(257))]
    spikes = numpy.ones(400)
    spikes[::37] = 5.0
    spikes[5::41] = 0.1
    out.append(spikes)
    t = numpy.linspace(0.0, 30.0, 700)
    out.append((1.0 + 0.02 * numpy.sin(t / 5.0)) * (1.0 + 5e-4 * rng.standard_normal(700)))
    return out


@pytest.mark.parametrize("k", [1, 3, 5, 25, 101, 361])
def test_mirror_equals_scipy(k):
    rng = numpy.random.default_rng(k)
    for y in _rows(rng):
        if k > len(y):
            continue
        flat, trend = mirror_medfilt(y, k)
        want = medfilt(y, k)
        assert numpy.array_equal(trend.view(numpy.uint64), want.view(numpy.uint64)), (k, len(y))
        assert numpy.array_equal(flat.view(numpy.uint64), (y / want).view(numpy.uint64))
        assert numpy.all(trend > 0)


def test_mirror_equals_scipy_at_the_edges_of_the_range():
    rng = numpy.random.default_rng(7)
    for n in (1, 2, 3, 7, 64, 65):
        y = 1.0 + 0.1 * rng.random(n)
        for k in range(1, n + 1, 2):
            assert numpy.array_equal(mirror_medfilt(y, k)[1], medfilt(y, k)), (n, k)
    y = 1.0 + 1e-3 * rng.standard_normal(4200)          # the largest kernel: P = 8192, two tiles
    k = _lib.MEDFILT_MAX_KERNEL
    assert span_of(4200, k) == 8192
    assert numpy.array_equal(mirror_medfilt(y, k)[1], medfilt(y, k))
    y = numpy.round(1.0 + 0.01 * rng.standard_normal(1500), 2)   # many tiles, ties across their seams
    assert numpy.array_equal(mirror_medfilt(y, 25)[1], medfilt(y, 25))
    assert numpy.array_equal(mirror_medfilt(numpy.ones(9), 1)[0], numpy.ones(9))   # k = 1: trend = y, flat = 1 exactly


def test_span_fits_the_lds():
    for k in (1, 25, 361, 2047, 2049, _lib.MEDFILT_MAX_KERNEL):
        for n in (k, k + 1, 10 * k + 7, 100000):
            P = span_of(n, k)
            assert P & (P - 1) == 0 and 64 <= P <= 8192 and P - (k - 1) >= 1
            assert 12 * P <= 160 * 1024


# ---- stand-in contexts: what the survey functions ask a device to do, in order

class Recorder(object):
    """A context stand-in: records every call, forms rows on the host (detrend with scipy), searches nothing."""

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

    def medfilt_detrend(self, y, kernel, return_trend=False):
        rows, k = _lib.medfilt_arguments(y, kernel)
        self.calls.append(("detrend", len(rows), k))
        trend = numpy.array([medfilt(r, k) for r in rows])
        flat = rows / trend
        if numpy.ndim(y) == 1:
            flat, trend = flat[0], trend[0]
        return (flat, trend) if return_trend else flat

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


def _flux(m, seed=1):
    rng = numpy.random.default_rng(seed)
    return (1.0 + 0.01 * numpy.sin(T / 3.0)) * (1.0 + 1e-3 * rng.standard_normal((m, len(T))))


INJ = dict(T0=[1.0, 1.5, 2.0, 2.5, 3.0], period=[2.5] * 5, rp_rs=[0.05] * 5, a=[10.0] * 5, inc=[90.0] * 5)


def test_detrend_batch_records_one_call_and_keeps_the_shape():
    f = _flux(3)
    ctx = Recorder()
    flat, trend = survey.detrend_batch(f, 25, return_trend=True, context=ctx)
    assert ctx.calls == [("detrend", 3, 25)]
    assert numpy.array_equal(trend, numpy.array([medfilt(r, 25) for r in f])) and numpy.array_equal(flat, f / trend)
    one = survey.detrend_batch(f[0], 5, context=ctx)
    assert one.shape == (len(T),) and numpy.array_equal(one, f[0] / medfilt(f[0], 5))


@pytest.mark.parametrize("call", ["search_batch", "power_batch", "power_results"])
def test_batch_search_detrends_first(call):
    f = _flux(3)
    ctx = Recorder()
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # (no "Ignoring unknown parameter": detrend is the call's own keyword)
        try:
            getattr(survey, call)(T, f, context=ctx, detrend=25, **KW)
        except Exception:
            if call != "power_results":   # (the stand-in's summary has no statistics: power_results stops behind the search)
                raise
    assert ctx.calls == [("detrend", 3, 25), ("search", 3)]
    assert numpy.array_equal(ctx.searched[0], f / numpy.array([medfilt(r, 25) for r in f]))
    ctx = Recorder()
    if call != "power_results":
        getattr(survey, call)(T, f, context=ctx, **KW)
        assert ctx.calls == [("search", 3)]
        assert numpy.array_equal(ctx.searched[0], f)


def test_injection_recovery_detrends_each_chunk_after_injecting():
    f = _flux(1)[0]
    ctx = Recorder()
    rec, summary, rows = survey.injection_recovery(T, f, INJ, chunk=2, return_rows=True, context=ctx, detrend=25, **KW)
    assert ctx.calls == [("inject", 2), ("detrend", 2, 25), ("search", 2), ("inject", 2), ("detrend", 2, 25), ("search", 2),
                         ("inject", 1), ("detrend", 1, 25), ("search", 1)]
    raw = numpy.array(numpy.broadcast_to(f, (5, len(T))))
    raw[:, ::50] *= 0.999
    want = raw / numpy.array([medfilt(r, 25) for r in raw])
    assert numpy.array_equal(rows, want) and numpy.array_equal(numpy.concatenate(ctx.searched), want)
    assert rec["n_in_transit"].tolist() == [0, 1, 0, 1, 0]   # (the stand-in's counts per chunk, unchanged)
    ctx = Recorder()
    survey.injection_recovery(T, f, INJ, chunk=2, context=ctx, **KW)
    assert ctx.calls == [("inject", 2), ("search", 2), ("inject", 2), ("search", 2), ("inject", 1), ("search", 1)]


@pytest.mark.parametrize("mode", ["white", "bootstrap"])
def test_null_sde_detrends_each_chunk_after_forming(mode):
    kw = dict(sigma=1e-3) if mode == "white" else dict(source=_flux(2), block=20)
    ctx = Recorder()
    summary, rows = survey.null_sde(T, 5, chunk=3, first_trial=4, return_rows=True, context=ctx, detrend=11, **kw, **KW)
    assert ctx.calls == [("null", 4, 3), ("detrend", 3, 11), ("search", 3), ("null", 7, 2), ("detrend", 2, 11), ("search", 2)]
    raw = numpy.array([1.0 + 1e-3 * numpy.random.default_rng(4 + r).standard_normal(len(T)) for r in range(5)])
    want = raw / numpy.array([medfilt(r, 11) for r in raw])
    assert numpy.array_equal(rows, want) and numpy.array_equal(numpy.concatenate(ctx.searched), want)
    ctx = Recorder()
    survey.null_sde(T, 5, chunk=3, first_trial=4, context=ctx, **kw, **KW)
    assert ctx.calls == [("null", 4, 3), ("search", 3), ("null", 7, 2), ("search", 2)]


# ---- argument errors: ValueError before any device work

BAD_KERNELS = [4, 0, -3, 2.0, 25.0, True, False, "25", 401]   # (401 > n = 400)


def test_detrend_batch_argument_errors():
    f = _flux(2)
    for k in BAD_KERNELS + [None]:
        ctx = Recorder()
        with pytest.raises(ValueError):
            survey.detrend_batch(f, k, context=ctx)
        assert ctx.calls == []
    big = numpy.ones(_lib.MEDFILT_MAX_KERNEL + 4)
    with pytest.raises(ValueError, match="MEDFILT_MAX_KERNEL"):
        survey.detrend_batch(big, _lib.MEDFILT_MAX_KERNEL + 2, context=Recorder())
    for bad in (numpy.nan, numpy.inf, -numpy.inf, 0.0, -1.0):
        g = f.copy()
        g[1, 17] = bad
        ctx = Recorder()
        with pytest.raises(ValueError, match="non-positive"):
            survey.detrend_batch(g, 25, context=ctx)
        assert ctx.calls == []
    for shape in ((2, 3, 4), (2, 0), ()):
        with pytest.raises(ValueError, match="shape"):
            survey.detrend_batch(numpy.ones(shape), 1, context=Recorder())


def test_survey_detrend_argument_errors():
    f = _flux(2)
    for k in BAD_KERNELS:
        for call in (survey.search_batch, survey.power_batch, survey.power_results):
            ctx = Recorder()
            with pytest.raises(ValueError):
                call(T, f, context=ctx, detrend=k, **KW)
            assert ctx.calls == []
        ctx = Recorder()
        with pytest.raises(ValueError):
            survey.injection_recovery(T, f[0], INJ, context=ctx, detrend=k, **KW)
        assert ctx.calls == []
        ctx = Recorder()
        with pytest.raises(ValueError):
            survey.null_sde(T, 3, sigma=1e-3, context=ctx, detrend=k, **KW)
        assert ctx.calls == []
    g = f.copy()
    g[0, 3] = numpy.nan
    for call in (survey.search_batch, survey.power_batch):
        ctx = Recorder()
        with pytest.raises(ValueError, match="non-positive"):
            call(T, g, context=ctx, detrend=25, **KW)
        assert ctx.calls == []
    ctx = Recorder()
    with pytest.raises(ValueError, match="non-positive"):
        survey.injection_recovery(T, g[0], INJ, context=ctx, detrend=25, **KW)
    assert ctx.calls == []
    ctx = Recorder()
    with pytest.raises(ValueError, match="shape"):
        survey.power_batch(T, f[0], context=ctx, detrend=25, **KW)
    assert ctx.calls == []
