"""SysRem without a GPU: the tls_sysrem declaration and constants against the binding, hand-worked cases of the restatement
(sysrem_spec), a numpy restatement of the kernels' partition (chunk grid, lane strides, tree) against it, the argument errors
(raised before any device work), the order of calls behind detrend=SysRem(...) and behind a tuple of steps in the survey
functions, with stand-in contexts that record what they are asked to do, and the science check on the restatement alone."""
import ctypes
import os
import re
import warnings

import numpy
import pytest

from tls_amd import _lib, survey
from tls_amd.search import DeviceGroup
from conftest import REPO
import biweight_spec
import sysrem_spec as spec


def _header():
    return open(os.path.join(REPO, "include", "tls_amd.h")).read()


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


# ---- header and binding

def test_declaration_matches_argtypes():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"int\s+tls_sysrem\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "tls_sysrem is not declared"
    c_types = {"tls_ctx *": ctypes.c_void_p, "int64_t": ctypes.c_int64, "const double *": _lib._c_double_p,
               "double *": _lib._c_double_p, "double": ctypes.c_double, "int64_t *": _lib._c_int64_p}
    want = []
    for p in m.group(1).split(","):
        words = p.replace("*", " * ").split()[:-1]   # (the type without the parameter's name)
        want.append(c_types[" ".join(words).replace(" *", " *")])
    got = _lib.load().tls_sysrem.argtypes
    assert len(got) == len(want) == 13
    assert list(got) == want
    assert _lib.load().tls_sysrem.restype == ctypes.c_int
    assert "tls_sysrem" in _lib.SYMBOLS
    assert re.search(r"Entries added without changing a layout.*tls_sysrem\)", _header(), flags=re.S)


def test_constants_mirrored_and_abi_8():
    h = _header()
    for name, mine, its in (("LANES", _lib.SYSREM_LANES, spec.LANES), ("ROW_CHUNK", _lib.SYSREM_ROW_CHUNK, spec.ROW_CHUNK),
                            ("MAX_COMPONENTS", _lib.SYSREM_MAX_COMPONENTS, spec.MAX_COMPONENTS),
                            ("MAX_ITER", _lib.SYSREM_MAX_ITER, spec.MAX_ITER)):
        m = re.search(r"#define TLS_SYSREM_%s (\d+)\b" % name, h)
        assert m and int(m.group(1)) == mine == its, name
    assert (_lib.SYSREM_LANES, _lib.SYSREM_ROW_CHUNK, _lib.SYSREM_MAX_COMPONENTS, _lib.SYSREM_MAX_ITER) == (256, 32, 8, 1000)
    assert _lib.ABI_VERSION == 8
    assert _lib.load().tls_abi_version() == 8
    assert re.search(r"#define TLS_AMD_ABI_VERSION 8\b", h)


# ---- hand-worked cases of the restatement

def test_rowsum_order():
    v = numpy.zeros(514)
    v[0], v[256], v[512] = 1e16, 1.0, -1e16          # all in lane 0: (1e16 + 1) + -1e16, the 1 is lost
    v[1] = 1.0                                       # lane 1 keeps its own
    assert spec.rowsum(v) == 1.0 and float(numpy.cumsum(v)[-1]) == 0.0
    w = numpy.zeros(300)
    w[0], w[128], w[1] = 1e16, -1e16, 1.0            # lanes 0 and 128 meet in the first fold, before lane 1 joins
    assert spec.rowsum(w) == 1.0 and float(numpy.cumsum(w)[-1]) == 0.0
    z = numpy.array([1e16, 1.0, -1e16, 1.0])         # lanes 0..3: (0 + 2) and (1 + 3), then their sum
    assert spec.rowsum(z) == (1e16 + -1e16) + (1.0 + 1.0) == 2.0
    assert float(numpy.cumsum(z)[-1]) == 1.0         # left to right loses the first 1
    assert spec.rowsum(numpy.zeros((3, 0))).tolist() == [0.0, 0.0, 0.0]
    rng = numpy.random.default_rng(0)
    v = rng.standard_normal((4, 1000))
    assert numpy.allclose(spec.rowsum(v), v.sum(axis=1), rtol=0, atol=1e-11)


def test_colsum_order():
    v = numpy.zeros(65)
    v[0], v[1], v[32] = 1e16, 1.0, -1e16             # chunk 0 = 1e16 + 1 = 1e16, chunk 1 = -1e16: 0, not 1
    assert spec.colsum(v) == 0.0 and (1e16 + -1e16) + 1.0 == 1.0
    v = numpy.zeros(65)
    v[0], v[32], v[33], v[64] = 1e16, 1.0, 1.0, -1e16   # chunk 1 = 2 survives next to 1e16, one at a time would not
    assert spec.colsum(v) == 2.0 and float(numpy.cumsum(v)[-1]) == 0.0
    cols = numpy.stack([v, numpy.arange(65.0)], axis=1)
    assert spec.colsum(cols).tolist() == [2.0, 2080.0]


def test_constant_row_has_no_weight():
    rng = numpy.random.default_rng(1)
    y = 1.0 + 1e-3 * rng.standard_normal((5, 40)) * (1.0 + numpy.linspace(-0.01, 0.01, 40))
    y[3] = 0.75
    flat, trend, c, a, iters = spec.fit(y, 2)
    assert c[3].tolist() == [0.0, 0.0] and numpy.all(trend[3] == 0.75) and numpy.all(flat[3] == 1.0)
    # ... and does not enter a: the fit of the other rows alone gives the same bits
    others = spec.fit(y[[0, 1, 2, 4]], 2)
    assert numpy.array_equal(_bits(others[3]), _bits(a)) and numpy.array_equal(_bits(others[0]), _bits(flat[[0, 1, 2, 4]]))


def test_column_without_coefficients_gives_a_zero_profile():
    y = numpy.full((3, 6), 2.0)                       # every row constant: every weight 0, every denominator 0
    flat, trend, c, a, iters = spec.fit(y, 1)
    assert numpy.all(a == 0.0) and numpy.all(c == 0.0) and iters.tolist() == [1] and numpy.all(flat == 1.0)
    assert not numpy.any(numpy.signbit(a))
    assert spec._ratio(numpy.array([1.0, -1.0, 0.0]), numpy.array([0.0, -2.0, numpy.nan])).tolist() == [0.0, 0.0, 0.0]


def test_rank_one_is_removed_by_one_component():
    rng = numpy.random.default_rng(2)
    c0 = rng.uniform(0.5, 2.0, 9)
    a0 = 1e-2 * numpy.sin(numpy.arange(50.0))
    a0 -= a0.mean()
    y = 3.0 * (1.0 + c0[:, None] * a0[None, :])
    flat, trend, c, a, iters = spec.fit(y, 1, max_iter=20)
    assert iters[0] <= 3
    assert numpy.max(numpy.abs(flat - 1.0)) <= 8 * numpy.finfo(float).eps
    assert numpy.max(numpy.abs(c[:, 0][:, None] * a[0][None, :] - c0[:, None] * a0[None, :])) <= 1e-16
    # rank one with every step exact in binary (m = 1, w = 2^16, a = 2 a0 and c = c0 / 2 from the first iteration on): the
    # second iteration repeats the first, the residual is an exact zero, and the second component stops at once
    c0 = numpy.array([1.0, 2.0, 4.0, 1.0])
    a0 = numpy.array([1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 2.0, -2.0]) / 64.0
    y = 1.0 + c0[:, None] * a0[None, :]
    flat, trend, c, a, iters = spec.fit(y, 2, dy=numpy.full(y.shape, 2.0 ** -8), max_iter=20, tol=0.0)
    assert iters.tolist() == [2, 1] and numpy.array_equal(a[0], 2.0 * a0) and numpy.array_equal(c[:, 0], c0 / 2.0)
    assert numpy.all(a[1] == 0.0) and numpy.all(c[:, 1] == 0.0) and numpy.array_equal(trend, y)
    assert numpy.max(numpy.abs(flat - 1.0)) <= 4 * numpy.finfo(float).eps


def test_tol_zero_runs_every_iteration():
    rng = numpy.random.default_rng(3)
    y = 1.0 + 1e-3 * rng.standard_normal((6, 30)) + 1e-2 * rng.standard_normal(6)[:, None] * numpy.linspace(-1, 1, 30)
    assert spec.fit(y, 2, max_iter=9, tol=0.0)[4].tolist() == [9, 9]
    assert spec.fit(y, 1, max_iter=200, tol=1e-3)[4][0] < 200


# ---- a numpy restatement of the kernels' partition (tls_sysrem.hip.h) against the restatement

def kernel_rowsum(v):
    """tls_sysrem_rows / _prepare: thread l loops j = l, l + 256, ... < n; the LDS tree with a barrier a step."""
    p = numpy.zeros(_lib.SYSREM_LANES)
    for l in range(_lib.SYSREM_LANES):
        acc = 0.0
        for j in range(l, len(v), _lib.SYSREM_LANES):
            acc = acc + v[j]
        p[l] = acc
    s = _lib.SYSREM_LANES // 2
    while s >= 1:
        for l in range(s):
            p[l] = p[l] + p[l + s]
        s //= 2
    return p[0]


def kernel_colsum(v):
    """tls_sysrem_columns + _epochs: grid (ceil(n / 256), chunks), a thread a column of a chunk, then the chunks in order."""
    n_rows, n = v.shape
    chunks = -(-n_rows // _lib.SYSREM_ROW_CHUNK)
    partial = numpy.zeros((chunks, n))
    for bx in range(-(-n // _lib.SYSREM_LANES)):
        for q in range(chunks):
            for l in range(_lib.SYSREM_LANES):
                j = bx * _lib.SYSREM_LANES + l
                if j >= n:
                    continue
                acc = 0.0
                for i in range(q * _lib.SYSREM_ROW_CHUNK, min((q + 1) * _lib.SYSREM_ROW_CHUNK, n_rows)):
                    acc = acc + v[i, j]
                partial[q, j] = acc
    out = numpy.zeros(n)
    for j in range(n):
        acc = 0.0
        for q in range(chunks):
            acc = acc + partial[q, j]
        out[j] = acc
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_kernel_partition_equals_the_restatement(n):
    rng = numpy.random.default_rng(n)
    for n_rows in (2, 31, 32, 33, 65):
        v = rng.standard_normal((n_rows, n)) * 10.0 ** rng.integers(-8, 8, (n_rows, n))
        assert numpy.array_equal(_bits(kernel_colsum(v)), _bits(spec.colsum(v))), (n, n_rows)
        for i in (0, n_rows - 1):
            assert _bits(kernel_rowsum(v[i])) == _bits(spec.rowsum(v[i])), (n, n_rows, i)
        assert numpy.array_equal(_bits(spec.rowsum(v)), _bits([spec.rowsum(r) for r in v]))


# ---- stand-in contexts: what the survey functions ask a device to do, in order

class Recorder(object):
    """A context stand-in: records every call, forms rows on the host (with the restatements), searches nothing."""

    def __init__(self, device=0, log=None):
        self.device = device
        self.calls = [] if log is None else log
        self.searched = []

    def sysrem(self, y, n_components=1, dy=None, max_iter=50, tol=1e-6, return_trend=False, return_components=False):
        rows, dy, k, iters, tol = _lib.sysrem_arguments(y, n_components, dy, max_iter, tol)
        self.calls.append(("sysrem", self.device, len(rows), k, iters, tol, None if dy is None else float(dy[0, 0])))
        flat, trend, c, a, ran = spec.fit(rows, k, dy=dy, max_iter=iters, tol=tol)
        out = (flat,) + ((trend,) if return_trend else ()) + (((c, a, ran),) if return_components else ())
        return out[0] if len(out) == 1 else out

    def biweight_detrend(self, t, y, window_length, break_tolerance, return_trend=False):
        t, rows, wl, bt = _lib.biweight_arguments(t, y, window_length, break_tolerance)
        self.calls.append(("biweight", self.device, len(rows), wl, bt))
        return biweight_spec.detrend(t, rows, wl, bt)[0]

    def medfilt_detrend(self, y, kernel, return_trend=False):
        rows, k = _lib.medfilt_arguments(y, kernel)
        self.calls.append(("medfilt", self.device, len(rows), k))
        return rows * (1.0 + 2.0 ** -20)

    def inject_transits(self, t, flux, constants, u1, u2):
        self.calls.append(("inject", self.device, len(constants)))
        return numpy.array(numpy.broadcast_to(flux, (len(constants), len(t)))), numpy.zeros(len(constants), dtype=numpy.int64)

    def null_rows(self, n, n_rows, seed, first_trial=0, sigma=None, source=None, block=None):
        self.calls.append(("null", self.device, int(n_rows)))
        return numpy.ones((n_rows, n))

    def _power_batch(self, t, y_rows, dy_rows, periods, table, params, kernel, **kw):
        self.calls.append(("search", self.device, len(y_rows)))
        self.searched.append(numpy.array(y_rows))
        summary = numpy.zeros(len(y_rows), dtype=_lib.POWER_SUMMARY_DTYPE)
        summary["no_fit"] = 1
        return dict(summary=summary)

    def search_batch(self, t, y_rows, dy_rows, periods, table, params):
        self.calls.append(("search", self.device, len(y_rows)))
        self.searched.append(numpy.array(y_rows))
        z = numpy.zeros((len(y_rows), len(periods)))
        return z, z.astype(numpy.int64), z


T = numpy.linspace(1.0, 21.0, 120)
KW = dict(period_min=2.0, period_max=3.0, oversampling_factor=2)
SR = survey.SysRem(2, 30, 1e-5)
BW = survey.Biweight(0.5, 0.25)
INJ = dict(T0=[1.0, 1.5], period=[2.5] * 2, rp_rs=[0.05] * 2, a=[10.0] * 2, inc=[90.0] * 2)


def _flux(m, seed=1):
    rng = numpy.random.default_rng(seed)
    shared = 0.01 * numpy.sin(T / 3.0)
    return (1.0 + rng.uniform(0.5, 2.0, m)[:, None] * shared) * (1.0 + 1e-3 * rng.standard_normal((m, len(T))))


def test_sysrem_value():
    assert survey.SysRem() == (1, 50, 1e-6) and survey.SysRem(3).n_components == 3
    assert survey.SysRem(2, max_iter=7).max_iter == 7 and survey.SysRem(tol=0.0).tol == 0.0
    with pytest.raises(AttributeError):
        survey.SysRem(1).n_components = 2
    assert isinstance(SR, tuple) and survey._detrend_steps(SR) == (SR,)       # (a value, not a list of steps)
    assert survey._detrend_steps(None) == () and survey._detrend_steps(25) == (25,) and survey._detrend_steps(BW) == (BW,)
    assert survey._detrend_steps([SR, BW, 25]) == (SR, BW, 25)


def test_sysrem_batch_records_one_call():
    f = _flux(5)
    ctx = Recorder()
    flat, trend, (c, a, iters) = survey.sysrem_batch(f, 2, max_iter=30, tol=1e-5, return_trend=True, return_components=True,
                                                     context=ctx)
    assert ctx.calls == [("sysrem", 0, 5, 2, 30, 1e-5, None)]
    want = spec.fit(f, 2, max_iter=30, tol=1e-5)
    for got, w in zip((flat, trend, c, a, iters), want):
        assert numpy.array_equal(got, w)
    assert c.shape == (5, 2) and a.shape == (2, len(T)) and iters.shape == (2,)
    dy = numpy.full(f.shape, 2e-3)
    assert numpy.array_equal(survey.sysrem_batch(f, dy_batch=dy, context=ctx), spec.fit(f, 1, dy=dy)[0])
    assert ctx.calls[-1] == ("sysrem", 0, 5, 1, 50, 1e-6, 2e-3)
    with pytest.raises(TypeError):
        survey.sysrem_batch(f, devices=[0, 1])       # (the fit spans the batch)


@pytest.mark.parametrize("call", ["search_batch", "power_batch", "power_results"])
@pytest.mark.parametrize("which", ["sysrem", "sysrem_biweight", "sysrem_medfilt", "biweight_sysrem"])
def test_batch_search_detrends_first(call, which):
    detrend = dict(sysrem=SR, sysrem_biweight=(SR, BW), sysrem_medfilt=[SR, 5], biweight_sysrem=(BW, SR))[which]
    f = _flux(5)
    ctx = Recorder()
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # (no "Ignoring unknown parameter": detrend is the call's own keyword)
        try:
            getattr(survey, call)(T, f, context=ctx, detrend=detrend, **KW)
        except Exception:
            if call != "power_results":   # (the stand-in's summary has no statistics: power_results stops behind the search)
                raise
    s, b = ("sysrem", 0, 5, 2, 30, 1e-5, None), ("biweight", 0, 5, 0.5, 0.25)
    want_calls = {"sysrem": [s], "sysrem_biweight": [s, b], "sysrem_medfilt": [s, ("medfilt", 0, 5, 5)],
                  "biweight_sysrem": [b, s]}
    assert ctx.calls == want_calls[which] + [("search", 0, 5)]
    rows = f
    for step in detrend if which != "sysrem" else (detrend,):
        if isinstance(step, survey.SysRem):
            rows = spec.fit(rows, 2, max_iter=30, tol=1e-5)[0]
        elif isinstance(step, survey.Biweight):
            rows = biweight_spec.detrend(T, rows, 0.5, 0.25)[0]
        else:
            rows = rows * (1.0 + 2.0 ** -20)
    assert numpy.array_equal(ctx.searched[0], rows)


def test_dy_batch_weights_the_fit():
    f = _flux(4)
    dy = numpy.full(f.shape, 2e-3)
    ctx = Recorder()
    survey.search_batch(T, f, dy, context=ctx, detrend=survey.SysRem(1), **KW)
    assert ctx.calls == [("sysrem", 0, 4, 1, 50, 1e-6, 2e-3), ("search", 0, 4)]
    assert numpy.array_equal(ctx.searched[0], spec.fit(f, 1, dy=dy)[0])


def test_devices_fit_on_the_first_then_deal_the_rows_out():
    """One sysrem over the WHOLE batch on the first context, then the per-row steps and the search on every device's slice."""
    f = _flux(70, seed=4)
    log = []
    group = DeviceGroup([0, 1], context_factory=lambda d: Recorder(d, log))
    survey.search_batch(T, f, devices=group, detrend=(survey.SysRem(1, 20), BW), **KW)
    assert log[0] == ("sysrem", 0, 70, 1, 20, 1e-6, None)
    assert sorted(log[1:3]) == [("biweight", 0, 32, 0.5, 0.25), ("biweight", 1, 38, 0.5, 0.25)]
    assert sorted(log[3:]) == [("search", 0, 32), ("search", 1, 38)]
    want = biweight_spec.detrend(T, spec.fit(f, 1, max_iter=20)[0], 0.5, 0.25)[0]
    got = numpy.concatenate([group.contexts[0].searched[0], group.contexts[1].searched[0]])
    assert numpy.array_equal(got, want)


def test_single_star_calls_refuse_an_ensemble_fit():
    f = _flux(1)[0]
    for detrend in (SR, (SR, BW), [BW, SR], (25, survey.SysRem())):
        ctx = Recorder()
        with pytest.raises(ValueError, match="ONE star"):
            survey.injection_recovery(T, f, INJ, context=ctx, detrend=detrend, **KW)
        with pytest.raises(ValueError, match="ONE star"):
            survey.null_sde(T, 3, sigma=1e-3, context=ctx, detrend=detrend, **KW)
        assert ctx.calls == []


def test_single_star_calls_take_per_row_steps_in_order():
    f = _flux(1)[0]
    ctx = Recorder()
    survey.injection_recovery(T, f, INJ, context=ctx, detrend=(BW, 5), **KW)
    assert ctx.calls == [("inject", 0, 2), ("biweight", 0, 2, 0.5, 0.25), ("medfilt", 0, 2, 5), ("search", 0, 2)]
    ctx = Recorder()
    survey.null_sde(T, 3, sigma=1e-3, context=ctx, detrend=[5, BW], **KW)
    assert ctx.calls == [("null", 0, 3), ("medfilt", 0, 3, 5), ("biweight", 0, 3, 0.5, 0.25), ("search", 0, 3)]


# ---- argument errors: ValueError before any device work

def _refused(fn, match=None):
    ctx = Recorder()
    with pytest.raises(ValueError, match=match):
        fn(ctx)
    assert ctx.calls == []


def _calls(f, sr, dy=None):
    yield lambda ctx: survey.sysrem_batch(f, sr.n_components, dy_batch=dy, max_iter=sr.max_iter, tol=sr.tol, context=ctx)
    for call in (survey.search_batch, survey.power_batch, survey.power_results):
        yield lambda ctx, call=call: call(T, f, dy, context=ctx, detrend=sr, **KW)
        yield lambda ctx, call=call: call(T, f, dy, context=ctx, detrend=(sr, BW), **KW)


BAD = [survey.SysRem(0), survey.SysRem(-1), survey.SysRem(4), survey.SysRem(9), survey.SysRem(1.0), survey.SysRem(True),
       survey.SysRem("1"), survey.SysRem(None), survey.SysRem(1, 0), survey.SysRem(1, 1001), survey.SysRem(1, 2.5),
       survey.SysRem(1, 50, -1e-9), survey.SysRem(1, 50, numpy.nan), survey.SysRem(1, 50, numpy.inf), survey.SysRem(1, 50, "x"),
       survey.SysRem(1, 50, None), survey.SysRem(1, 50, True)]


def test_argument_errors():
    f = _flux(4)                                      # (4 rows: at most 3 components)
    for sr in BAD:
        for fn in _calls(f, sr):
            _refused(fn)
    for bad in (numpy.nan, numpy.inf, -numpy.inf, 0.0, -1.0):
        g = f.copy()
        g[1, 17] = bad
        for fn in _calls(g, survey.SysRem()):
            _refused(fn, "non-positive")
        for fn in _calls(f, survey.SysRem(), dy=g):
            _refused(fn)
    for shape in ((2, 3, len(T)), (1, len(T)), (len(T),), (3, 0), ()):
        _refused(lambda ctx: survey.sysrem_batch(numpy.ones(shape), context=ctx), "shape")
    _refused(lambda ctx: survey.sysrem_batch(f, dy_batch=numpy.ones((4, len(T) - 1)), context=ctx), "shape")
    _refused(lambda ctx: survey.power_batch(T, f[:1], context=ctx, detrend=survey.SysRem(), **KW), "shape")
    _refused(lambda ctx: survey.power_batch(T, f[0], context=ctx, detrend=survey.SysRem(), **KW), "shape")
    for steps in ((survey.SysRem(), None), (survey.SysRem(), (BW, 5)), [[5]]):
        _refused(lambda ctx: survey.search_batch(T, f, context=ctx, detrend=steps, **KW), "step")
    assert _lib.sysrem_arguments(f, 3, None, 1000, 0.0)[2:] == (3, 1000, 0.0)
    assert _lib.sysrem_arguments(f, numpy.int64(2), None, numpy.int32(7), numpy.float32(0.5))[2:] == (2, 7, 0.5)


def test_other_detrend_values_unchanged():
    """None, a kernel size and a Biweight still take the paths they took (test_detrend_host.py and test_biweight_host.py
    pin their calls and errors): one call of the filter, then the search."""
    f = _flux(3)
    for detrend, want in ((None, []), (5, [("medfilt", 0, 3, 5)]), (BW, [("biweight", 0, 3, 0.5, 0.25)]), ((), [])):
        ctx = Recorder()
        survey.search_batch(T, f, context=ctx, detrend=detrend, **KW)
        assert ctx.calls == want + [("search", 0, 3)]


# ---- the science check, on the restatement alone

def test_shared_systematics_are_removed_and_the_transit_stays():
    """64 stars at 4320 epochs (90 d at 48 a day), white noise of 2e-4 to 6e-4, a ramp and a 6-day sawtooth shared with
    per-star coefficients of a few 1e-3 (seed 7); star 0 carries a 0.4 % transit.  Measured with this restatement: median rms /
    sigma 2.53 raw, 1.52 behind one component, 0.990 behind two (0.988 and 0.994 with seeds 1 and 2), depth kept 0.956."""
    rng = numpy.random.default_rng(7)
    n_rows, n = 64, 4320
    t = numpy.arange(n) / 48.0
    sigma = rng.uniform(2e-4, 6e-4, n_rows)
    ramp = (t - t.mean()) / (t.max() - t.min())
    saw = (t % 6.0) / 6.0 - 0.5
    c1, c2 = rng.normal(0.0, 3e-3, n_rows), rng.normal(0.0, 3e-3, n_rows)
    y = 1.0 + sigma[:, None] * rng.standard_normal((n_rows, n)) + c1[:, None] * ramp + c2[:, None] * saw
    in_transit = ((t - 1.3) % 7.7) < 0.2
    depth = 0.004
    y[0, in_transit] -= depth

    def scatter(flat):
        return float(numpy.median(numpy.std(flat[1:], axis=1) / sigma[1:]))

    assert scatter(y / y.mean(axis=1, keepdims=True)) > 2.0
    one = spec.fit(y, 1)
    assert scatter(one[0]) > 1.2
    two = spec.fit(y, 2)
    assert 0.97 <= scatter(two[0]) <= 1.02
    kept = numpy.mean(two[0][0, ~in_transit]) - numpy.mean(two[0][0, in_transit])
    assert kept >= 0.9 * depth
    assert two[4][1] < two[4][0]
