"""SysRem on the device (tls_sysrem, survey.sysrem_batch and detrend=SysRem(...) of the survey calls): flat, trend, c, a and
the iteration counts bit-equal to the numpy restatement of sysrem_spec at every size around the lane count and the row chunk,
kind of row, with and without dy; the stop decision (early, never, and a second component that stops before the first did);
the same errors at the C ABI and in Python; a trend that goes non-positive; the detrended searches equal the searches of rows
detrended beforehand; contexts and devices."""
import warnings

import numpy
import pytest

from tls_amd import _lib, survey, synthetic
from test_power_batch_results import assert_results_equal
import sysrem_spec as spec

pytestmark = pytest.mark.gpu


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _rows(n_rows, n, rng):
    """Rows of the kinds test_biweight.py takes -- noisy with transits, a few levels (heavy ties), constant, ramps up and
    down, isolated spikes, magnitudes near 1e-300 and 1e300 --, all but the constant ones times two shared profiles with a
    coefficient of their own."""
    x = numpy.linspace(0.0, 1.0, n)
    shared = (x - 0.5, numpy.sin(2 * numpy.pi * 2.5 * x))
    out = []
    for i in range(n_rows):
        kind = i % 8
        if kind == 0:
            r = 1.0 + 3e-4 * rng.standard_normal(n)
            r[(numpy.arange(n) % 97) < 4] *= 0.995
        elif kind == 1:
            r = numpy.round(1.0 + 0.01 * rng.standard_normal(n), 2)
        elif kind == 2:
            out.append(numpy.full(n, 0.75))
            continue
        elif kind == 3:
            r = numpy.linspace(0.5, 2.0, n)
        elif kind == 4:
            r = numpy.linspace(2.0, 0.5, n)
        elif kind == 5:
            r = numpy.ones(n)
            r[::37] = 3.0
            r[5::53] = 0.25
        elif kind == 6:
            r = 1e-300 * (1.0 + rng.random(n))
        else:
            r = 1e300 * (1.0 + rng.random(n))
        out.append(r * (1.0 + rng.normal(0.0, 5e-3) * shared[0] + rng.normal(0.0, 5e-3) * shared[1]))
    return numpy.abs(numpy.array(out)) + 0.0


def _errors(y, rng):
    """Per-point errors of about each row's own scatter (1e-3 of the level for a constant row), unequal by up to four."""
    scatter = numpy.std(y / y.mean(axis=1, keepdims=True), axis=1) * y.mean(axis=1)
    scatter = numpy.where(scatter > 0.0, scatter, 1e-3 * y[:, 0])
    return scatter[:, None] * rng.uniform(0.5, 2.0, y.shape)


def _check(ctx, y, k, dy=None, max_iter=30, tol=1e-6):
    flat, trend, (c, a, iters) = ctx.sysrem(y, k, dy=dy, max_iter=max_iter, tol=tol, return_trend=True, return_components=True)
    want = spec.fit(y, k, dy=dy, max_iter=max_iter, tol=tol)
    what = (y.shape, k, dy is not None, max_iter, tol)
    assert spec.trend_ok(want[1]), what
    assert iters.tolist() == want[4].tolist(), what
    assert numpy.array_equal(_bits(a), _bits(want[3])), what
    assert numpy.array_equal(_bits(c), _bits(want[2])), what
    assert numpy.array_equal(_bits(trend), _bits(want[1])), what
    assert numpy.array_equal(_bits(flat), _bits(want[0])), what
    return want


SHAPES = [(1, 2), (1, 33), (2, 2), (2, 65), (255, 2), (255, 31), (256, 32), (256, 65), (257, 2), (257, 31), (257, 32),
          (257, 33), (257, 65), (700, 2), (700, 33), (700, 65)]


@pytest.mark.parametrize("n,n_rows", SHAPES)
def test_bit_equal_small(gpu, n, n_rows):
    rng = numpy.random.default_rng(1000 * n + n_rows)
    y = _rows(n_rows, n, rng)
    dy = _errors(y, rng)
    for k in (1, 3):
        if k <= n_rows - 1:
            _check(gpu, y, k)
            _check(gpu, y, k, dy=dy)
    # the constant rows carry no weight and come out as y / m
    flat, (c, a, iters) = gpu.sysrem(y, 1, return_components=True)
    for i in range(2, n_rows, 8):
        assert numpy.all(flat[i] == 1.0) and c[i, 0] == 0.0


def _ensemble(n_rows, n, seed, amplitude=3e-3):
    """White noise of 2e-4 to 6e-4 a row plus two shared systematics, a ramp and a sawtooth, with per-row coefficients."""
    rng = numpy.random.default_rng(seed)
    x = numpy.arange(n) / float(n)
    sigma = rng.uniform(2e-4, 6e-4, n_rows)
    y = 1.0 + sigma[:, None] * rng.standard_normal((n_rows, n))
    y += rng.normal(0.0, amplitude, n_rows)[:, None] * (x - 0.5)
    y += rng.normal(0.0, amplitude, n_rows)[:, None] * ((x * 15.0) % 1.0 - 0.5)
    return y, sigma


def test_stops_early_and_never(gpu):
    y, _ = _ensemble(40, 300, 5)
    want = _check(gpu, y, 1, max_iter=40, tol=1e-2)
    assert 1 < want[4][0] < 40                      # stopped by the tolerance
    want = _check(gpu, y, 1, max_iter=12, tol=0.0)
    assert want[4][0] == 12                         # tol = 0: every iteration runs
    want = _check(gpu, y, 2, max_iter=1)
    assert want[4].tolist() == [1, 1]


def test_second_component_stops_before_the_first_did(gpu):
    """Component 1 sets its flag after more iterations than component 2 needs: the second starts from a clear flag, and the
    launches behind each stop return at once."""
    y, sigma = _ensemble(40, 300, 6)
    want = _check(gpu, y, 2, max_iter=60, tol=1e-3)
    assert 1 < want[4][1] < want[4][0] < 60, want[4]
    want = _check(gpu, y, 3, dy=numpy.broadcast_to(sigma[:, None], y.shape).copy(), max_iter=60, tol=1e-3)
    assert want[4][0] < 60


def test_bit_equal_96_by_4320(gpu):
    y, sigma = _ensemble(96, 4320, 7)
    _check(gpu, y, 2, max_iter=25)
    _check(gpu, y, 2, dy=sigma[:, None] * numpy.random.default_rng(8).uniform(0.5, 2.0, y.shape), max_iter=10)


def test_bit_equal_2_by_19440(gpu):
    y, _ = _ensemble(2, 19440, 9)
    _check(gpu, y, 1, max_iter=10)
    _check(gpu, y, 1, dy=numpy.full(y.shape, 3e-4), max_iter=10)


def test_null_outputs_give_the_same_flat(gpu):
    y, sigma = _ensemble(33, 257, 10)
    lib, dp = _lib.load(), _lib._dp
    full = gpu.sysrem(y, 2, return_trend=True, return_components=True)
    assert numpy.array_equal(_bits(gpu.sysrem(y, 2)), _bits(full[0]))
    assert numpy.array_equal(_bits(gpu.sysrem(y, 2, return_trend=True)[1]), _bits(full[1]))
    assert numpy.array_equal(_bits(gpu.sysrem(y, 2, return_components=True)[1][1]), _bits(full[2][1]))
    flat = numpy.empty_like(y)
    iters = numpy.zeros(2, dtype=numpy.int64)
    assert lib.tls_sysrem(gpu._h, dp(y), None, 257, 33, 2, 50, 1e-6, dp(flat), None, None, None, _lib._ip(iters)) == 0
    assert numpy.array_equal(_bits(flat), _bits(full[0])) and iters.tolist() == full[2][2].tolist()
    assert numpy.array_equal(_bits(survey.sysrem_batch(y, 2, context=gpu)), _bits(full[0]))
    got = survey.sysrem_batch(y, 2, return_trend=True, return_components=True, context=gpu)
    assert numpy.array_equal(_bits(got[1]), _bits(full[1])) and numpy.array_equal(_bits(got[2][0]), _bits(full[2][0]))


def test_argument_errors(gpu):
    """TLS_E_ARG at the C ABI (the binding's own checks bypassed) and ValueError in Python, for the same arguments."""
    lib, dp = _lib.load(), _lib._dp
    y, _ = _ensemble(5, 40, 11)
    dy = numpy.full(y.shape, 3e-4)
    out = numpy.empty_like(y)

    def c_call(rows, err, n=40, n_rows=5, k=1, max_iter=10, tol=1e-6):
        return lib.tls_sysrem(gpu._h, dp(rows), None if err is None else dp(err), n, n_rows, k, max_iter, tol, dp(out),
                              None, None, None, None)

    assert c_call(y, None) == 0 and c_call(y, dy) == 0 and c_call(y, None, tol=0.0) == 0
    assert c_call(y, None, k=4) == 0 and c_call(y, None, max_iter=_lib.SYSREM_MAX_ITER) == 0
    for kw in (dict(n=0), dict(n_rows=1), dict(n_rows=0), dict(k=0), dict(k=5), dict(k=-1), dict(max_iter=0),
               dict(max_iter=_lib.SYSREM_MAX_ITER + 1), dict(tol=-1e-9), dict(tol=numpy.nan), dict(tol=numpy.inf)):
        assert c_call(y, None, **kw) == -1, kw
    wide = numpy.ones((12, 4))
    assert lib.tls_sysrem(gpu._h, dp(wide), None, 4, 12, 9, 10, 1e-6, dp(numpy.empty_like(wide)), None, None, None, None) == -1
    for kw in (dict(n_components=0), dict(n_components=5), dict(n_components=1.5), dict(n_components=True), dict(max_iter=0),
               dict(max_iter=_lib.SYSREM_MAX_ITER + 1), dict(tol=-1e-9), dict(tol=numpy.nan), dict(tol=numpy.inf),
               dict(tol="1e-6"), dict(dy=dy[:, :39]), dict(dy=dy[:4])):
        with pytest.raises(ValueError):
            gpu.sysrem(y, **kw)
        with pytest.raises(ValueError):
            survey.sysrem_batch(y, context=gpu, **{dict(dy="dy_batch").get(k, k): v for k, v in kw.items()})
    with pytest.raises(ValueError):
        gpu.sysrem(wide, 9)
    for rows in (y[0], y[:1], y[None], numpy.ones((3, 0))):
        with pytest.raises(ValueError, match="shape"):
            gpu.sysrem(rows)
    for bad in (numpy.nan, numpy.inf, -numpy.inf, 0.0, -1.0):
        z = y.copy()
        z[3, 7] = bad
        assert c_call(z, None) == -1 and c_call(z, dy) == -1 and c_call(y, z) == -1, bad
        with pytest.raises(ValueError, match="non-positive"):
            gpu.sysrem(z)
        with pytest.raises(ValueError, match="non-positive"):
            gpu.sysrem(y, dy=z)
    _check(gpu, y, 2, dy=dy)   # (the context still works)


# the weights differ by ten orders of magnitude: the fit overshoots, and the trend of row 2 starts below zero
OVERSHOOT_Y = numpy.array([[3.0, 2.4, 1.6, 1.4], [2.7, 0.4, 2.2, 2.4], [2.4, 1.1, 2.4, 0.8]])
OVERSHOOT_DY = numpy.array([[0.1, 0.1, 10.0, 0.1], [0.1, 1.0, 1.0, 0.001], [100.0, 0.1, 0.01, 0.001]])


def test_non_positive_trend_is_an_error(gpu):
    trend = spec.fit(OVERSHOOT_Y, 1, dy=OVERSHOOT_DY, max_iter=20)[1]
    assert not spec.trend_ok(trend) and trend[2, 0] < 0 and numpy.all(trend.ravel()[:8] > 0)
    lib, dp = _lib.load(), _lib._dp
    out = numpy.empty_like(OVERSHOOT_Y)
    assert lib.tls_sysrem(gpu._h, dp(OVERSHOOT_Y), dp(OVERSHOOT_DY), 4, 3, 1, 20, 1e-6, dp(out), None, None, None, None) == -1
    assert "row 2, point 0" in lib.tls_last_error(gpu._h).decode()
    with pytest.raises(RuntimeError, match="row 2, point 0"):
        gpu.sysrem(OVERSHOOT_Y, 1, dy=OVERSHOOT_DY, max_iter=20)
    _check(gpu, OVERSHOOT_Y, 1)                       # (the context still works, and the same rows pass without dy)
    y, _ = _ensemble(5, 40, 12)
    _check(gpu, y, 2)


# ---- the survey calls with detrend=SysRem(...)

def _k2_batch(n_curves, seed=0):
    t, f0, kw = synthetic.config("k2_90d", seed=seed)
    rng = numpy.random.default_rng(seed)
    x = (t - t[0]) / (t[-1] - t[0])
    raw = numpy.array([synthetic.config("k2_90d", seed=seed + s)[1] for s in range(n_curves)])
    raw *= 1.0 + rng.normal(0.0, 4e-3, n_curves)[:, None] * (x - 0.5) \
        + rng.normal(0.0, 4e-3, n_curves)[:, None] * ((x * 15.0) % 1.0 - 0.5)
    raw *= 1.0 + 0.002 * numpy.sin(t[None, :] / (2.0 + numpy.arange(n_curves))[:, None])
    return t, raw, kw


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


STEPS = [survey.SysRem(2), (survey.SysRem(1), survey.Biweight(0.5))]


def _beforehand(t, raw, detrend, ctx, dy=None):
    if isinstance(detrend, survey.SysRem):
        return survey.sysrem_batch(raw, detrend.n_components, dy_batch=dy, context=ctx)
    return survey.biweight_batch(t, survey.sysrem_batch(raw, detrend[0].n_components, dy_batch=dy, context=ctx), 0.5,
                                 context=ctx)


@pytest.mark.parametrize("detrend", STEPS, ids=["sysrem2", "sysrem1_biweight"])
def test_power_batch_and_search_batch_detrend(gpu, detrend):
    t, raw, kw = _k2_batch(4)
    flat = _beforehand(t, raw, detrend, gpu)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_batch(t, raw, detrend=detrend, statistics=True, with_arrays=True, context=gpu, **kw)
        want = survey.power_batch(t, flat, statistics=True, with_arrays=True, context=gpu, **kw)
        _same_summary(got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert survey.power_batch(t, raw, context=gpu, **kw)[0]["SDE"].tobytes() != got[0]["SDE"].tobytes()
        got = survey.search_batch(t, raw, detrend=detrend, context=gpu, **kw)
        want = survey.search_batch(t, flat, context=gpu, **kw)
        for a, b in zip(got, want):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert survey.search_batch(t, raw, context=gpu, **kw)[1].tobytes() != got[1].tobytes()


def test_dy_batch_weights_the_fit_and_passes_through(gpu):
    t, raw, kw = _k2_batch(4, seed=2)
    dy = 3e-4 * numpy.random.default_rng(3).uniform(0.5, 2.0, raw.shape)
    flat = survey.sysrem_batch(raw, 2, dy_batch=dy, context=gpu)
    assert flat.tobytes() != survey.sysrem_batch(raw, 2, context=gpu).tobytes()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.search_batch(t, raw, dy, detrend=survey.SysRem(2), context=gpu, **kw)
        want = survey.search_batch(t, flat, dy, context=gpu, **kw)
    for a, b in zip(got, want):
        assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()


@pytest.mark.parametrize("detrend", STEPS, ids=["sysrem2", "sysrem1_biweight"])
def test_power_results_detrend(gpu, detrend):
    t, raw, kw = _k2_batch(3, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_results(t, raw, detrend=detrend, context=gpu, **kw)
        want = survey.power_results(t, _beforehand(t, raw, detrend, gpu), context=gpu, **kw)
        plain = survey.power_results(t, raw[:1], context=gpu, **kw)
    for k in range(len(want)):
        assert_results_equal(got[k], want[k], "curve %d" % k)
    assert got[0].SDE != plain[0].SDE


def test_two_contexts_and_devices_same_bits(gpu):
    t, raw, kw = _k2_batch(40)
    one = survey.sysrem_batch(raw, 2, return_trend=True, return_components=True, context=gpu)
    other = _lib.Context(0)
    try:
        two = survey.sysrem_batch(raw, 2, return_trend=True, return_components=True, context=other)
    finally:
        other.close()
    for a, b in zip(one[:2] + one[2], two[:2] + two[2]):
        assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same_summary(survey.power_batch(t, raw, detrend=STEPS[1], devices=[0, 0], **kw)[0],
                      survey.power_batch(t, raw, detrend=STEPS[1], context=gpu, **kw)[0])
