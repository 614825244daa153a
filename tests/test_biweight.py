"""Biweight detrending on the device (tls_biweight_detrend, survey.biweight_batch and detrend=Biweight(...) of the survey
calls): flat and trend bit-equal to the numpy restatement of biweight_spec at every size, kind of row, kind of time stamps and
window; the same errors at the C ABI and in Python; the detrended searches equal the searches of rows detrended beforehand;
K2-3 through the biweight; contexts and devices."""
import os
import warnings

import numpy
import pytest

from tls_amd import _lib, survey, synthetic
from conftest import GOLDEN
from test_power_batch_results import assert_results_equal
import biweight_spec as spec

pytestmark = pytest.mark.gpu

CADENCE = 1.0 / 64.0   # (exact in binary: gaps of exactly break_tolerance can be built)


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _rows(n, rng):
    """The kinds of rows test_detrend.py takes: noisy transits times a slow trend, a few levels (heavy ties), constant, ramps
    up and down, isolated spikes, magnitudes near 1e-300 and 1e300."""
    x = numpy.linspace(0.0, 1.0, n)
    noisy = (1.0 + 0.02 * numpy.sin(2 * numpy.pi * 3 * x)) * (1.0 + 3e-4 * rng.standard_normal(n))
    noisy[(numpy.arange(n) % 97) < 4] *= 0.995
    spikes = numpy.ones(n)
    spikes[::37] = 3.0
    spikes[5::53] = 0.25
    out = [noisy, numpy.round(1.0 + 0.01 * rng.standard_normal(n), 2), numpy.full(n, 0.75),
           numpy.linspace(0.5, 2.0, n), numpy.linspace(2.0, 0.5, n), spikes,
           1e-300 * (1.0 + rng.random(n)), 1e300 * (1.0 + rng.random(n))]
    return numpy.array([numpy.abs(r) + 0.0 for r in out])


def _times(n, kind, rng, cadence=CADENCE, tolerance=0.5):
    """Time stamps: regular, irregular, with repeated stamps, or with gaps of exactly `tolerance` (no split) and of one
    cadence more (a split)."""
    t = 1000.0 + cadence * numpy.arange(n)
    if kind == "irregular":
        t = 1000.0 + numpy.cumsum(cadence * rng.uniform(0.05, 2.5, n))
    elif kind == "duplicates":
        t[3::5] = t[2::5][:len(t[3::5])]
        t[4::11] = t[3::11][:len(t[4::11])]
    elif kind == "gaps":
        t[n // 3:] += tolerance - cadence               # a step of exactly `tolerance`: the same segment
        t[2 * n // 3:] += tolerance                     # a step of tolerance + cadence: a new segment
        t[5 * n // 6:] += 3.0                           # a wide gap
    assert numpy.all(t[1:] >= t[:-1])
    return t


def _check(ctx, t, rows, window_length, break_tolerance=0.5):
    flat, trend = ctx.biweight_detrend(t, rows, window_length, break_tolerance, return_trend=True)
    want_flat, want_trend = spec.detrend(t, rows, window_length, break_tolerance)
    assert numpy.array_equal(_bits(trend), _bits(want_trend)), (rows.shape, window_length, break_tolerance)
    assert numpy.array_equal(_bits(flat), _bits(want_flat)), (rows.shape, window_length, break_tolerance)
    assert numpy.array_equal(_bits(ctx.biweight_detrend(t, rows, window_length, break_tolerance)), _bits(flat))
    assert numpy.all(trend > 0) and numpy.all(numpy.isfinite(trend))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 256])
@pytest.mark.parametrize("kind", ["regular", "irregular", "duplicates", "gaps"])
def test_bit_equal_small(gpu, n, kind):
    rng = numpy.random.default_rng(n)
    rows = _rows(n, rng)
    t = _times(n, kind, rng)
    span = t[-1] - t[0]
    for wl in (0.3 * CADENCE, 0.5, 4.0 * span + 1.0):     # below one cadence, typical, longer than the series
        _check(gpu, t, rows, wl)
    _check(gpu, t, rows, 0.5, numpy.inf)                   # never split
    flat = gpu.biweight_detrend(t, rows[0], 0.5, 0.5)      # one row as [n]
    assert flat.shape == (n,) and numpy.array_equal(_bits(flat), _bits(spec.detrend(t, rows[0], 0.5, 0.5)[0]))


@pytest.mark.parametrize("kind", ["regular", "irregular", "duplicates", "gaps"])
def test_bit_equal_4320(gpu, kind):
    rng = numpy.random.default_rng(4320)
    rows = _rows(4320, rng)[[0, 1, 5, 7]]
    t = _times(4320, kind, rng)
    _check(gpu, t, rows, 0.5)
    _check(gpu, t, rows[[0]], 2.0, 0.25)


def test_bit_equal_tess_cadence(gpu):
    """19440 points at 2-min cadence (tess_27d): 361-point windows at 0.5 d, with a gap in the middle."""
    rng = numpy.random.default_rng(19440)
    rows = _rows(19440, rng)[[0, 6]]
    t = _times(19440, "gaps", rng, cadence=1.0 / 720.0)
    _check(gpu, t, rows, 0.5)


def test_window_at_the_cap(gpu):
    """Windows of exactly BIWEIGHT_MAX_WINDOW points (the largest span and LDS), and one point more is an error."""
    rng = numpy.random.default_rng(4095)
    rows = _rows(4320, rng)[[0]]
    t = _times(4320, "regular", rng)
    wl = (_lib.BIWEIGHT_MAX_WINDOW - 1) * CADENCE
    lo, hi = spec.windows(t, wl, 0.5)
    assert (hi - lo).max() == _lib.BIWEIGHT_MAX_WINDOW
    _check(gpu, t, rows, wl)
    with pytest.raises(ValueError, match="BIWEIGHT_MAX_WINDOW"):
        gpu.biweight_detrend(t, rows, wl + 2 * CADENCE, 0.5)


@pytest.mark.parametrize("n_rows", [1, 31, 32, 33])
def test_row_counts(gpu, n_rows):
    rng = numpy.random.default_rng(n_rows)
    t = _times(700, "irregular", rng)
    rows = (1.0 + 0.01 * numpy.sin(t[None, :] / rng.uniform(0.5, 3.0, (n_rows, 1)))) \
        * (1.0 + 1e-4 * rng.standard_normal((n_rows, 700)))
    _check(gpu, t, rows, 0.5)   # (about 32 points a window: 700 points are several tiles)


def test_argument_errors(gpu):
    """TLS_E_ARG at the C ABI (the binding's own checks bypassed) and ValueError in Python, for the same arguments."""
    lib = _lib.load()
    t = 1000.0 + CADENCE * numpy.arange(40)
    y = numpy.ones((2, 40))
    out = numpy.empty_like(y)
    dp = _lib._dp

    def c_call(tt, rows, n, n_rows, wl, bt):
        return lib.tls_biweight_detrend(gpu._h, dp(tt), dp(rows), n, n_rows, wl, bt, dp(out), None)

    for wl, bt in ((0.0, 0.5), (-1.0, 0.5), (numpy.inf, 0.5), (numpy.nan, 0.5), (0.5, 0.0), (0.5, -1.0), (0.5, numpy.nan)):
        assert c_call(t, y, 40, 2, wl, bt) == -1, (wl, bt)
        with pytest.raises(ValueError):
            gpu.biweight_detrend(t, y, wl, bt)
        with pytest.raises(ValueError):
            survey.biweight_batch(t, y, wl, bt, context=gpu)
    for bad_t in (t[::-1].copy(), numpy.where(numpy.arange(40) == 9, numpy.nan, t),
                  numpy.where(numpy.arange(40) == 39, numpy.inf, t)):
        assert c_call(bad_t, y, 40, 2, 0.5, 0.5) == -1
        with pytest.raises(ValueError):
            gpu.biweight_detrend(bad_t, y, 0.5, 0.5)
    long_t = CADENCE * numpy.arange(_lib.BIWEIGHT_MAX_WINDOW + 1)
    long_y = numpy.ones((1, len(long_t)))
    long_out = numpy.empty_like(long_y)
    assert lib.tls_biweight_detrend(gpu._h, dp(long_t), dp(long_y), len(long_t), 1, 1e6, 0.5, dp(long_out), None) == -1
    with pytest.raises(ValueError, match="BIWEIGHT_MAX_WINDOW"):
        gpu.biweight_detrend(long_t, long_y, 1e6, 0.5)
    for bad in (numpy.nan, numpy.inf, 0.0, -1.0):
        z = y.copy()
        z[1, 7] = bad
        assert c_call(t, z, 40, 2, 0.5, 0.5) == -1, bad
        with pytest.raises(ValueError):
            gpu.biweight_detrend(t, z, 0.5, 0.5)
    assert c_call(t, y, 0, 2, 0.5, 0.5) == -1 and c_call(t, y, 40, -1, 0.5, 0.5) == -1
    assert c_call(t, y, 40, 0, 0.5, 0.5) == 0                    # n_rows == 0: a no-op
    assert c_call(t, y, 40, 2, 0.5, numpy.inf) == 0              # inf: never split
    with pytest.raises(ValueError, match="shape"):
        gpu.biweight_detrend(t[:39], y, 0.5, 0.5)
    _check(gpu, t, 1.0 + numpy.arange(80.0).reshape(2, 40), 0.1)   # (the context still works)


# ---- the survey calls with detrend=Biweight(...)

def _k2_batch(n_curves, seed=0):
    t, f0, kw = synthetic.config("k2_90d", seed=seed)
    rng = numpy.random.default_rng(seed)
    raw = numpy.array([synthetic.config("k2_90d", seed=seed + s)[1] * (1.0 + 0.005 * numpy.sin(t / (2.0 + s) + s))
                       for s in range(n_curves)])
    raw *= 1.0 + 1e-5 * rng.standard_normal(raw.shape)
    return t, raw, kw


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


BW = survey.Biweight(0.5)


def test_power_batch_and_search_batch_detrend(gpu):
    t, raw, kw = _k2_batch(5)
    flat = survey.biweight_batch(t, raw, 0.5, context=gpu)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_batch(t, raw, detrend=BW, statistics=True, with_arrays=True, context=gpu, **kw)
        want = survey.power_batch(t, flat, statistics=True, with_arrays=True, context=gpu, **kw)
        _same_summary(got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert survey.power_batch(t, raw, context=gpu, **kw)[0]["SDE"].tobytes() != got[0]["SDE"].tobytes()
        got = survey.search_batch(t, raw, detrend=BW, context=gpu, **kw)
        want = survey.search_batch(t, flat, context=gpu, **kw)
        for a, b in zip(got, want):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()


def test_power_results_detrend(gpu):
    t, raw, kw = _k2_batch(2, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_results(t, raw, detrend=BW, context=gpu, **kw)
        want = survey.power_results(t, survey.biweight_batch(t, raw, 0.5, context=gpu), context=gpu, **kw)
    for k in range(len(want)):
        assert_results_equal(got[k], want[k], "curve %d" % k)


def test_injection_recovery_detrend(gpu):
    t, raw, kw = _k2_batch(1)
    base = raw[0]
    inj = survey.injection_grid(t, [3.0, 7.0], [0.03, 0.08], per_cell=9, b_max=0.5, seed=2)   # 36: two chunks of 32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec, summary, rows = survey.injection_recovery(t, base, inj, detrend=BW, chunk=32, return_rows=True, context=gpu,
                                                       **kw)
        injected, count = gpu.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(None, None,
                                                                                                                kw)[1:])
        assert numpy.array_equal(_bits(rows), _bits(survey.biweight_batch(t, injected, 0.5, context=gpu)))
        assert numpy.array_equal(rec["n_in_transit"], count)
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **kw)[0])


@pytest.mark.parametrize("mode", ["white", "bootstrap"])
def test_null_sde_detrend(gpu, mode):
    t, raw, kw = _k2_batch(2, seed=4)
    how = dict(sigma=3e-4) if mode == "white" else dict(source=raw, block=48)
    bw = survey.Biweight(1.0, 0.25)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        summary, rows = survey.null_sde(t, 36, seed=9, detrend=bw, return_rows=True, chunk=32, context=gpu, **how, **kw)
        plain = survey.null_sde(t, 36, seed=9, return_rows=True, chunk=32, context=gpu, **how, **kw)[1]
        assert numpy.array_equal(_bits(rows), _bits(survey.biweight_batch(t, plain, 1.0, 0.25, context=gpu)))
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **kw)[0])


def test_k2_known_answer(gpu):
    """K2-3 (EPIC 201367065, a 2.88 d gap): the biweight at 0.5 d finds the period the median filter (k = 25) finds, and the
    trend next to the gap is the restatement's, which never looks across it."""
    d = numpy.load(os.path.join(GOLDEN, "k2_EPIC201367065.npz"))
    t, y = d["t"], d["y"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        med = survey.power_results(t, y[None], detrend=25, context=gpu)[0]
        bw = survey.power_results(t, y[None], detrend=BW, context=gpu)[0]
    assert abs(bw.period - med.period) <= 1e-3 * med.period, (bw.period, med.period)
    assert bw.SDE > 9, bw.SDE
    gap = int(numpy.argmax(numpy.diff(t)))
    assert t[gap + 1] - t[gap] > 2.5
    assert gap >= 40 and gap + 41 < len(t)
    near = slice(gap - 40, gap + 41)
    flat, trend = survey.biweight_batch(t[near], y[near], 0.5, return_trend=True, context=gpu)
    want_flat, want_trend = spec.detrend(t[near], y[near], 0.5, 0.5)
    assert numpy.array_equal(_bits(trend), _bits(want_trend)) and numpy.array_equal(_bits(flat), _bits(want_flat))
    # the whole row: the points within 20 of the gap (windows of about +-12 points, ending at the gap) as the excerpt's
    whole = survey.biweight_batch(t, y, 0.5, return_trend=True, context=gpu)[1]
    inner = slice(gap - 20 - near.start, gap + 21 - near.start)
    assert numpy.array_equal(_bits(whole[gap - 20: gap + 21]), _bits(want_trend[inner]))


def test_two_contexts_and_devices_same_bits(gpu):
    t, raw, kw = _k2_batch(70)
    one = survey.biweight_batch(t, raw, 0.5, return_trend=True, context=gpu)
    other = _lib.Context(0)
    try:
        two = survey.biweight_batch(t, raw, 0.5, return_trend=True, context=other)
    finally:
        other.close()
    dealt = survey.biweight_batch(t, raw, 0.5, return_trend=True, devices=[0, 0])
    for a, b, c in zip(one, two, dealt):
        assert numpy.array_equal(_bits(a), _bits(b)) and numpy.array_equal(_bits(a), _bits(c))
    assert numpy.array_equal(_bits(one[1][:2]), _bits(spec.detrend(t, raw[:2], 0.5, 0.5)[1]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same_summary(survey.power_batch(t, raw[:40], detrend=BW, devices=[0, 0], **kw)[0],
                      survey.power_batch(t, raw[:40], detrend=BW, context=gpu, **kw)[0])
