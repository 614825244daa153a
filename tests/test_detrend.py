"""Median-filter detrending on the device (tls_medfilt_detrend, survey.detrend_batch and detrend= of the survey calls): flat
and trend bit-equal to y / scipy.signal.medfilt(y, k) and medfilt(y, k) at every size, kernel and kind of row; the same
errors at the C ABI and in Python; the detrended searches equal the searches of rows detrended beforehand; the K2-3
known-answer pins; injection-recovery and null calibration through the filter."""
import os
import warnings

import numpy
import pytest
from scipy.signal import medfilt

from tls_amd import _lib, survey, synthetic
from conftest import GOLDEN
from test_power_batch_results import assert_results_equal

pytestmark = pytest.mark.gpu

KERNELS = (1, 3, 5, 25, 101, 361, 721)


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def _rows(n, rng):
    """The kinds of rows the filter must take: noisy transits times a slow trend, a few levels (heavy ties), constant,
    ramps up and down, isolated spikes, magnitudes near 1e-300 and 1e300."""
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


def _check(ctx, rows, k):
    flat, trend = ctx.medfilt_detrend(rows, k, return_trend=True)
    want = numpy.array([medfilt(r, k) for r in rows])
    assert numpy.array_equal(_bits(trend), _bits(want)), (rows.shape, k)
    assert numpy.array_equal(_bits(flat), _bits(rows / want)), (rows.shape, k)
    assert numpy.array_equal(_bits(ctx.medfilt_detrend(rows, k)), _bits(flat))   # (without the trend: the same flat)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 256, 4320, 19440])
def test_bit_equal_to_scipy(gpu, n):
    rng = numpy.random.default_rng(n)
    rows = _rows(n, rng)
    ks = [k for k in KERNELS if k <= n]
    if n % 2 == 1:
        ks.append(n)                                    # k = n
    if n >= _lib.MEDFILT_MAX_KERNEL:
        ks.append(_lib.MEDFILT_MAX_KERNEL)              # the cap
    for k in sorted(set(ks)):
        _check(gpu, rows, k)
    # one row as [n]
    flat = gpu.medfilt_detrend(rows[0], ks[-1])
    assert flat.shape == (n,) and numpy.array_equal(_bits(flat), _bits(rows[0] / medfilt(rows[0], ks[-1])))


def test_long_rows(gpu):
    rng = numpy.random.default_rng(70128)
    rows = _rows(70128, rng)[[0, 1, 5, 7]]
    for k in (25, 361, _lib.MEDFILT_MAX_KERNEL):
        _check(gpu, rows, k)


def test_k_one_is_the_identity(gpu):
    y = 1.0 + 1e-3 * numpy.random.default_rng(1).standard_normal((3, 500))
    flat, trend = gpu.medfilt_detrend(y, 1, return_trend=True)
    assert numpy.array_equal(_bits(trend), _bits(y)) and numpy.all(flat == 1.0)


@pytest.mark.parametrize("n_rows", [1, 33])
def test_row_counts(gpu, n_rows):
    rng = numpy.random.default_rng(n_rows)
    t, f0, _ = synthetic.config("k2_90d", seed=0)
    rows = numpy.array([f0 * (1.0 + 0.01 * numpy.sin(t / (3.0 + r))) + 1e-4 * rng.standard_normal(len(t))
                        for r in range(n_rows)])
    for k in (25, 361):
        _check(gpu, rows, k)


def test_more_than_one_slab(gpu):
    """256-point rows: 65535 rows per launch (gridDim.y), so 65537 rows take two slabs, the second of two rows."""
    rng = numpy.random.default_rng(5)
    rows = numpy.round(1.0 + 0.01 * rng.standard_normal((65537, 256)), 3)
    flat, trend = gpu.medfilt_detrend(rows, 25, return_trend=True)
    want = numpy.array([medfilt(r, 25) for r in rows])
    assert numpy.array_equal(_bits(trend), _bits(want)) and numpy.array_equal(_bits(flat), _bits(rows / want))
    assert gpu.medfilt_detrend(numpy.ones((0, 256)), 25).shape == (0, 256)


def test_argument_errors(gpu):
    """TLS_E_ARG at the C ABI (the binding's own checks bypassed) and ValueError in Python, for the same arguments."""
    lib = _lib.load()
    y = numpy.ones((2, 40))
    out = numpy.empty_like(y)
    dp = _lib._dp

    def c_call(rows, n, n_rows, k):
        return lib.tls_medfilt_detrend(gpu._h, dp(rows), n, n_rows, k, dp(out), None)

    for k in (0, -1, 2, 40, 41, 43):
        assert c_call(y, 40, 2, k) == -1, k
        with pytest.raises(ValueError):
            gpu.medfilt_detrend(y, k)
        with pytest.raises(ValueError):
            survey.detrend_batch(y, k, context=gpu)
    for k in (2.0, 3.0, True, "3"):
        with pytest.raises(ValueError):
            gpu.medfilt_detrend(y, k)
    big = numpy.ones((1, _lib.MEDFILT_MAX_KERNEL + 2))
    big_out = numpy.empty_like(big)
    assert lib.tls_medfilt_detrend(gpu._h, dp(big), big.shape[1], 1, _lib.MEDFILT_MAX_KERNEL + 2, dp(big_out), None) == -1
    with pytest.raises(ValueError, match="MEDFILT_MAX_KERNEL"):
        gpu.medfilt_detrend(big, _lib.MEDFILT_MAX_KERNEL + 2)
    for bad in (numpy.nan, numpy.inf, 0.0, -1.0):
        z = y.copy()
        z[1, 7] = bad
        assert c_call(z, 40, 2, 3) == -1, bad
        with pytest.raises(ValueError):
            gpu.medfilt_detrend(z, 3)
    assert c_call(y, 0, 2, 1) == -1 and c_call(y, 40, -1, 3) == -1
    assert c_call(y, 40, 0, 3) == 0                        # n_rows == 0: a no-op
    _check(gpu, 1.0 + numpy.arange(80.0).reshape(2, 40), 3)   # (the context still works)


# ---- the survey calls with detrend=

def _k2_batch(n_curves, seed=0):
    t, f0, kw = synthetic.config("k2_90d", seed=seed)
    rng = numpy.random.default_rng(seed)
    raw = numpy.array([synthetic.config("k2_90d", seed=seed + s)[1] * (1.0 + 0.005 * numpy.sin(t / (2.0 + s) + s))
                       for s in range(n_curves)])
    raw *= 1.0 + 1e-5 * rng.standard_normal(raw.shape)
    return t, raw, kw


def _filtered(raw, k):
    return raw / numpy.array([medfilt(r, k) for r in raw])


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_power_batch_and_search_batch_detrend(gpu):
    t, raw, kw = _k2_batch(5)
    flat = _filtered(raw, 25)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_batch(t, raw, detrend=25, statistics=True, with_arrays=True, context=gpu, **kw)
        want = survey.power_batch(t, flat, statistics=True, with_arrays=True, context=gpu, **kw)
        _same_summary(got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        # the raw rows searched as they are give another answer
        assert survey.power_batch(t, raw, context=gpu, **kw)[0]["SDE"].tobytes() != got[0]["SDE"].tobytes()
        got = survey.search_batch(t, raw, detrend=25, context=gpu, **kw)
        want = survey.search_batch(t, flat, context=gpu, **kw)
        for a, b in zip(got, want):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()


def test_power_results_detrend(gpu):
    t, raw, kw = _k2_batch(2, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_results(t, raw, detrend=25, context=gpu, **kw)
        want = survey.power_results(t, _filtered(raw, 25), context=gpu, **kw)
    for k in range(len(want)):
        assert_results_equal(got[k], want[k], "curve %d" % k)


def test_k2_known_answer(gpu):
    """The reference's test_multi_planet.py first pass on K2-3 (EPIC 201367065), y / medfilt(y, 25) formed on the device."""
    d = numpy.load(os.path.join(GOLDEN, "k2_EPIC201367065.npz"))
    t, y = d["t"], d["y"]
    results = survey.power_results(t, y[None], detrend=25, context=gpu)[0]
    aae = numpy.testing.assert_almost_equal
    aae(max(results.power), 45.49085809486116, decimal=3)
    aae(max(results.power_raw), 42.93056655774114, decimal=3)
    aae(min(results.power), -0.6175100139942546, decimal=3)
    aae(min(results.power_raw), -0.3043720539933344, decimal=3)


def test_injection_recovery_detrend(gpu):
    t, raw, kw = _k2_batch(1)
    base = raw[0]
    inj = survey.injection_grid(t, [3.0, 7.0], [0.03, 0.08], per_cell=9, b_max=0.5, seed=2)   # 36: two chunks of 32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec, summary, rows = survey.injection_recovery(t, base, inj, detrend=25, chunk=32, return_rows=True, context=gpu,
                                                       **kw)
        injected, count = gpu.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(None, None,
                                                                                                                kw)[1:])
        assert numpy.array_equal(_bits(rows), _bits(_filtered(injected, 25)))
        assert numpy.array_equal(rec["n_in_transit"], count)
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **kw)[0])
        plain = survey.injection_recovery(t, base, inj, chunk=32, return_rows=True, context=gpu, **kw)
        assert numpy.array_equal(_bits(plain[2]), _bits(injected))


@pytest.mark.parametrize("mode", ["white", "bootstrap"])
def test_null_sde_detrend(gpu, mode):
    t, raw, kw = _k2_batch(2, seed=4)
    how = dict(sigma=3e-4) if mode == "white" else dict(source=raw, block=48)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        summary, rows = survey.null_sde(t, 36, seed=9, detrend=101, return_rows=True, chunk=32, context=gpu, **how, **kw)
        plain = survey.null_sde(t, 36, seed=9, return_rows=True, chunk=32, context=gpu, **how, **kw)[1]
        assert numpy.array_equal(_bits(rows), _bits(_filtered(plain, 101)))
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **kw)[0])
        first = survey.null_sde(t, 20, seed=9, detrend=101, return_rows=True, context=gpu, **how, **kw)[1]
        rest = survey.null_sde(t, 16, seed=9, first_trial=20, detrend=101, return_rows=True, context=gpu, **how, **kw)[1]
        assert numpy.array_equal(_bits(numpy.concatenate([first, rest])), _bits(rows))


def test_two_contexts_same_bits(gpu):
    t, raw, kw = _k2_batch(70)
    one = survey.detrend_batch(raw, 25, return_trend=True, context=gpu)
    two = survey.detrend_batch(raw, 25, return_trend=True, devices=[0, 0])
    for a, b in zip(one, two):
        assert numpy.array_equal(_bits(a), _bits(b))
    assert numpy.array_equal(_bits(one[1]), _bits(numpy.array([medfilt(r, 25) for r in raw])))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same_summary(survey.power_batch(t, raw[:40], detrend=25, devices=[0, 0], **kw)[0],
                      survey.power_batch(t, raw[:40], detrend=25, context=gpu, **kw)[0])
