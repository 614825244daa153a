"""Null light curves on the device (tls_null_rows) and survey.null_sde: the device's Philox words against numpy.random.Philox,
the bootstrap rows bit for bit against a numpy mirror, the white-noise normals against numpy's restatement on the same
uniforms, rows that depend on the trial alone (chunking, first_trial splits, device groups), the C entry's argument checks,
and the end-to-end summary against power_batch on the same rows."""
import warnings

import numpy
import pytest

from tls_amd import survey, synthetic
from test_null_calibration_host import bootstrap_rows, trial_words, white_rows, white_z

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2 ** 64 - 1)


@pytest.mark.parametrize("seed", SEEDS, ids=str)
def test_device_words_are_numpy_philox(gpu, seed):
    for n in (37, 64, 1001):
        for block in (None, 1, 3, n):
            for first_trial in (0, 12345):
                got = gpu.debug_null_words(n, 5, seed, first_trial, block=block)
                for r in range(5):
                    _, W, want = trial_words(n, seed, first_trial + r, block)
                    assert got.shape == (5, W)
                    numpy.testing.assert_array_equal(got[r], want, err_msg="n=%d block=%s R=%d" % (n, block, first_trial + r))


@pytest.mark.parametrize("seed", SEEDS, ids=str)
def test_bootstrap_rows_bit_exact(gpu, seed):
    rng = numpy.random.RandomState(5)
    for n in (50, 4320):
        src = 1.0 + 1e-3 * rng.standard_normal((3, n))
        for L in (1, 7, 48, n - 1, n):   # (7 and 48 leave a short last block at n = 50; 48 divides 4320)
            for first_trial in (0, 12345):
                got = gpu.null_rows(n, 4, seed, first_trial, source=src, block=L)
                want = bootstrap_rows(n, 4, seed, first_trial, src, L)
                assert numpy.array_equal(got.view(numpy.uint64), want.view(numpy.uint64)), (n, L, first_trial)
    # one source row, given as [n]
    src = 1.0 + 1e-3 * rng.standard_normal(301)
    numpy.testing.assert_array_equal(gpu.null_rows(301, 6, seed, 9, source=src, block=20),
                                     bootstrap_rows(301, 6, seed, 9, src, 20))


@pytest.mark.parametrize("seed", SEEDS, ids=str)
def test_white_noise_normals(gpu, seed):
    """z = (out - 1) / sigma is exact up to the rounding of out (<= 2^-53 / sigma); the device's log and cos may differ from
    numpy's by an ulp or so, which moves z by far less than 1e-14."""
    for n in (4321, 4320):
        for first_trial in (0, 12345):
            sigma = numpy.array([0.1, 0.05, 0.025, 0.0125])
            got = gpu.null_rows(n, 4, seed, first_trial, sigma=sigma)
            want = white_rows(n, 4, seed, first_trial, sigma)
            for r in range(4):
                _, _, w = trial_words(n, seed, first_trial + r)
                z = white_z(w[:2 * n])
                z_dev = (got[r] - 1.0) / sigma[r]
                assert numpy.max(numpy.abs(z_dev - z)) <= 1e-14 + 2.0 ** -53 / sigma[r] * (1 + 1e-9)
                assert numpy.max(numpy.abs(got[r] - want[r])) <= 2.0 ** -51
    # one shared sigma
    numpy.testing.assert_allclose(gpu.null_rows(33, 3, seed, 2, sigma=0.01), white_rows(33, 3, seed, 2, 0.01), rtol=0,
                                  atol=2.0 ** -51)


def test_normal_moments(gpu):
    """10^6 normals of one fixed seed (deterministic): mean, variance, tails and the range Box-Muller can reach."""
    z = ((gpu.null_rows(1000, 1000, 20261015, 0, sigma=0.1) - 1.0) / 0.1).ravel()
    assert abs(numpy.mean(z)) < 0.005
    assert abs(numpy.var(z) - 1.0) < 0.01
    assert abs(numpy.mean(numpy.abs(z) > 1.959963984540054) - 0.05) < 0.002
    assert numpy.max(numpy.abs(z)) < 8.6


def _small_search():
    t = numpy.linspace(3.14, 27.14, 24 * 48)
    return t, dict(period_min=1.0, period_max=6.0, oversampling_factor=2)


def _same(a, b):
    """Two summaries (or row blocks) bit for bit, NaN fields included."""
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def test_rows_depend_on_the_trial_only(gpu):
    t, kw = _small_search()
    n = len(t)
    src = 1.0 + 5e-4 * numpy.random.RandomState(8).standard_normal((2, n))
    for mode in ({"sigma": numpy.linspace(0.001, 0.004, 40)}, {"source": src, "block": 12}):
        ref_summary, ref_rows = survey.null_sde(t, 40, seed=3, first_trial=100, return_rows=True, context=gpu, **mode, **kw)
        for chunk in (1, 7, 32, 1000):
            summary, rows = survey.null_sde(t, 40, seed=3, first_trial=100, chunk=chunk, return_rows=True, context=gpu,
                                            **mode, **kw)
            _same(rows, ref_rows)
            _same(summary, ref_summary)
        # split at trial 13: first_trial 100 .. 112, then 113 .. 139
        part = dict(mode)
        if "sigma" in part:
            part["sigma"] = mode["sigma"][:13]
        a = survey.null_sde(t, 13, seed=3, first_trial=100, return_rows=True, context=gpu, **part, **kw)
        if "sigma" in part:
            part["sigma"] = mode["sigma"][13:]
        b = survey.null_sde(t, 27, seed=3, first_trial=113, return_rows=True, context=gpu, **part, **kw)
        _same(numpy.concatenate([a[1], b[1]]), ref_rows)
        _same(numpy.concatenate([a[0], b[0]]), ref_summary)
        # a device group: rows formed on its first device, searched over both
        summary, rows = survey.null_sde(t, 40, seed=3, first_trial=100, chunk=16, return_rows=True, devices=[0, 0], **mode, **kw)
        _same(rows, ref_rows)
        _same(summary, ref_summary)
    # another seed, another first trial: other rows
    other = survey.null_sde(t, 2, sigma=0.002, seed=4, first_trial=100, return_rows=True, context=gpu, **kw)[1]
    assert not numpy.array_equal(other, survey.null_sde(t, 2, sigma=0.002, seed=3, first_trial=100, return_rows=True,
                                                        context=gpu, **kw)[1])


def test_argument_errors_of_the_c_entry(gpu):
    """The C entry's own checks (the binding bypasses null_sde's)."""
    src = numpy.ones((2, 40))
    bad = [dict(sigma=0.0), dict(sigma=0.2), dict(sigma=numpy.nan), dict(sigma=[0.01, 0.01]),
           dict(source=src, block=0), dict(source=src, block=41),
           dict(source=numpy.where(numpy.arange(40) == 3, 0.0, 1.0), block=4),
           dict(source=numpy.where(numpy.arange(40) == 3, numpy.inf, 1.0), block=4),
           dict(source=numpy.where(numpy.arange(40) == 3, numpy.nan, 1.0), block=4)]
    for kwargs in bad:
        with pytest.raises(RuntimeError, match="tls_amd error"):
            gpu.null_rows(40, 3, 0, 0, **kwargs)
    with pytest.raises(RuntimeError, match="first_trial"):
        gpu.null_rows(40, 3, 0, -1, sigma=0.01)
    with pytest.raises(RuntimeError, match="counter"):
        gpu.null_rows(40, 3, 0, 2 ** 62, sigma=0.01)
    with pytest.raises(RuntimeError, match="counter"):
        gpu.debug_null_words(40, 3, 0, 2 ** 62)
    assert gpu.null_rows(40, 0, 0, 0, sigma=0.01).shape == (0, 40)


@pytest.mark.parametrize("statistics", [False, True], ids=["summary", "statistics"])
def test_null_sde_equals_power_batch_on_its_rows(gpu, statistics):
    """70 k2_90d trials (three launch groups of 32) in both modes: the summary is power_batch's on the same rows, field by
    field, bit for bit."""
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    src = numpy.stack([f0, synthetic.config("k2_90d", seed=1)[1]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for mode in ({"sigma": 3e-4}, {"source": src, "block": 48}):
            summary, rows = survey.null_sde(t, 70, seed=11, return_rows=True, statistics=statistics, context=gpu, **mode, **kw)
            assert rows.shape == (70, len(t))
            want = survey.power_batch(t, rows, statistics=statistics, context=gpu, **kw)[0]
            assert summary.dtype == want.dtype
            for k in want.dtype.names:
                assert summary[k].tobytes() == want[k].tobytes(), k
            assert numpy.all(numpy.isfinite(summary["SDE"]))
            table = survey.fap_table(summary["SDE"], max_fap=0.5)
            assert table[2] == 70
