"""The statistics of the main chain on a series whose out-of-transit flux is longer than numpy's reduction buffer.

numpy.add.reduce hands pairwise_sum a contiguous array 8192 elements at a time and adds the calls' sums from the left, so
numpy.std(flux_ootr) -- which the SNR divides by -- is one pairwise sum only up to 8192 points.  tls_transit_stats summed the
whole array in one pairwise pass and was one ulp off power()'s snr on some such series; it now sums in numpy's blocks
(tls_kernels.hip.h numpy_pairwise_sum).  The picks go through tls_debug_transit_stats, the kernel power_batch(
statistics=True) runs, against host_stats of tests/test_power_batch_statistics.py, every field and every per-transit row.

The noise seeds: on 1, 11 and 12 a single pairwise pass over the 10 182 out-of-transit points rounds their std, and with it
the snr, the other way than numpy's blocks do (worked out on the host, from numpy's pairwise_sum restated in Python, for
seeds 1 to 12); on seed 2 both agree."""
import numpy
import pytest

from tls_amd import _lib, transit_model
from test_power_batch_statistics import prepared, run_injected

pytestmark = pytest.mark.gpu


def test_out_of_transit_flux_longer_than_numpys_buffer():
    n = 10224
    t = numpy.linspace(3.0, 33.0, n)
    model = transit_model.light_curve(t, 3.4, 4.1, 0.06, 12, 89.8, 0, 90, [0.4, 0.3], "quadratic")
    curves = [model + numpy.random.RandomState(seed).normal(0, 4e-4, n) for seed in (1, 11, 12, 2)]
    ctx = _lib.Context(0)
    inp = prepared(ctx, t, curves[0], period_min=2.5, period_max=7.0, oversampling_factor=1)
    n_p = len(inp["periods"])
    power = numpy.exp(-0.5 * ((numpy.arange(n_p) - n_p / 2) / 40.0) ** 2)
    for y in [inp["y"]] + curves[1:]:
        stats, infos = run_injected(ctx, inp, y, [(4.1, 3.4, 3)], inp["table"].duration, [power])   # (period, T0, template row)
        assert infos[0]["n_ootr"] > 8192 and infos[0]["odd"] == 39 and stats["in_transit_count"][0] >= 39 + 40
        assert numpy.isfinite(stats["snr"][0])
    ctx.close()
