"""Context.device_bytes() counts every device buffer of the context (DESIGN.md "Device memory"): the eight row-stage entries
whose buffers the count once left out each raise it by at least their time stamps or one row, and a second fresh context
that runs the same call arrives at the same count.  The inputs are the smallest existing ones: the entry's first case in
tests/stage_memory_cases.py, or, for the three entries that have none there, the smallest input of the entry's own test."""
import numpy
import pytest

import multi_planet_cases
import stage_memory_cases as sm
from test_biweight import _rows, _times
from test_multi_planet import device as remove_transits
from tls_amd import _lib

pytestmark = pytest.mark.gpu


def _first_case(entry):
    case = next(c for c in sm.CASES.values() if c.entry == entry)
    return lambda ctx: sm.arrays(sm.quiet(case.run, ctx))[0]


def _transit_mask(ctx):
    """tests/test_transit_protect.py test_transit_mask_bit_equal at n = 257, its candidates that take part."""
    n = 257
    t = 3.0 + numpy.cumsum(numpy.random.default_rng(n).uniform(0.2, 1.8, n)) / 48.0
    span = t[-1] - t[0]
    period = numpy.array([span / 3.7, span / 5.1, span / 2.3])
    return ctx.transit_mask(t, period, t[0] + numpy.array([0.1, 0.3, 0.05]), numpy.array([0.11, 0.2, 0.07]), numpy.array([2, 0, 2]), 3, 1.5)


def _biweight_masked(ctx):
    """tests/test_transit_protect.py test_masked_biweight_bit_equal at n = 256, regular stamps, the typical window."""
    rng = numpy.random.default_rng(1000 + 256)
    t = _times(256, "regular", rng)
    rows = _rows(256, rng)[:2]
    masks = numpy.zeros(rows.shape, dtype=numpy.uint8)
    masks[1, 100:120] = 1
    return ctx.biweight_detrend_masked(t, rows, masks, 0.5, 0.5, 1)


def _remove_transits(ctx):
    """tests/test_multi_planet.py at its smallest layout."""
    return remove_transits(ctx, multi_planet_cases.layout(257, 64, 1))[0]


# entry -> a call on a context that returns rows [.., n]
CALLS = {
    "tls_inject_transits": _first_case("tls_inject_transits"),
    "tls_null_rows": _first_case("tls_null_rows"),
    "tls_medfilt_detrend": _first_case("tls_medfilt_detrend"),
    "tls_biweight_detrend": _first_case("tls_biweight_detrend"),
    "tls_transit_mask": _transit_mask,
    "tls_biweight_detrend_masked": _biweight_masked,
    "tls_remove_transits": _remove_transits,
    "tls_sysrem": _first_case("tls_sysrem"),
}


def _growth(call):
    ctx = _lib.Context(0)
    try:
        before = ctx.device_bytes()[0]
        n = numpy.asarray(call(ctx)).shape[-1]
        return n, before, ctx.device_bytes()[0]
    finally:
        ctx.close()


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_device_bytes_counts_the_stage(entry):
    n, before, after = _growth(CALLS[entry])
    print(entry, "n =", n, "bytes before", before, "after", after)
    assert after - before >= 8 * n, (entry, n, before, after)
    assert _growth(CALLS[entry]) == (n, before, after), entry    # the first context closed, a second fresh one: the same count
