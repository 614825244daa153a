"""Survey-mode statistics, the parts that need no GPU: the binding's record layout and the Python layer's checks."""
import ctypes

import numpy
import pytest

from tls_amd import _lib, search, survey, synthetic


def test_transit_stats_record_matches_its_dtype():
    assert ctypes.sizeof(_lib.TransitStats) == _lib.TRANSIT_STATS_DTYPE.itemsize == 16 * 8
    assert _lib.TRANSIT_STATS_DTYPE.names == tuple(k for k, _ in _lib.TransitStats._fields_)
    assert "tls_power_batch_stats" in _lib.SYMBOLS and "tls_debug_transit_stats" in _lib.SYMBOLS


def test_statistics_on_unsorted_time_stamps_fail_before_any_device_work(monkeypatch):
    def no_device(*args, **kwargs):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(search, "default_context", no_device)
    monkeypatch.setattr(search, "device_group", no_device)
    monkeypatch.setattr(_lib, "Context", no_device)
    t, f = synthetic.light_curve(20.0, 24, 2e-4, per=3.3, rp=0.05, a=10)
    t = t.copy()
    t[[10, 11]] = t[[11, 10]]
    with pytest.raises(ValueError, match="ascending"):
        survey.power_batch(t, numpy.stack([f, f]), statistics=True, period_min=1.0, period_max=6.0)
    with pytest.raises(ValueError, match="ascending"):
        survey.power_batch(t, numpy.stack([f, f]), per_transit=True, period_min=1.0, period_max=6.0)


def test_vectorised_fap_is_the_lookup_of_every_curve():
    from tls_amd.stats import FAP
    sde = numpy.array([0.0, 3.2, 7.0, 7.35, 9.0, 12.5, 25.7, 1e6, numpy.inf, numpy.nan, -1.0])
    got = survey._fap(sde)
    want = numpy.array([FAP(s) for s in sde])
    numpy.testing.assert_array_equal(got, want)


def test_count_roots_are_the_two_scalar_expressions_of_power():
    """stats.count_roots(n) against the expressions power() evaluates, element by element, for every count of a Kepler-sized
    series (k <= 70 129): root[k] is float(k) ** 0.5 (Python's pow) and root_count[k] is numpy.sum(k) ** 0.5 (the power of a
    numpy integer scalar, stats._mean_and_err's divisor).  The guard on the vectorised form of the second table: whichever
    counts the running numpy rounds differently, the table has them.  About 0.5 s."""
    from tls_amd.stats import count_roots
    n = 70129
    root, root_count = count_roots(n)
    assert root.dtype == root_count.dtype == numpy.float64 and root.shape == root_count.shape == (n + 1,)
    want_root = numpy.array([float(k) ** 0.5 for k in range(n + 1)])
    want_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(n + 1)])
    numpy.testing.assert_array_equal(root, want_root)
    numpy.testing.assert_array_equal(root_count, want_count)
    # a shorter table is the head of a longer one (the kernel indexes by the count alone)
    short = count_roots(1380)
    numpy.testing.assert_array_equal(short[0], root[:1381])
    numpy.testing.assert_array_equal(short[1], root_count[:1381])
    differ = numpy.flatnonzero(want_root != want_count)
    print("numpy %s: numpy.sum(k) ** 0.5 != float(k) ** 0.5 at %d of the counts 1 .. %d" % (numpy.__version__, len(differ), n))
    # (no expectation of that set: it belongs to the numpy build; the two are never more than one ulp apart)
    assert numpy.all(numpy.abs(want_root - want_count) <= numpy.spacing(want_root))
