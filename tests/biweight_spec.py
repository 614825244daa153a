"""The time-windowed biweight of tls_biweight_detrend (include/tls_amd.h) restated line by line in numpy, for the tests of
test_biweight_host.py and test_biweight.py: the windows by their definition, the location by its loop.  Every operation is
one IEEE double operation and both sums run in ascending order (numpy.cumsum accumulates sequentially), so the device's
result must equal this one bit for bit.  Slow by design: one numpy loop per point."""
import numpy

C = 5.0
FTOL = 1e-6
MAX_ITER = 50
MAX_WINDOW = 4095


def windows(t, window_length, break_tolerance):
    """(lo, hi): the window [lo[i], hi[i]) of every point -- the points j of i's segment (a new one starts at every j with
    t[j] - t[j-1] > break_tolerance) with abs(t[j] - t[i]) <= 0.5 * window_length -- grown outward from i by that test."""
    t = numpy.asarray(t, dtype=numpy.float64)
    n = len(t)
    half = 0.5 * window_length
    new = numpy.zeros(n, dtype=bool)
    new[1:] = (t[1:] - t[:-1]) > break_tolerance
    lo, hi = numpy.empty(n, dtype=numpy.int64), numpy.empty(n, dtype=numpy.int64)
    for i in range(n):
        a = i
        while a > 0 and not new[a] and abs(t[a - 1] - t[i]) <= half:
            a -= 1
        b = i + 1
        while b < n and not new[b] and abs(t[b] - t[i]) <= half:
            b += 1
        lo[i], hi[i] = a, b
    return lo, hi


def median(v):
    """numpy.median: the middle value, or (a + b) / 2 of the two middle values."""
    s = numpy.sort(v)
    m = len(s)
    return s[m // 2] if m % 2 else (s[m // 2 - 1] + s[m // 2]) / 2.0


def location(v):
    """The biweight location of one window's values v, in the header's steps."""
    v = numpy.asarray(v, dtype=numpy.float64)
    loc = median(v)
    for _ in range(MAX_ITER):
        d = v - loc
        mad = median(numpy.abs(d))
        if mad == 0:
            break
        s = C * mad
        u = d / s
        q = 1.0 - u * u
        w = numpy.where(numpy.abs(u) < 1.0, q * q, 0.0)
        new = numpy.cumsum(w * v)[-1] / numpy.cumsum(w)[-1]
        done = abs(new - loc) <= FTOL * abs(new)
        loc = new
        if done:
            break
    return loc


def detrend(t, y, window_length, break_tolerance):
    """(flat, trend) of y [n] or [n_rows, n] at the time stamps t."""
    y = numpy.asarray(y, dtype=numpy.float64)
    rows = y[None, :] if y.ndim == 1 else y
    lo, hi = windows(t, window_length, break_tolerance)
    assert (hi - lo).max() <= MAX_WINDOW
    trend = numpy.array([[location(r[a:b]) for a, b in zip(lo, hi)] for r in rows]).reshape(rows.shape)
    flat = rows / trend
    return (flat[0], trend[0]) if y.ndim == 1 else (flat, trend)
