"""The per-star noise profile of survey.noise_profile / tls_noise_profile -- a robust CDPP at a list of window widths --
restated in Python: the definition the kernels are tested against (include/tls_amd.h, DESIGN.md "Noise profile" and the
docstrings state the same lines).  It shares no code with the library.  Every step is one IEEE double operation.

    K = 1.4826022185056018
    median(v [m]): the value of rank m // 2 of the sorted values for odd m, 0.5 * (s[m/2 - 1] + s[m/2]) for even m
    curve y [n] (a -0.0 is taken as +0.0), optional t [n]:
        m = median(y);  d_j = y_j - m;  sigma = K * median(|d_j|)
        sigma == 0: status 1, n_clipped 0, n_pairs 0, sigma_p2p NaN, every per-width value NaN, every count 0
        keep_j = (d_j <= clip_upper * sigma) and (d_j >= -(clip_lower * sigma));  n_clipped = the others   (one pass)
        pairs: the j with keep_j, keep_{j+1} and t_{j+1} - t_j <= span_max[1];  n_pairs their number
        sigma_p2p = (K * median(|y_{j+1} - y_j| over the pairs)) / 1.4142135623730951;  NaN without a pair
    width w, windows i = 0 .. n - w over the samples [i, i + w):
        valid_i = every sample kept and t[i + w - 1] - t[i] <= span_max[w]
        v_i = (((0.0 + d_i) + d_{i+1}) + ... + d_{i+w-1}) / w
        count = the valid windows;  count < min_count: robust and rms NaN
        mu = median(valid v);  robust = K * median(|v_i - mu| over the valid)
        mean = lanes_sum(v, valid) / count;  rms = sqrt(lanes_sum((v_i - mean) * (v_i - mean), valid) / count)
    lanes_sum is the ordered 256-lane sum of tests/gls_spec.py.  Without t every span_max is inf.
    span_max[w] = (w - 1 + gap_tolerance) * cadence and span_max[1] = (1 + gap_tolerance) * cadence (the adjacency limit of
    the pairs, whether or not 1 is a width), cadence = numpy.median(numpy.diff(t)): formed on the host, by span_limits."""
import numpy

from gls_spec import lanes_sum

K = numpy.float64(1.4826022185056018)
ROOT2 = numpy.float64(1.4142135623730951)
CURVE_FIELDS = ("status", "n_clipped", "n_pairs", "median", "sigma", "sigma_p2p")


def median(values):
    s = numpy.sort(numpy.asarray(values, dtype=numpy.float64))
    m = len(s)
    if m % 2:
        return s[m // 2]
    return numpy.float64(0.5) * (s[m // 2 - 1] + s[m // 2])


def span_limits(t, widths, gap_tolerance=0.5):
    """(span_max [W], pair_span): the limits the host hands over; inf without t."""
    widths = numpy.asarray(widths, dtype=numpy.int64)
    if t is None:
        return numpy.full(len(widths), numpy.inf), numpy.float64(numpy.inf)
    cadence = numpy.median(numpy.diff(numpy.asarray(t, dtype=numpy.float64)))
    g = numpy.float64(gap_tolerance)
    return numpy.array([(numpy.float64(w - 1) + g) * cadence for w in widths], dtype=numpy.float64), (numpy.float64(1.0) + g) * cadence


def curve_part(y, t, pair_span, clip_upper, clip_lower):
    """(record dict, d [n], keep [n]) of one curve."""
    y = numpy.asarray(y, dtype=numpy.float64) + 0.0
    n = len(y)
    m = median(y)
    d = y - m
    sigma = K * median(numpy.fabs(d))
    nan = numpy.float64(numpy.nan)
    if sigma == 0.0:
        return dict(status=1.0, n_clipped=0.0, n_pairs=0.0, median=m, sigma=sigma, sigma_p2p=nan), d, numpy.zeros(n, dtype=bool)
    with numpy.errstate(all="ignore"):
        up = numpy.float64(clip_upper) * sigma
        low = -(numpy.float64(clip_lower) * sigma)
    keep = (d <= up) & (d >= low)
    pair = keep[:-1] & keep[1:]
    if t is not None:
        t = numpy.asarray(t, dtype=numpy.float64)
        pair &= (t[1:] - t[:-1]) <= pair_span
    n_pairs = int(pair.sum())
    p2p = nan
    if n_pairs:
        p2p = (K * median(numpy.fabs(y[1:] - y[:-1])[pair])) / ROOT2
    return dict(status=0.0, n_clipped=float(n - int(keep.sum())), n_pairs=float(n_pairs), median=m, sigma=sigma, sigma_p2p=p2p), d, keep


def window_means(d, w):
    """v [n - w + 1]: the direct left-to-right sums of every window, from 0.0, over w."""
    count = len(d) - w + 1
    s = numpy.zeros(count)
    for j in range(w):
        s = s + d[j:j + count]
    return s / numpy.float64(w)


def width_part(d, keep, t, w, span, min_count):
    """(count, robust, rms) of one width of one curve of status 0."""
    n = len(d)
    count_all = n - w + 1
    bad = numpy.concatenate([[0], numpy.cumsum(~keep)])
    valid = (bad[w:] - bad[:count_all]) == 0
    if t is not None:
        t = numpy.asarray(t, dtype=numpy.float64)
        valid &= (t[w - 1:] - t[:count_all]) <= span
    v = window_means(d, w)
    count = int(valid.sum())
    nan = numpy.float64(numpy.nan)
    if count < min_count:
        return count, nan, nan
    mu = median(v[valid])
    robust = K * median(numpy.fabs(v - mu)[valid])
    c = numpy.float64(count)
    mean = lanes_sum(v, valid) / c
    dv = v - mean
    rms = numpy.sqrt(lanes_sum(dv * dv, valid) / c)
    return count, robust, rms


def noise_profile(y, widths, t=None, clip_upper=5.0, clip_lower=5.0, gap_tolerance=0.5, min_count=3):
    """dict(curve (CURVE_FIELDS), count int64 [W], robust [W], rms [W], beta [W]) of one curve."""
    widths = numpy.asarray(widths, dtype=numpy.int64)
    span_max, pair_span = span_limits(t, widths, gap_tolerance)
    record, d, keep = curve_part(y, t, pair_span, clip_upper, clip_lower)
    W = len(widths)
    count, robust, rms = numpy.zeros(W, dtype=numpy.int64), numpy.full(W, numpy.nan), numpy.full(W, numpy.nan)
    if record["status"] == 0.0:
        for k, w in enumerate(widths):
            count[k], robust[k], rms[k] = width_part(d, keep, t, int(w), span_max[k], min_count)
    with numpy.errstate(all="ignore"):
        beta = robust * numpy.sqrt(widths.astype(numpy.float64)) / record["sigma"]
    return dict(curve=record, count=count, robust=robust, rms=rms, beta=beta)


def noise_profile_batch(rows, widths, t=None, **kw):
    """The device's arrays for rows [R, n]: (records [R] structured with CURVE_FIELDS, count [R, W] int64, robust, rms, beta)."""
    rows = numpy.atleast_2d(numpy.asarray(rows, dtype=numpy.float64))
    parts = [noise_profile(row, widths, t, **kw) for row in rows]
    records = numpy.zeros(len(rows), dtype=[(k, "f8") for k in CURVE_FIELDS])
    for r, p in enumerate(parts):
        for k in CURVE_FIELDS:
            records[k][r] = p["curve"][k]
    stack = lambda key, dtype: numpy.array([p[key] for p in parts], dtype=dtype).reshape(len(rows), len(widths))
    return records, stack("count", numpy.int64), stack("robust", numpy.float64), stack("rms", numpy.float64), stack("beta", numpy.float64)
