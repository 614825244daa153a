"""The cleaning stage of tls_clean_rows (include/tls_amd.h) restated in Python, for test_clean_host.py and test_clean.py: the
bad points of every light curve flagged (missing, the caller's, high and low outliers) and replaced with defined values.
Twice: `clean_row_py` in plain Python floats and lists, `clean_row` in numpy; the two are equal bit for bit.  Every step is
one IEEE double operation in a stated order and the medians are selections (the middle value, or (a + b) / 2.0 of the two
middle ones), so the device's rows, flags and records must equal these bit for bit.  Slow by design.

Inputs: t [n] finite and non-decreasing; y [n_curves, n], which may hold NaN, +-inf, zero and negative values; bad (None, or
y's shape, != 0: the caller's quality flag); window_length in days or None; break_tolerance; sigma_upper and sigma_lower (inf
switches a side off); max_run >= 1; n_iter in [0, 16]; min_points >= 1.

Flags (uint8 a point): 1 missing, not (isfinite(y) and y > 0); 2 the caller's bad; 4 high outlier; 8 low outlier.  A point is
valid while its flags are 0.

Segments and windows are the biweight's (biweight_spec.windows): a new segment starts behind every gap > break_tolerance, the
window of i is the points of its segment with |t_j - t_i| <= 0.5 window_length.

A clip round (up to n_iter; none when both sigmas are inf):
  1. window_length None: centre = median of the row's valid points, and every valid point has a residual.  Otherwise the
     centre of a valid point is the median of the valid points of its window OTHER THAN ITSELF; with fewer than min_points
     such members the point has no residual this round, and the clip cannot flag it.
  2. r_i = y_i - centre_i
  3. fewer than two points with a residual: the rounds end (this round is not counted).
     c0 = median(r);  sigma = 1.4826 * median(|r - c0|) over the points with a residual;  rounds = rounds + 1;  the record's
     center is the row's median (window_length None) or c0 (a sliding centre), its sigma this sigma.
  4. not (sigma > 0): the rounds end.
  5. d_i = r_i - c0;  high: d_i > sigma_upper * sigma;  low candidates: d_i < -(sigma_lower * sigma)
  6. a run is a maximal set of low candidates that are neighbours in the sequence of the round's valid points of one
     segment: an invalid point is stepped over, a valid point that is no candidate (one without a residual, a high one) and a
     segment boundary end a run.  The candidates of a run of at most max_run are flagged low.
  7. nobody flagged: the rounds end.  Fewer than two valid points would be left: the round is not applied, the rounds end.
     Otherwise flags |= 4 (high), |= 8 (low).

Repair, for every point i with flags != 0, a < i < b the nearest valid points inside i's segment:
  both:  y_a where t_b == t_a, else  y_a + (y_b - y_a) * ((t_i - t_a) / (t_b - t_a))
  one:   that neighbour's value;  none: the median of the row's valid points (status |= 1)
  a row without a valid point becomes all 1.0 (status = 2).
Valid points pass through with their bits.

Record (FIELDS): status, n_missing (flags & 1), n_bad (flags & 2), n_high, n_low, n_filled (flags != 0), longest_run (the
longest stretch of consecutive filled indices), rounds, center, sigma (NaN: no round formed them)."""
import math

import numpy

from biweight_spec import windows

FIELDS = ("status", "n_missing", "n_bad", "n_high", "n_low", "n_filled", "longest_run", "rounds", "center", "sigma")
RECORD_DTYPE = numpy.dtype([(k, "f8") for k in FIELDS])
K_MAD = 1.4826
MAX_ITER = 16

DEFAULTS = dict(window_length=None, break_tolerance=0.5, sigma_upper=4.0, sigma_lower=math.inf, max_run=1, n_iter=3,
                min_points=3)


def median(v):
    """numpy.median: the middle value, or (a + b) / 2 of the two middle values."""
    s = numpy.sort(numpy.asarray(v, dtype=numpy.float64))
    m = len(s)
    return s[m // 2] if m % 2 else (s[m // 2 - 1] + s[m // 2]) / 2.0


def segment_starts(t, break_tolerance):
    """new [n] bool: True at 0 and at every j with t[j] - t[j-1] > break_tolerance."""
    t = numpy.asarray(t, dtype=numpy.float64)
    new = numpy.zeros(len(t), dtype=bool)
    new[0] = True
    new[1:] = (t[1:] - t[:-1]) > break_tolerance
    return new


def _runs(new, valid, cand, max_run):
    """The low candidates in runs of at most max_run (step 6)."""
    low = numpy.zeros(len(valid), dtype=bool)
    run = []

    def close():
        if 0 < len(run) <= max_run:
            low[run] = True
        del run[:]

    for i in range(len(valid)):
        if new[i]:
            close()
        if not valid[i]:
            continue
        if cand[i]:
            run.append(i)
        else:
            close()
    close()
    return low


def clean_row(t, y, bad, lo, hi, new, sigma_upper, sigma_lower, max_run, n_iter, min_points):
    """(row, flags, record tuple in FIELDS order) of one curve, numpy form.  lo / hi: the windows, or None for the row's
    median."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    n = len(y)
    flags = numpy.zeros(n, dtype=numpy.uint8)
    with numpy.errstate(invalid="ignore"):
        flags[~(numpy.isfinite(y) & (y > 0.0))] |= 1
    if bad is not None:
        flags[numpy.asarray(bad) != 0] |= 2
    rounds, center, sigma = 0, math.nan, math.nan
    if not (math.isinf(sigma_upper) and math.isinf(sigma_lower)):
        while rounds < n_iter:
            valid = flags == 0
            nv = int(valid.sum())
            r = numpy.full(n, numpy.nan)
            has = numpy.zeros(n, dtype=bool)
            med = math.nan
            if lo is None:
                if nv:
                    med = median(y[valid])
                    r[valid] = y[valid] - med
                    has = valid.copy()
            else:
                for i in numpy.flatnonzero(valid):
                    member = valid[lo[i]:hi[i]].copy()
                    member[i - lo[i]] = False
                    if member.sum() >= min_points:
                        r[i] = y[i] - median(y[lo[i]:hi[i]][member])
                        has[i] = True
            if has.sum() < 2:
                break
            c0 = median(r[has])
            sig = K_MAD * median(numpy.abs(r[has] - c0))
            rounds += 1
            center, sigma = (med if lo is None else c0), sig
            if not sig > 0.0:
                break
            with numpy.errstate(invalid="ignore"):
                d = r - c0
                high = has & (d > sigma_upper * sig)
                cand = has & (d < -(sigma_lower * sig))
            low = _runs(new, valid, cand, max_run)
            fresh = int(high.sum()) + int(low.sum())
            if fresh == 0 or nv - fresh < 2:
                break
            flags[high] |= 4
            flags[low] |= 8
    # repair
    valid = flags == 0
    out = y.copy()
    status = 0
    if not valid.any():
        out[:] = 1.0
        status = 2
    else:
        seg = numpy.cumsum(new)
        idx = numpy.arange(n)
        left = numpy.maximum.accumulate(numpy.where(valid, idx, -1))
        right = numpy.minimum.accumulate(numpy.where(valid, idx, n)[::-1])[::-1]
        row_median = median(y[valid])
        for i in numpy.flatnonzero(~valid):
            a, b = left[i], right[i]
            has_a = a >= 0 and seg[a] == seg[i]
            has_b = b < n and seg[b] == seg[i]
            if has_a and has_b:
                den = t[b] - t[a]
                if den == 0.0:
                    out[i] = y[a]
                else:
                    rise = y[b] - y[a]
                    num = t[i] - t[a]
                    q = num / den
                    step = rise * q
                    out[i] = y[a] + step
            elif has_a:
                out[i] = y[a]
            elif has_b:
                out[i] = y[b]
            else:
                out[i] = row_median
                status |= 1
    filled = flags != 0
    longest = run = 0
    for f in filled:
        run = run + 1 if f else 0
        longest = max(longest, run)
    record = (float(status), float(((flags & 1) != 0).sum()), float(((flags & 2) != 0).sum()), float(((flags & 4) != 0).sum()),
              float(((flags & 8) != 0).sum()), float(filled.sum()), float(longest), float(rounds), float(center), float(sigma))
    return out, flags, record


def _median_py(values):
    s = sorted(values)
    m = len(s)
    return s[m // 2] if m % 2 else (s[m // 2 - 1] + s[m // 2]) / 2.0


def clean_row_py(t, y, bad, lo, hi, new, sigma_upper, sigma_lower, max_run, n_iter, min_points):
    """clean_row in plain Python floats and lists."""
    t = [float(v) for v in t]
    y = [float(v) for v in y]
    n = len(y)
    flags = [0 if (math.isfinite(v) and v > 0.0) else 1 for v in y]
    if bad is not None:
        flags = [f | 2 if b else f for f, b in zip(flags, bad)]
    rounds, center, sigma = 0, math.nan, math.nan
    if not (math.isinf(sigma_upper) and math.isinf(sigma_lower)):
        while rounds < n_iter:
            valid = [f == 0 for f in flags]
            nv = sum(valid)
            r = [None] * n
            med = math.nan
            if lo is None:
                if nv:
                    med = _median_py([y[i] for i in range(n) if valid[i]])
                    for i in range(n):
                        if valid[i]:
                            r[i] = y[i] - med
            else:
                for i in range(n):
                    if valid[i]:
                        member = [y[j] for j in range(int(lo[i]), int(hi[i])) if valid[j] and j != i]
                        if len(member) >= min_points:
                            r[i] = y[i] - _median_py(member)
            rr = [v for v in r if v is not None]
            if len(rr) < 2:
                break
            c0 = _median_py(rr)
            sig = K_MAD * _median_py([abs(v - c0) for v in rr])
            rounds += 1
            center, sigma = (med if lo is None else c0), sig
            if not sig > 0.0:
                break
            up = sigma_upper * sig
            down = -(sigma_lower * sig)
            high = [r[i] is not None and r[i] - c0 > up for i in range(n)]
            cand = [r[i] is not None and r[i] - c0 < down for i in range(n)]
            low = [False] * n
            run = []
            for i in range(n + 1):
                if i == n or new[i]:
                    if 0 < len(run) <= max_run:
                        for j in run:
                            low[j] = True
                    run = []
                if i == n or not valid[i]:
                    continue
                if cand[i]:
                    run.append(i)
                else:
                    if 0 < len(run) <= max_run:
                        for j in run:
                            low[j] = True
                    run = []
            fresh = sum(high) + sum(low)
            if fresh == 0 or nv - fresh < 2:
                break
            flags = [f | (4 if h else 0) | (8 if l else 0) for f, h, l in zip(flags, high, low)]
    valid = [f == 0 for f in flags]
    out = list(y)
    status = 0
    if not any(valid):
        out = [1.0] * n
        status = 2
    else:
        row_median = _median_py([y[i] for i in range(n) if valid[i]])
        for i in range(n):
            if valid[i]:
                continue
            a, has_a = i, False
            while a > 0 and not new[a]:          # (a step from a to a - 1 leaves the segment where new[a])
                a -= 1
                if valid[a]:
                    has_a = True
                    break
            b, has_b = i, False
            while b + 1 < n and not new[b + 1]:
                b += 1
                if valid[b]:
                    has_b = True
                    break
            if has_a and has_b:
                den = t[b] - t[a]
                if den == 0.0:
                    out[i] = y[a]
                else:
                    rise = y[b] - y[a]
                    num = t[i] - t[a]
                    q = num / den
                    step = rise * q
                    out[i] = y[a] + step
            elif has_a:
                out[i] = y[a]
            elif has_b:
                out[i] = y[b]
            else:
                out[i] = row_median
                status |= 1
    longest = run_len = 0
    for f in flags:
        run_len = run_len + 1 if f else 0
        longest = max(longest, run_len)
    record = (float(status), float(sum(1 for f in flags if f & 1)), float(sum(1 for f in flags if f & 2)),
              float(sum(1 for f in flags if f & 4)), float(sum(1 for f in flags if f & 8)), float(sum(1 for f in flags if f)),
              float(longest), float(rounds), float(center), float(sigma))
    return out, flags, record


def clean(t, y, bad=None, window_length=None, break_tolerance=0.5, sigma_upper=4.0, sigma_lower=math.inf, max_run=1, n_iter=3,
          min_points=3, plain=False):
    """(rows [n_curves, n], flags uint8 [n_curves, n], record RECORD_DTYPE [n_curves]) of y [n_curves, n] (or one row) at the
    shared time stamps t.  plain=True runs the plain-Python form."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    rows = y[None, :] if y.ndim == 1 else y
    bad_rows = None if bad is None else numpy.asarray(bad).reshape(rows.shape)
    new = segment_starts(t, break_tolerance)
    lo = hi = None
    if window_length is not None:
        lo, hi = windows(t, window_length, break_tolerance)
    one = clean_row_py if plain else clean_row
    out = numpy.empty(rows.shape, dtype=numpy.float64)
    flags = numpy.empty(rows.shape, dtype=numpy.uint8)
    record = numpy.zeros(len(rows), dtype=RECORD_DTYPE)
    for k, row in enumerate(rows):
        o, f, rec = one(t, row, None if bad_rows is None else bad_rows[k], lo, hi, new, float(sigma_upper), float(sigma_lower),
                        max_run, n_iter, min_points)
        out[k], flags[k], record[k] = o, f, rec
    if y.ndim == 1:
        return out[0], flags[0], record[0]
    return out, flags, record
