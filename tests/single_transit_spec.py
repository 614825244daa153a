"""The single-transit search of survey.single_transits (tls_single_transits), stated in plain Python and numpy: what the
device is tested against bit for bit (include/tls_amd.h tls_single_event, DESIGN.md "Single-transit events").

A limb-darkened template of every trial duration slides along the time series itself, not along a fold.  Inputs: t[n]
ascending and finite; one curve's y[n] and dy[n] as survey._batch_inputs hands them out; R rows of strictly ascending widths
L_r in [3, 4096] samples, each with the shape b_r[j] = 1 - reference_transit(L_r, **shape)[j] (0 out of transit, 1 at the
bottom); span_max[r] in days; depth_min >= 0.

    w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb_r[j] = b_r[j] * b_r[j]
    for every centre c in 0..n-1, rows r ascending (nothing held at first):
        h = (L_r - 1) // 2;  lo = c - h;  hi = lo + L_r - 1
        skip if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max[r])        # the window runs over a gap
        N = 0.0; D = 0.0; for j = 0..L_r-1 ascending: N = N + xw[lo+j] * b_r[j];  D = D + w[lo+j] * bb_r[j]
        d = N / D                       # least-squares depth of the template in this window
        skip if not (d > depth_min)     # dips only
        s = N / sqrt(D)                 # single-event statistic: sqrt of the chi^2 the template removes
        take (s, r, d) if nothing is held or s > held s           # the first row wins ties
    ses[c], row[c], depth[c] = held, or NaN, -1, NaN

    events, at most k <= 32: a centre is alive where ses[c] is no NaN and ses[c] >= min_ses; its window is [lo_c, hi_c] of
    its own best row.  Repeat: take the alive centre of the largest ses (the lowest index on ties) and record it; with
    g = int(separation * L) of the taken row, every alive centre whose window meets [lo_c - g, hi_c + g] leaves (integers
    only: lo' <= hi_c + g and hi' >= lo_c - g).  Stop at k events or when nothing is alive.

    record (tls_single_event, 8 doubles): index, time = t[c], ses, depth, row, width, t_first = t[lo], t_last = t[hi];
    ranks past n_events hold index = -1 and NaN in every other field.

Every step is one IEEE double operation (Python floats and numpy's element-wise operations never contract) and every sum
runs in the stated order.  `statistic` is the vectorised form -- all centres of a row, and any number of curves, advance
through j together, each element on its own left-to-right chain -- and `statistic_loops` the double loop itself, one curve;
the two are equal bit for bit (tests/test_single_transit_host.py).  The host adds duration_days = width * dt."""
import math

import numpy

FIELDS = ("index", "time", "ses", "depth", "row", "width", "t_first", "t_last")
MAX_WIDTH, MAX_K = 4096, 32


def shapes_of(widths, **shape):
    """b_r of every width: 1 - reference_transit(L_r, **shape)."""
    from tls_amd.template import reference_transit
    return [1.0 - numpy.asarray(reference_transit(int(L), **shape), dtype=numpy.float64) for L in widths]


def statistic(t, y, dy, widths, shapes, span_max, depth_min=0.0):
    """(ses, row, depth) of every centre, vectorised: y and dy are [n] or [n_curves, n]; the planes have their shape."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y, dy = numpy.asarray(y, dtype=numpy.float64), numpy.asarray(dy, dtype=numpy.float64)
    n = len(t)
    w = 1.0 / (dy * dy)
    xw = (1.0 - y) * w
    ses, depth = numpy.full(y.shape, numpy.nan), numpy.full(y.shape, numpy.nan)
    row = numpy.full(y.shape, -1, dtype=numpy.int64)
    depth_min = numpy.float64(depth_min)
    for r, L in enumerate(int(v) for v in widths):
        h = (L - 1) // 2
        c = numpy.arange(h, n - L // 2)                  # lo = c - h >= 0 and hi = c + L // 2 <= n - 1
        if len(c) == 0:
            continue
        lo = c - h
        hi = lo + L - 1
        whole = t[hi] - t[lo] <= numpy.float64(span_max[r])     # (a NaN span_max keeps nothing)
        c, lo = c[whole], lo[whole]
        if len(c) == 0:
            continue
        b = numpy.asarray(shapes[r], dtype=numpy.float64)
        bb = b * b
        N, D = numpy.zeros(y.shape[:-1] + (len(c),)), numpy.zeros(y.shape[:-1] + (len(c),))
        for j in range(L):
            N = N + xw[..., lo + j] * b[j]
            D = D + w[..., lo + j] * bb[j]
        with numpy.errstate(all="ignore"):
            d = N / D
            s = N / numpy.sqrt(D)
            take = (d > depth_min) & ((row[..., c] < 0) | (s > ses[..., c]))
        for plane, value in ((ses, s), (depth, d), (row, numpy.int64(r))):
            part = plane[..., c]
            part[take] = value[take] if numpy.ndim(value) else value
            plane[..., c] = part
    return ses, row, depth


def statistic_loops(t, y, dy, widths, shapes, span_max, depth_min=0.0):
    """The same for one curve as the statement's double loop over centres and rows, in Python floats."""
    t = [float(v) for v in t]
    n = len(t)
    w = [1.0 / (float(e) * float(e)) for e in dy]
    xw = [(1.0 - float(v)) * w[i] for i, v in enumerate(y)]
    ses, row, depth = [math.nan] * n, [-1] * n, [math.nan] * n
    rows = [[float(v) for v in b] for b in shapes]
    squares = [[v * v for v in b] for b in rows]
    for c in range(n):
        for r, L in enumerate(int(v) for v in widths):
            h = (L - 1) // 2
            lo = c - h
            hi = lo + L - 1
            if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= float(span_max[r])):
                continue
            N = D = 0.0
            b, bb = rows[r], squares[r]
            for j in range(L):
                N = N + xw[lo + j] * b[j]
                D = D + w[lo + j] * bb[j]
            d = N / D
            if not (d > float(depth_min)):
                continue
            s = N / math.sqrt(D)
            if row[c] < 0 or s > ses[c]:
                ses[c], row[c], depth[c] = s, r, d
    return numpy.array(ses), numpy.array(row, dtype=numpy.int64), numpy.array(depth)


def select(t, ses, row, depth, widths, k=8, min_ses=0.0, separation=0.5):
    """(events [k] structured by FIELDS, n_events) of one curve's planes: the greedy selection."""
    n = len(ses)
    widths = [int(v) for v in widths]
    ses_l, row_l = [float(v) for v in ses], [int(v) for v in row]
    alive = [not math.isnan(s) and s >= float(min_ses) for s in ses_l]
    lo = [c - (widths[row_l[c]] - 1) // 2 if row_l[c] >= 0 else 0 for c in range(n)]
    hi = [lo[c] + widths[row_l[c]] - 1 if row_l[c] >= 0 else 0 for c in range(n)]
    events = numpy.zeros(int(k), dtype=[(f, "f8") for f in FIELDS])
    for f in FIELDS:
        events[f] = numpy.nan
    events["index"] = -1
    taken = 0
    while taken < int(k):
        best = -1
        for c in range(n):
            if alive[c] and (best < 0 or ses_l[c] > ses_l[best]):
                best = c
        if best < 0:
            break
        L = widths[row_l[best]]
        events[taken] = (best, t[best], ses_l[best], float(depth[best]), row_l[best], L, t[lo[best]], t[hi[best]])
        taken += 1
        g = int(float(separation) * L)
        first, last = lo[best] - g, hi[best] + g
        for c in range(n):
            if alive[c] and lo[c] <= last and hi[c] >= first:
                alive[c] = False
    return events, taken


def expected(t, y_rows, dy_rows, widths, shapes, span_max, depth_min=0.0, k=8, min_ses=0.0, separation=0.5):
    """(events [n_curves, k], n_events [n_curves], ses, row, depth [n_curves, n]) of a batch of rows."""
    y_rows, dy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(dy_rows)
    ses, row, depth = statistic(t, y_rows, dy_rows, widths, shapes, span_max, depth_min)
    picks = [select(t, ses[i], row[i], depth[i], widths, k, min_ses, separation) for i in range(len(y_rows))]
    return (numpy.array([p[0] for p in picks]), numpy.array([p[1] for p in picks], dtype=numpy.int64), ses, row, depth)
