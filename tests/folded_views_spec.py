"""The folded views, stated in plain numpy: what tls_folded_views (tls_amd/csrc/tls_views.hip.h) computes on the device and
survey.folded_views returns, bit for bit, and survey.normalize_views.  This file is the definition.

A candidate is (curve c, P, T0, d, phi_s): y is row c of the batch over the shared, ascending t; d is in days; phi_s is the
phase of the secondary, which may be NaN.  A view is (phi_c, x_min, x_max, w, B, parity).  For every point i, ascending:

    x    = (t[i] - T0) / P
    u    = x - phi_c
    e    = floor(u + 0.5)
    tau  = (u - e) * P                      # days from the view's centre

Bin b (0 <= b < B):

    s    = ((x_max - x_min) - w) / (B - 1)
    lo_b = b * s + x_min
    member iff lo_b <= tau and tau < lo_b + w       (and, with a parity, e - 2 * floor(e / 2) == parity)

Every step is one IEEE double operation in that order -- b * s + x_min is a multiplication and then an addition -- and those
two comparisons alone decide membership: with w > s a point is a member of several bins, with w < s maybe of none, and a point
whose rounding puts it outside every bin is outside every bin.  count[b] is the number of members; median[b] is the middle
member by value for an odd count, (a + b) / 2 of the two middle ones for an even count, NaN for none.  A median depends on
the multiset alone and is unweighted.  n_members of a view is the number of points that are a member of at least one bin.

The five views of a candidate (k = local_durations, width = local_width):

    global      phi_c 0      x_min, x_max = -0.5 * P, 0.5 * P    w = P / n_global    n_global bins
    local       phi_c 0      x_min, x_max = -(k * d), k * d      w = width * d       n_local bins
    local_even  as local, parity 0
    local_odd   as local, parity 1
    secondary   as local, phi_c = phi_s

WHICH IS EVEN: with the fit's own T0 -- power()'s T0 is its first transit, e = 0 -- parity 0 takes the first, third, ...
transit of the series.  Those are power()'s even ones: transit_depths[::2], depth_mean_even (stats.py).  (With a T0 moved by
one period the two views change places: the parity is that of the epoch counted from the T0 given.)

The record (FIELDS): status 0 binned, 1 where P, T0 or d is not finite, P <= 0 or d <= 0 -- then every median is NaN, every
count and every n_* is 0; secondary_status 1, and the secondary view alone NaN / 0, where there is no candidate, phi_s is not
finite or no phases are given; the n_members of the five views."""
import numpy

FIELDS = ("status", "secondary_status", "n_global", "n_local", "n_local_even", "n_local_odd", "n_secondary")
LOCAL = ("local", "local_even", "local_odd", "secondary")
NAMES = ("global",) + LOCAL
DEFAULTS = dict(n_global=2001, n_local=201, local_durations=4.0, local_width=0.16)     # (Astronet's)


def fold(t, P, T0, phi_c):
    """(tau, e) of every point about the centre phi_c."""
    with numpy.errstate(all="ignore"):
        x = (numpy.asarray(t, dtype=numpy.float64) - T0) / P
        u = x - phi_c
        e = numpy.floor(u + 0.5)
        return (u - e) * P, e


def edges(x_min, x_max, w, B):
    """(lo, hi) [B] of the bins of a table."""
    with numpy.errstate(all="ignore"):
        s = ((x_max - x_min) - w) / numpy.float64(B - 1)
        lo = numpy.arange(B, dtype=numpy.float64) * s + x_min
        return lo, lo + w


def median_of(values):
    """The middle member by value, (a + b) / 2 of the two middle ones, NaN of none."""
    v = numpy.sort(numpy.asarray(values, dtype=numpy.float64))
    c = len(v)
    if c == 0:
        return numpy.nan
    return v[c // 2] if c % 2 else (v[c // 2 - 1] + v[c // 2]) / 2.0


def bin_view(tau, e, y, x_min, x_max, w, B, parity=None):
    """(median [B], count [B] int32, n_members) of one view of the folded points."""
    lo, hi = edges(x_min, x_max, w, B)
    with numpy.errstate(all="ignore"):
        member = (lo[:, None] <= tau[None, :]) & (tau[None, :] < hi[:, None])
        if parity is not None:
            member &= (e - 2.0 * numpy.floor(e / 2.0) == parity)[None, :]
    count = member.sum(axis=1).astype(numpy.int32)
    median = numpy.full(B, numpy.nan)
    for b in numpy.nonzero(count)[0]:
        median[b] = median_of(y[member[b]])
    return median, count, int(member.any(axis=0).sum())


def tables(P, d, n_global=2001, n_local=201, local_durations=4.0, local_width=0.16):
    """(x_min, x_max, w, B) of the global and of the local views."""
    with numpy.errstate(all="ignore"):
        P, d = numpy.float64(P), numpy.float64(d)
        kd = numpy.float64(local_durations) * d
        return (-0.5 * P, 0.5 * P, P / numpy.float64(n_global), n_global), (-kd, kd, numpy.float64(local_width) * d, n_local)


def candidate_views(t, y, P, T0, d, phi_s=numpy.nan, **table):
    """(record [7], {name: median, name_count: count}) of one candidate on the row y."""
    par = dict(DEFAULTS, **table)
    n_global, n_local = par["n_global"], par["n_local"]
    views = {}
    for name in NAMES:
        B = n_global if name == "global" else n_local
        views[name], views[name + "_count"] = numpy.full(B, numpy.nan), numpy.zeros(B, dtype=numpy.int32)
    record = numpy.array([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    if not (numpy.isfinite(P) and numpy.isfinite(T0) and numpy.isfinite(d) and P > 0 and d > 0):
        return record, views
    y = numpy.asarray(y, dtype=numpy.float64)
    wide, narrow = tables(P, d, **par)
    tau, e = fold(t, P, T0, 0.0)
    todo = [("global", tau, e, wide, None), ("local", tau, e, narrow, None), ("local_even", tau, e, narrow, 0.0),
            ("local_odd", tau, e, narrow, 1.0)]
    record[0] = 0.0
    if numpy.isfinite(phi_s):
        record[1] = 0.0
        todo.append(("secondary",) + fold(t, P, T0, numpy.float64(phi_s)) + (narrow, None))
    for name, tau_v, e_v, table_v, parity in todo:
        views[name], views[name + "_count"], record[2 + NAMES.index(name)] = bin_view(tau_v, e_v, y, *table_v, parity=parity)
    return record, views


def folded_views(t, y_rows, period, T0, duration, curve=None, secondary_phase=None, **table):
    """(records [n_fits, 7], {name: [n_fits, B], name_count: [n_fits, B]}) of the candidates on the rows curve[f] (None:
    candidate f is row f); secondary_phase None: no secondary view."""
    par = dict(DEFAULTS, **table)
    y_rows = numpy.atleast_2d(numpy.asarray(y_rows, dtype=numpy.float64))
    n_fits = len(period)
    curve = numpy.arange(n_fits) if curve is None else curve
    records = numpy.zeros((n_fits, len(FIELDS)))
    views = {}
    for name in NAMES:
        B = par["n_global"] if name == "global" else par["n_local"]
        views[name], views[name + "_count"] = numpy.full((n_fits, B), numpy.nan), numpy.zeros((n_fits, B), dtype=numpy.int32)
    for f in range(n_fits):
        phi = numpy.nan if secondary_phase is None else secondary_phase[f]
        records[f], one = candidate_views(t, y_rows[curve[f]], period[f], T0[f], duration[f], phi, **par)
        for k, v in one.items():
            views[k][f] = v
    return records, views


def normalize_row(row):
    """A view's row of medians as a vetter takes it: the empty bins (NaN) filled by linear interpolation between the
    neighbouring non-empty ones, the edges held; the row's median subtracted; divided by the absolute value of its minimum,
    so the deepest bin is -1 (a row whose minimum is 0 is left undivided).  A row without a non-empty bin stays NaN."""
    row = numpy.asarray(row, dtype=numpy.float64)
    full = ~numpy.isnan(row)
    if not full.any():
        return numpy.full(row.shape, numpy.nan)
    where = numpy.arange(len(row), dtype=numpy.float64)
    out = numpy.interp(where, where[full], row[full])
    out = out - numpy.median(out)
    low = out.min()
    return out if low == 0.0 else out / abs(low)


def normalize_views(views):
    """normalize_row of every row of every array of medians; the counts as they are."""
    out = {}
    for k, v in views.items():
        if k.endswith("_count"):
            out[k] = numpy.array(v)
            continue
        v = numpy.asarray(v, dtype=numpy.float64)
        flat = v.reshape(-1, v.shape[-1])
        out[k] = numpy.array([normalize_row(r) for r in flat]).reshape(v.shape)
    return out
