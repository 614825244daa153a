"""The search of one trial period (the reference's search_period, core.py:96-188) stated as its DEFINITION in plain numpy,
for test_search_spec_host.py, test_input_scales.py and the template-shape modules (template_shapes.py): the yardstick the CPU oracle and the kernels are both read against.

It is neither arithmetic.  The oracle restates the reference's (a running out-of-transit sum, core.py:79-93, plus
`intransit + ootr[i] - edge`), the kernels compute S0 + rs^2 A - 2 rs B in double; this module values a cell as what both
approximate, with every sum in numpy.longdouble (64-bit significand, 2^-64 a step: 2000 times finer than a double).

    search_period(t[n], y[n], dy[n], P, table, params):
      fold      x = t / P;  phase = x - floor(x)                     in double, as the reference (core.py:15-18)
                order = numpy.argsort(phase, kind="mergesort");  f = y[order];  s = dy[order]
      patch     W = the widest width of the table, + 1 if odd;  pf = f ++ f[:W];  ps = s ++ s[:W]       (core.py:113-132)
      cell set  decided as the reference decides it, IN DOUBLE -- the predicate is part of the answer and does not move:
                C = numpy.cumsum(0 ++ pf) (sequential: helpers.running_mean);  durations d: the distinct widths, ascending,
                within [floor(T14min n), ceil(T14max n correction)] (core.py:143-156), each with the FIRST table row of its width;
                mean[i] = 1 - (C[i+d] - C[i]) / d  for i = 0 .. n + W - d;  xth as core.py:50-55;
                a cell (d, i) exists where mean[i] > transit_depth_min and i % xth == 0;
                target_depth = mean[i] * overshoot[row]  (double);  its depth is 1 - target_depth  (double)
      value     in long double, from the double inputs widened:  e = 1 - pf,  w = 1 / ps^2,  q_j = 1 - signal_j,
                rs = target_depth / SIGNAL_DEPTH,
                chi2(d, i) = sum over the n folded points of (f - model)^2 / s^2, model = 1 - q_j rs inside the window
                             (patched positions i .. i + d - 1: it wraps through the patch, so no edge correction) and 1 outside
                           = S0 + rs^2 A - 2 rs B,   S0 = sum_k e_k^2 w_k (k < n),  A = sum_j q_j^2 w_{i+j},  B = sum_j q_j (e w)_{i+j}
      short row a row may be SHORTER than its width, L = len(signal) < d (an eccentric orbit's table: the stability cut-off trims
                the slow side of the transit, transit.py:143-149).  The reference takes the whole window of d samples out of the
                out-of-transit sum and puts back the residuals of the row's first L (core.py:59-70): the last d - L samples
                of the window count for nothing, neither as data nor as model,
                chi2(d, i) = S0 + rs^2 A - 2 rs B - sum_{j = L}^{d - 1} e_{i+j}^2 w_{i+j},   A and B over j < L;
                the cell set, the depth scale (the mean over all d samples) and the stride stay those of the width d, and a
                cell costs L template samples (`inner_steps`).  `pad_short_rows` values the row as if it were padded to d
                with q = 0 (no tail term): what a kernel without the term computes -- for the tests that show the difference.
      select    as the reference: a duration starts from `datapoints` = n and takes the first cell (ascending i) with the
                strictly smallest value below it (core.py:46,71); the period starts from infinity and takes, durations
                ascending, each duration whose value is strictly smaller (core.py:183).  best_row is the row of the duration
                that last lowered the value: a period in which no cell beats n reports the FIRST in-range duration's row with
                depth 0 and chi2 n (not row 0); one without an in-range duration reports infinity, row 0, depth 0.

Beside (chi2, row, depth) a period reports `row_gap`: how far, relative, the values would have to move for another row to
win -- the winner's value against the smallest value any OTHER duration reports (n where none of its cells is below n); in
a period where nothing was fitted, n against the smallest cell of any other duration.  Two arithmetics that agree to less
than the gap must report the same row.  `period_gap` is the same between the smallest and the second smallest chi2 of a list.

`reverse_rows` reads every row backwards (q_j -> q_{L-1-j}): what a kernel that pairs tap j with sample d - 1 - j computes."""
import math

import numpy
from numpy.lib.stride_tricks import sliding_window_view

LD = numpy.longdouble
# the valuation is only a yardstick with a significand wider than a double's: x87 extended precision (every machine the
# suite runs on is x86).  A failure, never a skip.
assert numpy.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is no wider than a double here: %r" % numpy.finfo(LD).eps

# tls_constants.py:20-25,71,78
G = 6.673e-11
R_SUN = 695508000.0
R_JUP = 69911000.0
M_SUN = 1.989 * 1e30
SECONDS_PER_DAY = 86400.0
SIGNAL_DEPTH = 0.5
FRACTIONAL_TRANSIT_DURATION_MAX = 0.12


def t14(R_s, M_s, P, small):
    """grid.py:9-32: the fractional duration of a central transit."""
    P = P * SECONDS_PER_DAY
    R_s = R_SUN * R_s
    M_s = M_SUN * M_s
    if small:
        T14max = R_s * ((4 * P) / (math.pi * G * M_s)) ** (1 / 3)
    else:
        T14max = (R_s + 2 * R_JUP) * ((4 * P) / (math.pi * G * M_s)) ** (1 / 3)
    return min(T14max / P, FRACTIONAL_TRANSIT_DURATION_MAX)


def durations_in_range(t, period, table, params):
    """[(width, first row of that width)] ascending, inside the period's window (core.py:113,143-156,163-165)."""
    n = len(t)
    width = numpy.asarray(table.width, dtype=numpy.int64)
    duration_max = t14(params["R_star_max"], params["M_star_max"], period, small=False)
    duration_min = t14(params["R_star_min"], params["M_star_min"], period, small=True)
    length = float(numpy.max(t) - numpy.min(t))
    naive = length / period
    correction = (naive + 1) / naive
    lo = int(numpy.floor(duration_min * n))
    hi = int(numpy.ceil(duration_max * n * correction))
    return [(int(d), int(numpy.nonzero(width == d)[0][0])) for d in numpy.unique(width) if lo <= d <= hi]


def stride(duration, T0_fit_margin):
    """core.py:50-55"""
    xth = 1
    if T0_fit_margin > 0 and duration > T0_fit_margin:
        xth = max(1, int(duration / (1 / T0_fit_margin)))
    return xth


def fold_order(t, period):
    """core.py:15-18,120: the stable order of the phases, in double."""
    x = numpy.asarray(t, dtype=numpy.float64) / numpy.float64(period)
    return numpy.argsort(x - numpy.floor(x), kind="mergesort")


def search_period(t, y, dy, period, table, params, reverse_rows=False, pad_short_rows=False):
    """dict(chi2 (long double), row, depth, row_gap, evaluated_cells, inner_steps) of one period."""
    t, y, dy = (numpy.asarray(a, dtype=numpy.float64) for a in (t, y, dy))
    period = float(period)
    n = len(t)
    width = numpy.asarray(table.width, dtype=numpy.int64)
    W = int(width.max())
    W += W % 2
    order = fold_order(t, period)
    pf = numpy.append(y[order], y[order][:W])
    ps = numpy.append(dy[order], dy[order][:W])
    C = numpy.cumsum(numpy.insert(pf, 0, 0))

    e = LD(1) - pf.astype(LD)
    w = LD(1) / (ps.astype(LD) * ps.astype(LD))
    ew = e * w
    S0 = numpy.sum((e * e * w)[:n])
    E2 = numpy.cumsum(numpy.insert(e * e * w, 0, LD(0)))        # (long double: a tail term is E2[i + d] - E2[i + L])

    reported, smallest_cell, rows, depths = [], [], [], []      # per in-range duration
    evaluated = steps = 0
    for d, row in durations_in_range(t, period, table, params):
        signal = numpy.asarray(table.values[table.offset[row]: table.offset[row] + table.length[row]], dtype=numpy.float64)
        L = len(signal)
        assert 1 <= L <= d, (row, L, d)
        if reverse_rows:
            signal = signal[::-1]
        mean = 1 - (C[d:] - C[:-d]) / float(d)
        at = numpy.nonzero((mean > params["transit_depth_min"])
                           & (numpy.arange(len(mean)) % stride(d, params["T0_fit_margin"]) == 0))[0]
        value, depth, cell = LD(n), 0.0, LD(numpy.inf)
        if len(at):
            target = mean[at] * float(table.overshoot[row])
            rs = target.astype(LD) / LD(SIGNAL_DEPTH)
            q = LD(1) - signal.astype(LD)
            A = sliding_window_view(w, L)[at] @ (q * q)
            B = sliding_window_view(ew, L)[at] @ q
            chi2 = S0 + rs * rs * A - LD(2) * rs * B
            if L < d and not pad_short_rows:
                chi2 = chi2 - (E2[at + d] - E2[at + L])
            k = int(numpy.argmin(chi2))                          # the first of the smallest: strict '<', ascending i
            cell = chi2[k]
            if cell < value:
                value, depth = cell, float(1 - target[k])
            evaluated += len(at)
            steps += len(at) * L
        reported.append(value)
        smallest_cell.append(cell)
        rows.append(row)
        depths.append(depth)

    out = dict(chi2=LD(numpy.inf), row=0, depth=0.0, row_gap=float("inf"), evaluated_cells=evaluated, inner_steps=steps)
    if not reported:
        return out
    best = 0
    for k in range(1, len(reported)):
        if reported[k] < reported[best]:
            best = k
    out.update(chi2=reported[best], row=rows[best], depth=depths[best])
    if reported[best] < LD(n):
        others = [reported[k] for k in range(len(reported)) if k != best]
    else:
        others = [smallest_cell[k] for k in range(len(reported)) if k != best]
    if others:
        out["row_gap"] = float(abs(min(others) - reported[best]) / reported[best])
    return out


def period_gap(chi2):
    """The relative distance between the smallest and the second smallest chi2 of a list (inf for fewer than two)."""
    v = numpy.sort(numpy.asarray(chi2, dtype=LD))
    return float((v[1] - v[0]) / v[0]) if len(v) > 1 and numpy.isfinite(v[0]) else float("inf")


def search(t, y, dy, periods, table, params, **variant):
    """dict of arrays over the periods (chi2 long double, row, depth, row_gap, evaluated_cells, inner_steps), `period_gap`
    and `argmin`."""
    per = [search_period(t, y, dy, P, table, params, **variant) for P in periods]
    out = {key: numpy.array([p[key] for p in per], dtype=(LD if key == "chi2" else None)) for key in per[0]}
    out["period_gap"] = period_gap(out["chi2"])
    out["argmin"] = int(numpy.argmin(out["chi2"]))
    return out


def distance(chi2, spec_chi2):
    """max |chi2 - spec| / spec over the finite entries, formed in long double."""
    spec_chi2 = numpy.asarray(spec_chi2, dtype=LD)
    finite = numpy.isfinite(spec_chi2)
    if not finite.any():
        return 0.0
    return float(numpy.max(numpy.abs(numpy.asarray(chi2, dtype=LD)[finite] - spec_chi2[finite]) / spec_chi2[finite]))
