"""The individual transit times and the refitted ephemeris of survey.transit_times (tls_transit_times), stated in plain
Python and numpy: what the device is tested against bit for bit (include/tls_amd.h tls_ephemeris and tls_transit_time,
DESIGN.md "Transit times").

Inputs: t[n] ascending and finite; one curve's y[n] and dy[n] as survey._batch_inputs hands them out; one candidate (P, T0,
row r, reach S >= 1); row r has L in [3, 4096] samples, the shape b[j] = 1 - reference_transit(L, **shape)[j] (0 out of
transit, 1 at the bottom) and span_max in days; depth_min >= 0, min_ses, max_epochs.

    w = 1.0 / (dy * dy);  xw = (1.0 - y) * w                                        # per curve
    bb[j] = b[j]*b[j];  g[j] = 0.5 * (b[j+1] - b[j-1]) with b[-1] = b[L] = 0.0      # per row: the shape's slope per sample
    gg[j] = g[j]*g[j];  bg[j] = b[j]*g[j];  h = (L - 1) // 2

    status 1 and NaN in every other field unless P and T0 are finite and P > 0
    e_first = ceil((t[0] - T0) / P);  e_last = floor((t[n-1] - T0) / P);  n_epochs = (e_last - e_first) + 1.0   # doubles
    status 2 unless 1 <= n_epochs <= max_epochs: n_epochs is reported, the rest is NaN

    every epoch e = e_first + i, i = 0 .. n_epochs-1:
        tc = T0 + e * P
        j = first index with t[j] >= tc (n-1 if there is none)
        if j > 0 and tc - t[j-1] <= t[j] - tc:  j = j - 1                # the nearer sample; the lower one on a tie
        for s = -S .. S ascending:
            c = j + s;  lo = c - h;  hi = lo + L - 1
            skip if lo < 0 or hi > n-1 or not (t[hi] - t[lo] <= span_max)
            N = 0; D = 0; for k ascending:  N = N + xw[lo+k]*b[k];  D = D + w[lo+k]*bb[k]
            d = N / D;  skip if not (d > depth_min)
            q = N / sqrt(D);  hold (q, d, c, lo) if nothing is held or q > held q      # the first shift wins ties
        nothing held: epoch status 1, time_linear = tc, the rest NaN
        ses = q, depth = d, index = c;  tm = 0.5 * (t[lo+h] + t[lo+L-1-h])             # the window's centre; t[c] for odd L
        epoch status 3 if not (q >= min_ses)                                           # too weak to time
        epoch status 2 if c-1 < 0 or c+1 > n-1
        H = 0; Bg = 0; G = 0
        for k ascending:  H = H + xw[lo+k]*g[k];  Bg = Bg + w[lo+k]*bg[k];  G = G + w[lo+k]*gg[k]
        delta = (d*Bg - H) / (d*G);  step = 0.5 * (t[c+1] - t[c-1])                    # one Gauss-Newton step of the shift
        epoch status 2 if not (fabs(delta) <= 1.0)                                     # (NaN and G == 0 included)
        epoch status 0:  time = tm + delta*step;  time_err = step / (d * sqrt(G))

    ephemeris over the epochs of status 0, ascending:
        wgt = 1.0/(time_err*time_err);  x = e;  tau = time - T0
        Sw += wgt;  Se += wgt*x;  See += (wgt*x)*x;  St += wgt*tau;  Set += (wgt*x)*tau
        Dl = Sw*See - Se*Se
        where n_timed >= 2 and Dl > 0:
            slope = (Sw*Set - Se*St)/Dl;  icpt = (See*St - Se*Set)/Dl
            period = slope;  T0_fit = T0 + icpt;  period_err = sqrt(Sw/Dl);  T0_err = sqrt(See/Dl)
        where also n_timed >= 3, over the same epochs:
            oc = tau - (icpt + slope*x);  rr = oc/time_err;  chi2 += rr*rr;  ss += oc*oc
            ttv_chi2 = chi2;  ttv_rms = sqrt(ss / n_timed)
            ttv_max_sigma, ttv_max_epoch = the largest fabs(rr) and its epoch (the first on ties)
    everything that cannot be formed is NaN

    records, all doubles: per candidate the 12 of EPHEMERIS_FIELDS; per epoch the 8 of TIME_FIELDS, NaN in every field (the
    epoch included) at ranks past n_epochs and for a candidate of status 1 or 2.

Every step is one IEEE double operation and every sum runs in the stated order.  `transit_times_loops` is the statement as
loops over Python floats; `transit_times` is the vectorised form -- all (epoch, shift) units of a candidate advance through
k together, each element on its own left-to-right chain, and the pick runs over the shifts with all epochs side by side --
and the two are equal bit for bit (tests/test_transit_times_host.py).  They share the ephemeris, a loop over the epochs."""
import math

import numpy

EPHEMERIS_FIELDS = ("status", "n_epochs", "n_timed", "epoch_first", "period", "period_err", "T0", "T0_err", "ttv_chi2",
                    "ttv_rms", "ttv_max_sigma", "ttv_max_epoch")
TIME_FIELDS = ("epoch", "status", "time_linear", "time", "time_err", "ses", "depth", "index")
MAX_WIDTH, MAX_REACH, MAX_EPOCHS = 4096, 4096, 65536
NAN = math.nan


def shapes_of(widths, **shape):
    """b of every width: 1 - reference_transit(L, **shape)."""
    from tls_amd.template import reference_transit
    return [1.0 - numpy.asarray(reference_transit(int(L), **shape), dtype=numpy.float64) for L in widths]


def _div(a, b):
    """a / b as IEEE has it (Python raises on b == 0)."""
    return float(numpy.divide(numpy.float64(a), numpy.float64(b)))


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else NAN


def _round(x, down):
    if not math.isfinite(x):
        return x
    return float(math.floor(x) if down else math.ceil(x))


def row_constants(b):
    """(b, bb, g, gg, bg) of a shape, as lists of Python floats."""
    b = [float(v) for v in b]
    L = len(b)
    bb = [v * v for v in b]
    g = [0.5 * ((b[j + 1] if j + 1 < L else 0.0) - (b[j - 1] if j > 0 else 0.0)) for j in range(L)]
    return b, bb, g, [v * v for v in g], [b[j] * g[j] for j in range(L)]


def epochs_of(t, P, T0, max_epochs):
    """(status, e_first, n_epochs) of a candidate: doubles, NaN where they are not formed."""
    P, T0 = float(P), float(T0)
    if not (math.isfinite(P) and math.isfinite(T0) and P > 0.0):
        return 1, NAN, NAN
    with numpy.errstate(all="ignore"):
        e_first = _round(_div(float(t[0]) - T0, P), False)
        e_last = _round(_div(float(t[-1]) - T0, P), True)
        n_epochs = (e_last - e_first) + 1.0
    if not (1.0 <= n_epochs <= float(max_epochs)):
        return 2, e_first, n_epochs
    return 0, e_first, n_epochs


def ephemeris(T0, epochs, status, time, time_err):
    """The 8 fields behind epoch_first of the candidate's record, from the epoch records: n_timed is computed by the caller."""
    T0 = float(T0)
    timed = [i for i in range(len(epochs)) if status[i] == 0.0]
    out = dict(period=NAN, period_err=NAN, T0=NAN, T0_err=NAN, ttv_chi2=NAN, ttv_rms=NAN, ttv_max_sigma=NAN,
               ttv_max_epoch=NAN)
    Sw = Se = See = St = Set = 0.0
    for i in timed:
        err, x = float(time_err[i]), float(epochs[i])
        wgt = _div(1.0, err * err)
        tau = float(time[i]) - T0
        wx = wgt * x
        Sw = Sw + wgt
        Se = Se + wx
        See = See + wx * x
        St = St + wgt * tau
        Set = Set + wx * tau
    Dl = Sw * See - Se * Se
    if not (len(timed) >= 2 and Dl > 0.0):
        return out
    slope = _div(Sw * Set - Se * St, Dl)
    icpt = _div(See * St - Se * Set, Dl)
    out.update(period=slope, T0=T0 + icpt, period_err=_sqrt(_div(Sw, Dl)), T0_err=_sqrt(_div(See, Dl)))
    if len(timed) < 3:
        return out
    chi2 = ss = 0.0
    held = False
    for i in timed:
        x = float(epochs[i])
        tau = float(time[i]) - T0
        oc = tau - (icpt + slope * x)
        rr = _div(oc, float(time_err[i]))
        chi2 = chi2 + rr * rr
        ss = ss + oc * oc
        if not held or math.fabs(rr) > out["ttv_max_sigma"]:
            held = True
            out["ttv_max_sigma"], out["ttv_max_epoch"] = math.fabs(rr), x
    out.update(ttv_chi2=chi2, ttv_rms=_sqrt(_div(ss, float(len(timed)))))
    return out


def _records(status, e_first, n_epochs, T0, times, max_epochs):
    """(ephemeris [12], times [max_epochs, 8]) from the epoch rows `times` (a list of 8-tuples) of a status-0 candidate, or
    the NaN records of status 1 and 2."""
    out_t = numpy.full((int(max_epochs), len(TIME_FIELDS)), numpy.nan)
    eph = numpy.full(len(EPHEMERIS_FIELDS), numpy.nan)
    eph[0] = status
    if status == 1:
        return eph, out_t
    eph[1] = n_epochs
    if status == 2:
        return eph, out_t
    rows = numpy.array(times, dtype=numpy.float64).reshape(-1, len(TIME_FIELDS))
    out_t[:len(rows)] = rows
    eph[2] = float(numpy.count_nonzero(rows[:, 1] == 0.0))
    eph[3] = e_first
    fit = ephemeris(T0, rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4])
    for k, name in enumerate(EPHEMERIS_FIELDS[4:]):
        eph[4 + k] = fit[name]
    return eph, out_t


def transit_times_loops(t, y, dy, P, T0, b, span_max, S, depth_min=0.0, min_ses=3.0, max_epochs=64):
    """(ephemeris [12], times [max_epochs, 8]) of one candidate on one curve: the statement as loops over Python floats."""
    t = [float(v) for v in t]
    n = len(t)
    P, T0, span_max, depth_min, min_ses, S = float(P), float(T0), float(span_max), float(depth_min), float(min_ses), int(S)
    status, e_first, n_epochs = epochs_of(t, P, T0, max_epochs)
    if status:
        return _records(status, e_first, n_epochs, T0, None, max_epochs)
    w = [_div(1.0, float(e) * float(e)) for e in dy]
    xw = [(1.0 - float(v)) * w[i] for i, v in enumerate(y)]
    b, bb, g, gg, bg = row_constants(b)
    L = len(b)
    h = (L - 1) // 2
    rows = []
    for i in range(int(n_epochs)):
        e = e_first + float(i)
        tc = T0 + e * P
        j = n - 1
        for m in range(n):
            if t[m] >= tc:
                j = m
                break
        if j > 0 and tc - t[j - 1] <= t[j] - tc:
            j = j - 1
        held = None
        for s in range(-S, S + 1):
            c = j + s
            lo = c - h
            hi = lo + L - 1
            if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max):
                continue
            N = D = 0.0
            for k in range(L):
                N = N + xw[lo + k] * b[k]
                D = D + w[lo + k] * bb[k]
            d = _div(N, D)
            if not (d > depth_min):
                continue
            q = _div(N, _sqrt(D))
            if held is None or q > held[0]:
                held = (q, d, c, lo)
        if held is None:
            rows.append((e, 1.0, tc, NAN, NAN, NAN, NAN, NAN))
            continue
        q, d, c, lo = held
        tm = 0.5 * (t[lo + h] + t[lo + L - 1 - h])
        state, time, time_err = 0.0, NAN, NAN
        if not (q >= min_ses):
            state = 3.0
        elif c - 1 < 0 or c + 1 > n - 1:
            state = 2.0
        else:
            H = Bg = G = 0.0
            for k in range(L):
                H = H + xw[lo + k] * g[k]
                Bg = Bg + w[lo + k] * bg[k]
                G = G + w[lo + k] * gg[k]
            delta = _div(d * Bg - H, d * G)
            step = 0.5 * (t[c + 1] - t[c - 1])
            if not (math.fabs(delta) <= 1.0):
                state = 2.0
            else:
                time = tm + delta * step
                time_err = _div(step, d * _sqrt(G))
        rows.append((e, state, tc, time, time_err, q, d, float(c)))
    return _records(0, e_first, n_epochs, T0, rows, max_epochs)


def transit_times(t, y, dy, P, T0, b, span_max, S, depth_min=0.0, min_ses=3.0, max_epochs=64):
    """The same, vectorised over the (epoch, shift) units of the candidate."""
    t = numpy.asarray(t, dtype=numpy.float64)
    n = len(t)
    P, T0, S = float(P), float(T0), int(S)
    status, e_first, n_epochs = epochs_of(t, P, T0, max_epochs)
    if status:
        return _records(status, e_first, n_epochs, T0, None, max_epochs)
    f8 = numpy.float64
    y, dy = numpy.asarray(y, dtype=f8), numpy.asarray(dy, dtype=f8)
    with numpy.errstate(all="ignore"):
        w = 1.0 / (dy * dy)
        xw = (1.0 - y) * w
        b, bb, g, gg, bg = (numpy.array(v, dtype=f8) for v in row_constants(b))
        L = len(b)
        h = (L - 1) // 2
        ne = int(n_epochs)
        e = e_first + numpy.arange(ne, dtype=f8)
        tc = T0 + e * P
        j = numpy.minimum(numpy.searchsorted(t, tc, side="left"), n - 1)
        below = numpy.maximum(j - 1, 0)
        j = numpy.where((j > 0) & (tc - t[below] <= t[j] - tc), j - 1, j)
        c = j[:, None] + numpy.arange(-S, S + 1)[None, :]
        lo = c - h
        hi = lo + L - 1
        whole = (lo >= 0) & (hi <= n - 1)
        whole &= t[numpy.clip(hi, 0, n - 1)] - t[numpy.clip(lo, 0, n - 1)] <= f8(span_max)
        at = lo[whole]
        N, D = numpy.zeros(len(at)), numpy.zeros(len(at))
        for k in range(L):
            N = N + xw[at + k] * b[k]
            D = D + w[at + k] * bb[k]
        d_units = N / D
        ok = numpy.zeros(c.shape, dtype=bool)
        ok[whole] = d_units > f8(depth_min)
        Q, Dp = numpy.full(c.shape, numpy.nan), numpy.full(c.shape, numpy.nan)
        Q[whole] = N / numpy.sqrt(D)
        Dp[whole] = d_units
        held = numpy.zeros(ne, dtype=bool)
        q, d, shift = numpy.full(ne, numpy.nan), numpy.full(ne, numpy.nan), numpy.zeros(ne, dtype=numpy.int64)
        for s in range(2 * S + 1):
            take = ok[:, s] & (~held | (Q[:, s] > q))
            q[take], d[take], shift[take] = Q[take, s], Dp[take, s], s
            held |= take
        rows = numpy.full((ne, len(TIME_FIELDS)), numpy.nan)
        rows[:, 0], rows[:, 1], rows[:, 2] = e, 1.0, tc
        ch = c[numpy.arange(ne), shift]
        rows[held, 5], rows[held, 6], rows[held, 7] = q[held], d[held], ch[held]
        weak = held & ~(q >= f8(min_ses))
        edge = held & ~weak & ((ch - 1 < 0) | (ch + 1 > n - 1))
        rows[weak, 1], rows[edge, 1] = 3.0, 2.0
        fit = numpy.flatnonzero(held & ~weak & ~edge)
        at, cf, df = ch[fit] - h, ch[fit], d[fit]
        H, Bg, G = numpy.zeros(len(fit)), numpy.zeros(len(fit)), numpy.zeros(len(fit))
        for k in range(L):
            H = H + xw[at + k] * g[k]
            Bg = Bg + w[at + k] * bg[k]
            G = G + w[at + k] * gg[k]
        delta = (df * Bg - H) / (df * G)
        step = 0.5 * (t[cf + 1] - t[cf - 1])
        tm = 0.5 * (t[at + h] + t[at + L - 1 - h])
        good = numpy.fabs(delta) <= 1.0
        rows[fit, 1] = numpy.where(good, 0.0, 2.0)
        rows[fit[good], 3] = (tm + delta * step)[good]
        rows[fit[good], 4] = (step / (df * numpy.sqrt(G)))[good]
    return _records(0, e_first, n_epochs, T0, rows, max_epochs)


def expected(t, y_rows, dy_rows, curve, period, T0, row, reach, shapes, span_max, depth_min=0.0, min_ses=3.0, max_epochs=64,
             loops=False):
    """(ephemeris [n_fits], times [n_fits, max_epochs]) as structured arrays, candidate by candidate."""
    y_rows, dy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(dy_rows)
    form = transit_times_loops if loops else transit_times
    eph = numpy.zeros(len(period), dtype=[(f, "f8") for f in EPHEMERIS_FIELDS])
    times = numpy.zeros((len(period), int(max_epochs)), dtype=[(f, "f8") for f in TIME_FIELDS])
    for f in range(len(period)):
        a, b = form(t, y_rows[int(curve[f])], dy_rows[int(curve[f])], period[f], T0[f], shapes[int(row[f])],
                    span_max[int(row[f])], reach[f], depth_min, min_ses, max_epochs)
        eph[f] = tuple(a)
        times[f] = [tuple(r) for r in b]
    return eph, times
