"""The per-transit event vetting of survey.event_vetting (tls_event_vetting), stated in plain Python and numpy: what the device
is tested against bit for bit (include/tls_amd.h tls_event_summary and tls_event_record, DESIGN.md "Event vetting").  The tests
of a candidate's individual events after the Kepler Robovetter (Thompson et al. 2018, section A.3.7: Rubble, Marshall, Chases,
Zuma): is an event unique in its neighbourhood, does it rest on one sample, does the flux come back to the baseline, and does
the candidate survive without its bad events or without its strongest one.

Inputs, those of transit_times_spec: t[n] ascending and finite; one curve's y[n] and dy[n]; one candidate (P, T0, row r, reach
S >= 1); row r has L in [3, 4096] samples, the shape b and span_max in days; depth_min >= 0, min_ses, max_epochs.  The
candidate also has a chase reach R >= 0, a guard Gd >= 0 (both in samples) and a chase_span > 0 in days; the call has
chase_fraction in (0, 1], chase_min in [0, 1], point_fraction > 0 and step_fraction > 0.

    w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb[k] = b[k]*b[k];  h = (L - 1) // 2
    candidate status 1 / 2 and n_epochs exactly as transit_times_spec.epochs_of
    every epoch e = e_first + i:
        tc, the nearest sample j and the held window (q, d, c, lo) over the shifts -S .. S: the loop of transit_times_spec (the
        same skips, the same chains, the first shift wins ties); N, D of the held window are kept
        nothing held: event status 1, epoch and time_linear = tc reported, every other field NaN
        event status 0:  ses = q;  depth = d;  index = c;  depth_err = 1.0 / sqrt(D)
        point:   pm = xw[lo]*b[0];  k = 1 .. L-1 ascending:  v = xw[lo+k]*b[k];  pm = v if v > pm
                 point_share = pm / N                                  # the numerator's share resting on one sample
        sides:   before over [lo-L, lo-1], after over [lo+L, lo+2L-1]; for a side [a, z]:
                 NaN if a < 0 or z > n-1 or not (t[z] - t[a] <= span_max)
                 Ns = 0; Ws = 0; k ascending:  Ns = Ns + xw[a+k];  Ws = Ws + w[a+k];   side = (Ns / Ws) / d
        chase:   n_chased = 0;  found = False
                 for m = Gd+1 .. R, for c' in (c - m, c + m):  lo' = c' - h;  hi' = lo' + L - 1
                     skip if lo' < 0 or hi' > n-1 or not (t[hi'] - t[lo'] <= span_max)
                     n_chased += 1;  N', D' as N, D (k ascending);  q' = N' / sqrt(D')
                     if fabs(q') >= chase_fraction * q:  dtc = fabs(t[c'] - t[c]);  chase_dt = dtc if not found or dtc < chase_dt
                                                         found = True
                 chases = NaN if n_chased == 0;  1.0 if not found;  else x = chase_dt / chase_span, 1.0 if not (x < 1.0)
                 chase_dt is NaN unless found
        flags = 1 * (not q >= min_ses) + 2 * (point_share > point_fraction)
              + 4 * (before > step_fraction or after > step_fraction) + 8 * (chases < chase_min)     # NaN compares false
        good iff flags == 0
    candidate, over the events of status 0 ascending (n_held of them):
        SN = SN + N;  SD = SD + D;  mes = SN / sqrt(SD);  depth_mean = SN / SD
        ses_max, ses_max_epoch: the largest q and its epoch, the first on ties;  dominance = ses_max / mes
        n_good, mes_good: the same two sums over the good events only (NaN where n_good == 0)
        mes_rest: the same over the held events except the ses_max epoch (NaN where n_held < 2)
        depth_chi2:  r = d_e - depth_mean;  chi2 = chi2 + (r*r)*D_e
        chases_min, chases_mean (sum / count, ascending) over the events whose chases is not NaN; NaN if none
        n_held == 0: n_held = 0, n_good = 0, the rest NaN (status, n_epochs and epoch_first stay)

    records, all doubles: per candidate the 15 of SUMMARY_FIELDS; per epoch the 14 of EVENT_FIELDS, NaN in every field (the
    epoch included) at ranks past n_epochs and for a candidate of status 1 or 2.

chase_dt is a minimum of non-negative doubles and n_chased a count: neither depends on the order the chase windows are visited
in.  Every other sum runs in the stated order, and every step is one IEEE double operation.

mes is formed from each event's BEST shift, so it is biased upward against a strictly linear ephemeris: it is to be compared
with mes_good and mes_rest, which are formed the same way, not with the search's SNR.

`event_vetting_loops` is the statement as loops over Python floats; `event_vetting` is the vectorised form -- the (epoch,
shift) units, the held windows, the side windows and the (epoch, m, side) chase units of a candidate each advance through k
together, every element on its own left-to-right chain -- and the two are equal bit for bit
(tests/test_event_vetting_host.py).  They share the summary, a loop over the events."""
import math

import numpy

from transit_times_spec import _div, _sqrt, epochs_of, row_constants, shapes_of  # noqa: F401 (shapes_of: for the tests)

SUMMARY_FIELDS = ("status", "n_epochs", "epoch_first", "n_held", "n_good", "mes", "mes_good", "mes_rest", "ses_max",
                  "ses_max_epoch", "dominance", "depth_mean", "depth_chi2", "chases_min", "chases_mean")
EVENT_FIELDS = ("epoch", "status", "time_linear", "ses", "depth", "depth_err", "index", "point_share", "before", "after",
                "chases", "chase_dt", "n_chased", "flags")
MAX_CHASE = 8192
NAN = math.nan
DEFAULTS = dict(depth_min=0.0, min_ses=3.0, chase_fraction=0.6, chase_min=0.5, point_fraction=0.5, step_fraction=0.5,
                max_epochs=64)


def _sums(events, N, D, keep):
    """(count, SN / sqrt(SD), SN / SD) over the events i with keep(i), ascending."""
    SN = SD = 0.0
    count = 0
    for i in range(len(events)):
        if keep(i):
            SN = SN + N[i]
            SD = SD + D[i]
            count += 1
    if count == 0:
        return 0, NAN, NAN
    return count, _div(SN, _sqrt(SD)), _div(SN, SD)


def summary(status, e_first, n_epochs, events, N, D):
    """The candidate's record from its event rows (14-tuples) and the N, D of their held windows (NaN where none is held)."""
    out = numpy.full(len(SUMMARY_FIELDS), numpy.nan)
    out[0] = status
    if status == 1:
        return out
    out[1] = n_epochs
    if status == 2:
        return out
    out[2] = e_first
    held = [float(r[1]) == 0.0 for r in events]
    n_held, mes, depth_mean = _sums(events, N, D, lambda i: held[i])
    n_good, mes_good, _ = _sums(events, N, D, lambda i: held[i] and float(events[i][13]) == 0.0)
    out[3], out[4] = float(n_held), float(n_good)
    if n_held == 0:
        return out
    top = None
    for i in range(len(events)):
        if held[i] and (top is None or float(events[i][3]) > float(events[top][3])):
            top = i
    n_rest, mes_rest, _ = _sums(events, N, D, lambda i: held[i] and i != top)
    chi2 = 0.0
    chased, lowest, total = 0, NAN, 0.0
    for i in range(len(events)):
        if not held[i]:
            continue
        r = float(events[i][4]) - depth_mean
        chi2 = chi2 + (r * r) * D[i]
        x = float(events[i][10])
        if not math.isnan(x):
            lowest = x if chased == 0 or x < lowest else lowest
            total = total + x
            chased += 1
    ses_max = float(events[top][3])
    out[5], out[6], out[7] = mes, mes_good, mes_rest
    out[8], out[9], out[10] = ses_max, float(events[top][0]), _div(ses_max, mes)
    out[11], out[12] = depth_mean, chi2
    out[13], out[14] = (lowest, _div(total, float(chased))) if chased else (NAN, NAN)
    return out


def _records(status, e_first, n_epochs, events, N, D, max_epochs):
    """(summary [15], events [max_epochs, 14])."""
    out = numpy.full((int(max_epochs), len(EVENT_FIELDS)), numpy.nan)
    if status == 0:
        rows = numpy.array(events, dtype=numpy.float64).reshape(-1, len(EVENT_FIELDS))
        out[:len(rows)] = rows
        return summary(0, e_first, n_epochs, rows, [float(v) for v in N], [float(v) for v in D]), out
    return summary(status, e_first, n_epochs, None, None, None), out


def _flags(q, share, before, after, chases, min_ses, chase_min, point_fraction, step_fraction):
    return float(1 * (not q >= min_ses) + 2 * (share > point_fraction)
                 + 4 * (before > step_fraction or after > step_fraction) + 8 * (chases < chase_min))


def event_vetting_loops(t, y, dy, P, T0, b, span_max, S, R, Gd, chase_span, depth_min=0.0, min_ses=3.0, chase_fraction=0.6,
                        chase_min=0.5, point_fraction=0.5, step_fraction=0.5, max_epochs=64):
    """(summary [15], events [max_epochs, 14]) of one candidate on one curve: the statement as loops over Python floats."""
    t = [float(v) for v in t]
    n = len(t)
    P, T0, span_max, depth_min, min_ses = float(P), float(T0), float(span_max), float(depth_min), float(min_ses)
    S, R, Gd, chase_span, chase_fraction = int(S), int(R), int(Gd), float(chase_span), float(chase_fraction)
    status, e_first, n_epochs = epochs_of(t, P, T0, max_epochs)
    if status:
        return _records(status, e_first, n_epochs, None, None, None, max_epochs)
    w = [_div(1.0, float(e) * float(e)) for e in dy]
    xw = [(1.0 - float(v)) * w[i] for i, v in enumerate(y)]
    b, bb = row_constants(b)[:2]
    L = len(b)
    h = (L - 1) // 2

    def whole(lo):
        return lo >= 0 and lo + L - 1 <= n - 1 and t[lo + L - 1] - t[lo] <= span_max

    def window(lo):
        N = D = 0.0
        for k in range(L):
            N = N + xw[lo + k] * b[k]
            D = D + w[lo + k] * bb[k]
        return N, D

    events, Ns, Ds = [], [], []
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
            if not whole(lo):
                continue
            N, D = window(lo)
            d = _div(N, D)
            if not (d > depth_min):
                continue
            q = _div(N, _sqrt(D))
            if held is None or q > held[0]:
                held = (q, d, c, lo, N, D)
        if held is None:
            events.append((e, 1.0, tc) + (NAN,) * 11)
            Ns.append(NAN)
            Ds.append(NAN)
            continue
        q, d, c, lo, N, D = held
        pm = xw[lo] * b[0]
        for k in range(1, L):
            v = xw[lo + k] * b[k]
            if v > pm:
                pm = v
        share = _div(pm, N)
        sides = []
        for a in (lo - L, lo + L):
            if not whole(a):
                sides.append(NAN)
                continue
            sn = sw = 0.0
            for k in range(L):
                sn = sn + xw[a + k]
                sw = sw + w[a + k]
            sides.append(_div(_div(sn, sw), d))
        n_chased, found, chase_dt = 0, False, NAN
        for m in range(Gd + 1, R + 1):
            for c2 in (c - m, c + m):
                if not whole(c2 - h):
                    continue
                n_chased += 1
                N2, D2 = window(c2 - h)
                q2 = _div(N2, _sqrt(D2))
                if math.fabs(q2) >= chase_fraction * q:
                    dtc = math.fabs(t[c2] - t[c])
                    if not found or dtc < chase_dt:
                        chase_dt = dtc
                    found = True
        if n_chased == 0:
            chases = NAN
        elif not found:
            chases = 1.0
        else:
            x = _div(chase_dt, chase_span)
            chases = x if x < 1.0 else 1.0
        flags = _flags(q, share, sides[0], sides[1], chases, min_ses, float(chase_min), float(point_fraction), float(step_fraction))
        events.append((e, 0.0, tc, q, d, _div(1.0, _sqrt(D)), float(c), share, sides[0], sides[1], chases, chase_dt,
                       float(n_chased), flags))
        Ns.append(N)
        Ds.append(D)
    return _records(0, e_first, n_epochs, events, Ns, Ds, max_epochs)


def event_vetting(t, y, dy, P, T0, b, span_max, S, R, Gd, chase_span, depth_min=0.0, min_ses=3.0, chase_fraction=0.6,
                  chase_min=0.5, point_fraction=0.5, step_fraction=0.5, max_epochs=64):
    """The same, vectorised over the units of the candidate."""
    t = numpy.asarray(t, dtype=numpy.float64)
    n = len(t)
    P, T0, S, R, Gd = float(P), float(T0), int(S), int(R), int(Gd)
    status, e_first, n_epochs = epochs_of(t, P, T0, max_epochs)
    if status:
        return _records(status, e_first, n_epochs, None, None, None, max_epochs)
    f8 = numpy.float64
    y, dy = numpy.asarray(y, dtype=f8), numpy.asarray(dy, dtype=f8)
    span_max = f8(span_max)
    with numpy.errstate(all="ignore"):
        w = 1.0 / (dy * dy)
        xw = (1.0 - y) * w
        b, bb = (numpy.array(v, dtype=f8) for v in row_constants(b)[:2])
        L = len(b)
        h = (L - 1) // 2

        def whole(lo):
            ok = (lo >= 0) & (lo + L - 1 <= n - 1)
            return ok & (t[numpy.clip(lo + L - 1, 0, n - 1)] - t[numpy.clip(lo, 0, n - 1)] <= span_max)

        def windows(at):
            N, D = numpy.zeros(len(at)), numpy.zeros(len(at))
            for k in range(L):
                N = N + xw[at + k] * b[k]
                D = D + w[at + k] * bb[k]
            return N, D

        ne = int(n_epochs)
        e = e_first + numpy.arange(ne, dtype=f8)
        tc = T0 + e * P
        j = numpy.minimum(numpy.searchsorted(t, tc, side="left"), n - 1)
        below = numpy.maximum(j - 1, 0)
        j = numpy.where((j > 0) & (tc - t[below] <= t[j] - tc), j - 1, j)
        c = j[:, None] + numpy.arange(-S, S + 1)[None, :]
        inside = whole(c - h)
        N, D = windows((c - h)[inside])
        d_units = N / D
        ok = numpy.zeros(c.shape, dtype=bool)
        ok[inside] = d_units > f8(depth_min)
        Q, Dp, Nn, Dd = (numpy.full(c.shape, numpy.nan) for _ in range(4))
        Q[inside], Dp[inside], Nn[inside], Dd[inside] = N / numpy.sqrt(D), d_units, N, D
        held = numpy.zeros(ne, dtype=bool)
        q, shift = numpy.full(ne, numpy.nan), numpy.zeros(ne, dtype=numpy.int64)
        for s in range(2 * S + 1):
            take = ok[:, s] & (~held | (Q[:, s] > q))
            q[take], shift[take] = Q[take, s], s
            held |= take
        every = numpy.arange(ne)
        rows = numpy.full((ne, len(EVENT_FIELDS)), numpy.nan)
        rows[:, 0], rows[:, 1], rows[:, 2] = e, 1.0, tc
        at = numpy.flatnonzero(held)
        ch, qh = c[every, shift][at], q[at]
        dh, Nh, Dh = Dp[every, shift][at], Nn[every, shift][at], Dd[every, shift][at]
        lo = ch - h
        rows[at, 1], rows[at, 3], rows[at, 4], rows[at, 5], rows[at, 6] = 0.0, qh, dh, 1.0 / numpy.sqrt(Dh), ch
        pm = xw[lo] * b[0]
        for k in range(1, L):
            v = xw[lo + k] * b[k]
            pm = numpy.where(v > pm, v, pm)
        rows[at, 7] = pm / Nh
        for column, a in ((8, lo - L), (9, lo + L)):
            side = numpy.flatnonzero(whole(a))
            sn, sw = numpy.zeros(len(side)), numpy.zeros(len(side))
            for k in range(L):
                sn = sn + xw[a[side] + k]
                sw = sw + w[a[side] + k]
            rows[at[side], column] = (sn / sw) / dh[side]
        # the chase units (event, m, side) whose window is whole
        m = numpy.arange(Gd + 1, R + 1)
        offsets = numpy.stack([-m, m], axis=1).reshape(-1)
        n_chased, chase_dt = numpy.zeros(len(at)), numpy.full(len(at), numpy.inf)
        step = max(1, (1 << 20) // max(1, len(offsets)))               # (events a pass: the units of a pass stay bounded)
        for first in range(0, len(at) if len(offsets) else 0, step):
            part = slice(first, first + step)
            c2 = ch[part, None] + offsets[None, :]
            alive = whole(c2 - h)
            owner = numpy.nonzero(alive)[0]
            N2, D2 = windows((c2 - h)[alive])
            q2 = N2 / numpy.sqrt(D2)
            n_chased[part] = alive.sum(axis=1)
            close = numpy.fabs(q2) >= f8(chase_fraction) * qh[part][owner]
            dtc = numpy.fabs(t[c2[alive]] - t[ch[part][owner]])
            numpy.minimum.at(chase_dt, first + owner[close], dtc[close])
        found = numpy.isfinite(chase_dt)
        x = chase_dt / f8(chase_span)
        chases = numpy.where(n_chased == 0, numpy.nan, numpy.where(found & (x < 1.0), x, 1.0))
        rows[at, 10], rows[at, 11], rows[at, 12] = chases, numpy.where(found, chase_dt, numpy.nan), n_chased
        rows[at, 13] = (1.0 * ~(qh >= f8(min_ses)) + 2.0 * (rows[at, 7] > f8(point_fraction))
                        + 4.0 * ((rows[at, 8] > f8(step_fraction)) | (rows[at, 9] > f8(step_fraction)))
                        + 8.0 * (chases < f8(chase_min)))
        Ne, De = numpy.full(ne, numpy.nan), numpy.full(ne, numpy.nan)
        Ne[at], De[at] = Nh, Dh
    return _records(0, e_first, n_epochs, rows, Ne, De, max_epochs)


def expected(t, y_rows, dy_rows, curve, period, T0, row, reach, chase_reach, guard, chase_span, shapes, span_max, loops=False,
             **options):
    """(summary [n_fits], events [n_fits, max_epochs]) as structured arrays, candidate by candidate."""
    y_rows, dy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(dy_rows)
    options = dict(DEFAULTS, **options)
    form = event_vetting_loops if loops else event_vetting
    out = numpy.zeros(len(period), dtype=[(f, "f8") for f in SUMMARY_FIELDS])
    events = numpy.zeros((len(period), int(options["max_epochs"])), dtype=[(f, "f8") for f in EVENT_FIELDS])
    for f in range(len(period)):
        a, b = form(t, y_rows[int(curve[f])], dy_rows[int(curve[f])], period[f], T0[f], shapes[int(row[f])],
                    span_max[int(row[f])], reach[f], chase_reach[f], guard[f], chase_span[f], **options)
        out[f] = tuple(a)
        events[f] = [tuple(r) for r in b]
    return out, events
