"""The removal of fitted transits of survey.remove_transits (tls_remove_transits), stated in plain Python and numpy: what the
device is tested against bit for bit (include/tls_amd.h, DESIGN.md "Multi-planet search").

Inputs: t[n] finite and non-decreasing; the rows y[n_curves][n]; the candidates f = 0 .. m - 1, each with its curve, the period
P and T0 of a peak and the row j, amplitude A, impact b, duration T and shift c0 of that peak's transit-fit record
(transit_fit_spec: row, amplitude, b, duration, shift); and the tables of that fit: k_rows[nK], profile[nK][M + 1], sub[S].

    candidate constants:  e1 = 1.0 + k_rows[j];  e2 = e1 * e1;  sM = M / e1;  bb = b * b;  cc = e2 - bb;  rh = 1.0 / (0.5 * T)
    status 0 (it takes part) iff P, T0, A, b, T, c0 are finite, P > 0, T > 0, A > 0, b >= 0, bb < e2 and
        A * max_m profile[j][m] < 1.0;  otherwise status 1: skipped, it changes nothing

    model = 1.0 everywhere;  for every point i of a curve, the candidates of that curve that take part, f ascending:
        x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P
        acc = 0.0;  for s = 0 .. S - 1 in order:
            ts = tau + sub[s];  v = (ts - c0) * rh;  vv = v * v;  zz = bb + cc * vv
            sample = 0.0 unless zz < e2 (a NaN is 0.0 too); else
                z = sqrt(zz);  q = z * sM;  m = min(floor(q), M - 1);  fr = q - m
                sample = p[m] + (p[m + 1] - p[m]) * fr
            acc = acc + sample
        mval = acc / S
        where mval > 0:  mod = 1.0 - A * mval;  y[i] = y[i] / mod;  model[i] = model[i] * mod
        elsewhere y[i] and model[i] stay as they are, bit for bit

The sub-samples are those of transit_fit_spec, operation for operation, so mval at a fit's members is that fit's own
(model_values there, for the fit's own unit).  Every step is one IEEE double operation.  `remove_transits_loops` is the
statement as loops over Python floats; `remove_transits` forms a candidate's mval for all points of its curve at once, element
by element with the same operations, and the two are equal bit for bit (tests/test_multi_planet_host.py).

The repeat rule of the multi-planet search (survey.power_batch_multi) is stated here too: a later pass's period P repeats an
earlier planet found at Q iff P lies in one of the windows the peak selection (peaks_spec.windows) draws around Q -- worded
on periods, not on grid indices: fabs(P - r * Q) <= separation * (r * Q) for r = 1 or an r of ratios."""
import math

import numpy

import peaks_spec
from transit_fit_spec import _div, _floor


def constants(kj, M, b, T):
    """(e1, e2, sM, bb, cc, rh) of a candidate on the row of k_rows value kj."""
    e1 = 1.0 + float(kj)
    e2 = e1 * e1
    sM = _div(float(M), e1)
    bb = float(b) * float(b)
    cc = e2 - bb
    rh = _div(1.0, 0.5 * float(T))
    return e1, e2, sM, bb, cc, rh


def takes_part(P, T0, A, b, T, c0, kj, p):
    """Whether the candidate takes part (status 0); p is its profile row [M + 1]."""
    P, T0, A, b, T, c0 = (float(v) for v in (P, T0, A, b, T, c0))
    if not all(math.isfinite(v) for v in (P, T0, A, b, T, c0)):
        return False
    e1, e2, sM, bb, cc, rh = constants(kj, len(p) - 1, b, T)
    return P > 0.0 and T > 0.0 and A > 0.0 and b >= 0.0 and bb < e2 and A * max(float(v) for v in p) < 1.0


def mval_loops(t, P, T0, b, T, c0, kj, p, sub):
    """mval of a candidate that takes part at every time stamp, as loops over Python floats."""
    P, T0, c0 = float(P), float(T0), float(c0)
    p = [float(v) for v in p]
    sub = [float(v) for v in sub]
    M, S = len(p) - 1, len(sub)
    e1, e2, sM, bb, cc, rh = constants(kj, M, b, T)
    out = []
    for ti in t:
        x = _div(float(ti) - T0, P)
        k = _floor(x + 0.5)
        tau = (x - k) * P
        acc = 0.0
        for s in range(S):
            ts = tau + sub[s]
            v = (ts - c0) * rh
            vv = v * v
            zz = bb + cc * vv
            sample = 0.0
            if zz < e2:
                z = math.sqrt(zz)
                q = z * sM
                m = min(int(math.floor(q)), M - 1)
                fr = q - float(m)
                sample = p[m] + (p[m + 1] - p[m]) * fr
            acc = acc + sample
        out.append(acc / float(S))
    return out


def mval(t, P, T0, b, T, c0, kj, p, sub):
    """mval [n] of a candidate that takes part, formed for all time stamps at once."""
    t = numpy.asarray(t, dtype=numpy.float64)
    p = numpy.asarray(p, dtype=numpy.float64)
    sub = numpy.asarray(sub, dtype=numpy.float64)
    M, S = len(p) - 1, len(sub)
    e1, e2, sM, bb, cc, rh = constants(kj, M, b, T)
    P, T0, c0 = float(P), float(T0), float(c0)
    with numpy.errstate(all="ignore"):
        x = (t - T0) / P
        k = numpy.floor(x + 0.5)
        tau = (x - k) * P
        acc = numpy.zeros(len(t))
        for s in range(S):
            ts = tau + sub[s]
            v = (ts - c0) * rh
            vv = v * v
            zz = bb + cc * vv
            inside = zz < e2
            z = numpy.sqrt(numpy.where(inside, zz, 0.0))
            q = z * sM
            m = numpy.minimum(numpy.floor(q), float(M - 1))
            fr = q - m
            at = m.astype(numpy.int64)
            acc = acc + numpy.where(inside, p[at] + (p[at + 1] - p[at]) * fr, 0.0)
        return acc / float(S)


def _inputs(y, curve, columns, k_rows, profile):
    y = numpy.array(numpy.atleast_2d(numpy.asarray(y, dtype=numpy.float64)))
    columns = [numpy.atleast_1d(numpy.asarray(v, dtype=numpy.float64)) for v in columns]
    m = len(columns[0])
    curve = numpy.arange(m) if curve is None else numpy.asarray(curve, dtype=numpy.int64)
    return y, curve, columns, numpy.asarray(k_rows, dtype=numpy.float64), numpy.asarray(profile, dtype=numpy.float64)


def remove_transits_loops(t, y, curve, P, T0, row, A, b, T, c0, k_rows, profile, sub):
    """(rows, model, status) as loops over Python floats.  curve None: candidate f belongs to curve f."""
    y, curve, (P, T0, A, b, T, c0), k_rows, profile = _inputs(y, curve, (P, T0, A, b, T, c0), k_rows, profile)
    rows = [[float(v) for v in r] for r in y]
    model = [[1.0] * len(r) for r in rows]
    status = []
    for f in range(len(P)):
        j = int(row[f])
        if not takes_part(P[f], T0[f], A[f], b[f], T[f], c0[f], k_rows[j], profile[j]):
            status.append(1.0)
            continue
        status.append(0.0)
        c, Af = int(curve[f]), float(A[f])
        mv = mval_loops(t, P[f], T0[f], b[f], T[f], c0[f], k_rows[j], profile[j], sub)
        for i in range(len(mv)):
            if mv[i] > 0.0:
                mod = 1.0 - Af * mv[i]
                rows[c][i] = _div(rows[c][i], mod)
                model[c][i] = model[c][i] * mod
    return numpy.array(rows).reshape(y.shape), numpy.array(model).reshape(y.shape), numpy.array(status)


def remove_transits(t, y, curve, P, T0, row, A, b, T, c0, k_rows, profile, sub):
    """(rows, model, status), a candidate's points all at once.  curve None: candidate f belongs to curve f."""
    rows, curve, (P, T0, A, b, T, c0), k_rows, profile = _inputs(y, curve, (P, T0, A, b, T, c0), k_rows, profile)
    model = numpy.ones_like(rows)
    status = numpy.ones(len(P))
    for f in range(len(P)):                          # (ascending f: the candidates of a curve in their order)
        j = int(row[f])
        if not takes_part(P[f], T0[f], A[f], b[f], T[f], c0[f], k_rows[j], profile[j]):
            continue
        status[f] = 0.0
        c = int(curve[f])
        mv = mval(t, P[f], T0[f], b[f], T[f], c0[f], k_rows[j], profile[j], sub)
        dips = mv > 0.0
        with numpy.errstate(all="ignore"):
            mod = 1.0 - float(A[f]) * mv
            rows[c] = numpy.where(dips, rows[c] / mod, rows[c])
            model[c] = numpy.where(dips, model[c] * mod, model[c])
    return rows, model, status


def is_repeat(period, earlier, separation=0.02, ratios=peaks_spec.HARMONICS):
    """Whether a later pass's `period` repeats the planet found earlier at `earlier` days."""
    return bool(peaks_spec.windows([period], earlier, separation, ratios)[0])
