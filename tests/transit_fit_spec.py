"""The limb-darkened transit fit of survey.transit_fit (tls_transit_fit), stated in plain Python and numpy: what the device is
tested against bit for bit (include/tls_amd.h tls_transit_fit_record, DESIGN.md "Transit fit").

Inputs: t[n] ascending and finite; one curve's y[n] and dy[n] as survey._batch_inputs hands them out; one candidate (P, T0, d
in days) and its seed row j0 in [0, nK); the profile table k_rows[nK] ascending and > 0 with profile[nK][M + 1],
profile[j][m] = 1 - F(z_m; k_rows[j]) at z_m = (1 + k_rows[j]) m / M and profile[j][M] = 0, every entry finite (the host
forms it: survey.transit_profile); the ascending tables impact[nB] in [0, 1) (the impact parameter as a fraction of 1 + k),
ratio[nT] > 0 and shift[nS]; the sub-exposure offsets sub[S] in days (S == 1 with sub[0] == 0: no smearing); window,
min_count >= 1, delta >= 0.

    w = 1.0 / (dy * dy);  xw = (1.0 - y) * w                                        # per curve

    status 1 and NaN in every other field unless P, T0, d are finite, P > 0, d > 0 and wd = window * d < 0.5 * P
    members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff fabs(tau) <= wd
    x2 = 0;  over the members in index order:  x2 = x2 + (xw * xw) / w

    one pass with profile row j, p = profile[j]:
        e1 = 1.0 + k_rows[j];  e2 = e1 * e1;  sM = M / e1
        unit (ib, a, c), ib outermost, c innermost -- unit index (ib * nT + a) * nS + c:
            b = impact[ib] * e1;  bb = b * b;  cc = e2 - bb
            T = d * ratio[a];  rh = 1.0 / (0.5 * T);  c0 = d * shift[c]
            cnt = 0; N = 0; D = 0
            over the members in index order:
                acc = 0.0;  for s = 0 .. S - 1 in order:
                    ts = tau + sub[s];  v = (ts - c0) * rh;  vv = v * v;  zz = bb + cc * vv
                    sample = 0.0 unless zz < e2 (a NaN is 0.0 too); else
                        z = sqrt(zz);  q = z * sM;  m = min(floor(q), M - 1);  fr = q - m
                        sample = p[m] + (p[m + 1] - p[m]) * fr
                    acc = acc + sample
                mval = acc / S
                the member counts iff mval > 0:  cnt += 1;  N = N + xw * mval;  D = D + w * (mval * mval)
            valid iff cnt >= min_count and D > 0 and A = N / D > 0;  q = N / sqrt(D)
        the pick = the valid unit of the largest q, the first in unit order on ties

    pass 1 uses row j0;  k1 = k_rows[j0] * sqrt(A of its pick);  j1 = the row of the least fabs(k_rows[j] - k1), the lowest j
    on ties;  pass 2 uses row j1 (where j1 == j0 it is pass 1).  status 2 (n_points reported, the rest NaN) if either pass has
    no valid unit.  Of pass 2 and its pick (q, A, cnt, ib, a, c):
        k = k_rows[j1] * sqrt(A);  b = impact[ib] * (1.0 + k_rows[j1]);  T = d * ratio[a];  c0 = d * shift[c]
        the intervals: over the valid units with q_u * q_u >= q * q - delta, the least and the largest of
        k_rows[j1] * sqrt(A_u), b_u, T_u and c0_u

    the record, 24 doubles: status, n_points (the members), n_in (cnt), row_first (j0), row (j1), ses (q), amplitude (A), k, b,
    duration (T), shift (c0), i_impact, i_duration, i_shift, x2, k_lo, k_hi, b_lo, b_hi, duration_lo, duration_hi, shift_lo,
    shift_hi, reserved (0.0 whatever the status).

The geometry is the straight chord at constant speed: the projected separation is z^2 = b^2 + ((1 + k)^2 - b^2) v^2 with
v = (time from mid-transit) / (T / 2), so the contacts are at |v| == 1.  Every step is one IEEE double operation and every
sum runs in index order.  `transit_fit_loops` is the statement as loops over Python floats; `transit_fit` is the vectorised
form -- the samples of all (member, sub-exposure, unit) triples of a block of members are formed at once, element by element
with the same operations, and then added in the same order -- and the two are equal bit for bit
(tests/test_transit_fit_host.py)."""
import math

import numpy

from shape_fit_spec import _div, _floor, candidate_ok, members_of, pairs_of

FIELDS = ("status", "n_points", "n_in", "row_first", "row", "ses", "amplitude", "k", "b", "duration", "shift", "i_impact",
          "i_duration", "i_shift", "x2", "k_lo", "k_hi", "b_lo", "b_hi", "duration_lo", "duration_hi", "shift_lo", "shift_hi",
          "reserved")
MAX_UNITS = 65536
MAX_M = 4096
MAX_SUB = 16
NAN = math.nan

DEFAULT_K_ROWS = numpy.geomspace(0.01, 0.5, 81)
DEFAULT_IMPACTS = numpy.linspace(0.0, 0.96, 13)
DEFAULT_RATIOS = numpy.geomspace(0.7, 1.4, 29)
DEFAULT_SHIFTS = numpy.linspace(-0.1, 0.1, 9)


def sub_offsets(exposure, n_sub):
    """sub[s] = exposure * ((2 s + 1) / (2 S) - 0.5); exposure 0 (or S == 1) is no smearing: [0.0]."""
    if not exposure or n_sub == 1:
        return numpy.zeros(1)
    return float(exposure) * ((2.0 * numpy.arange(n_sub) + 1.0) / (2.0 * n_sub) - 0.5)


def _record(**fields):
    out = {k: NAN for k in FIELDS}
    out["reserved"] = 0.0
    out.update(fields)
    return [float(out[k]) for k in FIELDS]


def nearest_row(k_rows, k1):
    """The row of the least |k_rows[j] - k1|, the lowest j on ties."""
    best, at = None, 0
    for j in range(len(k_rows)):
        gap = math.fabs(float(k_rows[j]) - k1)
        if best is None or gap < best:
            best, at = gap, j
    return at


def _finish(n_points, x2, j0, j1, k_rows, d, e1, impact, ratio, shift, best, interval):
    """The record of a fitted candidate from pass 2's pick (q, A, cnt, ib, a, c) and intervals."""
    q, A, cnt, ib, a, c = best
    kj = float(k_rows[j1])
    return _record(status=0.0, n_points=n_points, n_in=cnt, row_first=j0, row=j1, ses=q, amplitude=A, k=kj * math.sqrt(A),
                   b=float(impact[ib]) * e1, duration=d * float(ratio[a]), shift=d * float(shift[c]), i_impact=ib, i_duration=a,
                   i_shift=c, x2=x2, **interval)


def _pass_loops(members, p, kj, M, d, impact, ratio, shift, sub, min_count):
    """Every unit of one pass, in unit order: (valid, q, A, cnt, b, T, c0)."""
    S = len(sub)
    e1 = 1.0 + kj
    e2 = e1 * e1
    sM = _div(float(M), e1)
    units = []
    for ib in range(len(impact)):
        b = impact[ib] * e1
        bb = b * b
        cc = e2 - bb
        for a in range(len(ratio)):
            T = d * ratio[a]
            rh = _div(1.0, 0.5 * T)
            for c in range(len(shift)):
                c0 = d * shift[c]
                cnt, N, D = 0, 0.0, 0.0
                for tau, xw, w in members:
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
                    mval = acc / float(S)
                    if mval > 0.0:
                        cnt += 1
                        N = N + xw * mval
                        D = D + w * (mval * mval)
                valid, q, A = False, NAN, NAN
                if cnt >= min_count and D > 0.0:
                    A = _div(N, D)
                    if A > 0.0:
                        valid, q = True, _div(N, math.sqrt(D))
                units.append((valid, q, A, cnt, b, T, c0, ib, a, c))
    return units


def _pick_loops(units):
    held = None
    for u in units:
        if u[0] and (held is None or u[1] > held[1]):
            held = u
    return held


def transit_fit_loops(t, y, dy, P, T0, d, j0, k_rows, profile, impact, ratio, shift, sub, window=1.0, min_count=3, delta=1.0):
    """The record of one candidate, as loops over Python floats."""
    ok, wd = candidate_ok(P, T0, d, window)
    if not ok:
        return _record(status=1.0)
    P, T0, d, delta, j0 = float(P), float(T0), float(d), float(delta), int(j0)
    k_rows = [float(v) for v in k_rows]
    impact, ratio, shift, sub = ([float(v) for v in table] for table in (impact, ratio, shift, sub))
    rows = [[float(v) for v in row] for row in numpy.asarray(profile)]
    M = len(rows[0]) - 1
    members, x2 = [], 0.0
    for i in range(len(t)):
        e = float(dy[i])
        w = _div(1.0, e * e)
        xw = (1.0 - float(y[i])) * w
        x = _div(float(t[i]) - T0, P)
        k = _floor(x + 0.5)
        tau = (x - k) * P
        if math.fabs(tau) <= wd:
            members.append((tau, xw, w))
            x2 = x2 + _div(xw * xw, w)
    units = _pass_loops(members, rows[j0], k_rows[j0], M, d, impact, ratio, shift, sub, min_count)
    first = _pick_loops(units)
    if first is None:
        return _record(status=2.0, n_points=len(members))
    j1 = nearest_row(k_rows, k_rows[j0] * math.sqrt(first[2]))
    if j1 != j0:
        units = _pass_loops(members, rows[j1], k_rows[j1], M, d, impact, ratio, shift, sub, min_count)
    best = _pick_loops(units)
    if best is None:
        return _record(status=2.0, n_points=len(members))
    floor = best[1] * best[1] - delta
    lo = [math.inf] * 4
    hi = [-math.inf] * 4
    for valid, q, A, cnt, b, T, c0, ib, a, c in units:
        if valid and q * q >= floor:
            for i, v in enumerate((k_rows[j1] * math.sqrt(A), b, T, c0)):
                lo[i], hi[i] = min(lo[i], v), max(hi[i], v)
    interval = dict(k_lo=lo[0], k_hi=hi[0], b_lo=lo[1], b_hi=hi[1], duration_lo=lo[2], duration_hi=hi[2], shift_lo=lo[3],
                    shift_hi=hi[3])
    return _finish(len(members), x2, j0, j1, k_rows, d, 1.0 + k_rows[j1], impact, ratio, shift,
                   (best[1], best[2], best[3], best[7], best[8], best[9]), interval)


def model_values(taus, p, kj, M, d, impact, ratio, shift, sub, block=128):
    """mval [members, units] of one pass (unit order: ib outermost, c innermost), formed block by block of members."""
    p = numpy.asarray(p, dtype=numpy.float64)
    impact, ratio, shift, sub = (numpy.asarray(v, dtype=numpy.float64) for v in (impact, ratio, shift, sub))
    ib, ia, ic = (v.reshape(-1) for v in numpy.meshgrid(numpy.arange(len(impact)), numpy.arange(len(ratio)),
                                                          numpy.arange(len(shift)), indexing="ij"))
    S = len(sub)
    e1 = 1.0 + float(kj)
    e2 = e1 * e1
    sM = float(M) / e1
    taus = numpy.asarray(taus, dtype=numpy.float64)
    out = numpy.zeros((len(taus), len(ib)))
    with numpy.errstate(all="ignore"):
        b = impact[ib] * e1
        bb = b * b
        cc = e2 - bb
        T = float(d) * ratio[ia]
        rh = 1.0 / (0.5 * T)
        c0 = float(d) * shift[ic]
        for m0 in range(0, len(taus), block):
            ts = taus[m0:m0 + block, None] + sub[None, :]                   # [members, S]
            v = (ts[:, :, None] - c0[None, None, :]) * rh[None, None, :]     # [members, S, units]
            vv = v * v
            zz = bb[None, None, :] + cc[None, None, :] * vv
            inside = zz < e2
            z = numpy.sqrt(numpy.where(inside, zz, 0.0))
            q = z * sM
            m = numpy.minimum(numpy.floor(q), float(M - 1))
            fr = q - m
            at = m.astype(numpy.int64)
            sample = numpy.where(inside, p[at] + (p[at + 1] - p[at]) * fr, 0.0)
            acc = numpy.zeros((sample.shape[0], sample.shape[2]))
            for s in range(S):
                acc = acc + sample[:, s, :]
            out[m0:m0 + block] = acc / float(S)
    return out, (ib, ia, ic, b, T, c0)


def _pass(taus, xw, w, p, kj, M, d, impact, ratio, shift, sub, min_count):
    mval, (ib, ia, ic, b, T, c0) = model_values(taus, p, kj, M, d, impact, ratio, shift, sub)
    units = mval.shape[1]
    cnt = numpy.zeros(units, dtype=numpy.int64)
    N, D = numpy.zeros(units), numpy.zeros(units)
    with numpy.errstate(all="ignore"):
        for i in range(len(taus)):
            mv = mval[i]
            counts = mv > 0.0
            cnt += counts
            N = numpy.where(counts, N + xw[i] * mv, N)
            D = numpy.where(counts, D + w[i] * (mv * mv), D)
        A = N / D
        valid = (cnt >= min_count) & (D > 0.0) & (A > 0.0)
        q = N / numpy.sqrt(D)
    return dict(valid=valid, q=q, A=A, cnt=cnt, ib=ib, ia=ia, ic=ic, b=b, T=T, c0=c0)


def _pick(u):
    """The first unit of the largest q among the valid ones (q > 0 there), or None."""
    if not u["valid"].any():
        return None
    return int(numpy.argmax(numpy.where(u["valid"], u["q"], -1.0)))


def transit_fit(t, y, dy, P, T0, d, j0, k_rows, profile, impact, ratio, shift, sub, window=1.0, min_count=3, delta=1.0,
                pairs=None):
    """The record of one candidate, vectorised (pairs: pairs_of(y, dy), where the caller holds it)."""
    ok, wd = candidate_ok(P, T0, d, window)
    if not ok:
        return _record(status=1.0)
    d, j0 = float(d), int(j0)
    k_rows = numpy.asarray(k_rows, dtype=numpy.float64)
    profile = numpy.asarray(profile, dtype=numpy.float64)
    M = profile.shape[1] - 1
    xw_all, w_all = pairs_of(y, dy) if pairs is None else pairs
    index, taus = members_of(t, P, T0, wd)
    xw, w = xw_all[index], w_all[index]
    x2 = 0.0
    with numpy.errstate(all="ignore"):
        for e in ((xw * xw) / w).tolist():
            x2 = x2 + e
    u = _pass(taus, xw, w, profile[j0], k_rows[j0], M, d, impact, ratio, shift, sub, min_count)
    first = _pick(u)
    if first is None:
        return _record(status=2.0, n_points=len(index))
    j1 = nearest_row(k_rows, float(k_rows[j0] * numpy.sqrt(u["A"][first])))
    if j1 != j0:
        u = _pass(taus, xw, w, profile[j1], k_rows[j1], M, d, impact, ratio, shift, sub, min_count)
    best = _pick(u)
    if best is None:
        return _record(status=2.0, n_points=len(index))
    with numpy.errstate(all="ignore"):
        q = u["q"]
        among = u["valid"] & (q * q >= q[best] * q[best] - float(delta))
        kk = k_rows[j1] * numpy.sqrt(numpy.where(among, u["A"], 1.0))
    interval = {}
    for name, v in (("k", kk), ("b", u["b"]), ("duration", u["T"]), ("shift", u["c0"])):
        interval[name + "_lo"], interval[name + "_hi"] = v[among].min(), v[among].max()
    return _finish(len(index), x2, j0, j1, k_rows, d, 1.0 + float(k_rows[j1]), impact, ratio, shift,
                   (q[best], u["A"][best], int(u["cnt"][best]), int(u["ib"][best]), int(u["ia"][best]), int(u["ic"][best])),
                   interval)


def transit_fit_batch(t, y_rows, dy_rows, period, T0, duration, curve, row_first, k_rows, profile, impact, ratio, shift, sub,
                      window=1.0, min_count=3, delta=1.0, fit=transit_fit):
    """The records [n_fits, 24] of the candidates (period[f], T0[f], duration[f], row_first[f]) on the rows curve[f]."""
    y_rows, dy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(dy_rows)
    out = numpy.empty((len(period), len(FIELDS)))
    for f in range(len(period)):
        out[f] = fit(t, y_rows[curve[f]], dy_rows[curve[f]], period[f], T0[f], duration[f], row_first[f], k_rows, profile,
                     impact, ratio, shift, sub, window, min_count, delta)
    return out
