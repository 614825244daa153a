"""The trapezoid shape fit of survey.shape_fit (tls_shape_fit), stated in plain Python and numpy: what the device is tested
against bit for bit (include/tls_amd.h tls_shape_record, DESIGN.md "Shape fit").

Inputs: t[n] ascending and finite; one curve's y[n] and dy[n] as survey._batch_inputs hands them out; one candidate (P, T0, d
in days); the ascending tables ratio[nT] > 0, ingress[nQ] with ingress[0] == 0.0 (a box) and ingress[nQ-1] == 0.5 (a V),
shift[nS]; window, min_count >= 1, depth_min >= 0.

    w = 1.0 / (dy * dy);  xw = (1.0 - y) * w                                        # per curve

    status 1 and NaN in every other field unless P, T0, d are finite, P > 0, d > 0 and wd = window * d < 0.5 * P
    members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff fabs(tau) <= wd
    unit (a, b, c), a outermost, c innermost -- unit index (a * nQ + b) * nS + c:
        T = d * ratio[a];  ho = 0.5 * T;  hb = ho * (1.0 - 2.0 * ingress[b])
        r = 1.0 / (ho - hb) where hb < ho;  c0 = d * shift[c]
        cnt = 0; N = 0; D = 0
        over the members in index order:  u = fabs(tau - c0)
            s = 1.0 if u <= hb, else (ho - u) * r if u < ho, else the member does not count
            cnt += 1;  N = N + xw * s;  s2 = s * s;  D = D + w * s2
        valid iff cnt >= min_count and D > 0 and dep = N / D > depth_min;  q = N / sqrt(D)
    best = the valid unit of the largest q, the first in unit order on ties (a unit replaces the held one only if q > held q)
    box, vee = the same pick among the units with b == 0 and with b == nQ - 1
    status 2 (n_points reported, the rest NaN) if no unit is valid

    the record, 16 doubles: status, n_points (the members), n_in (cnt of best), ses (q), depth (dep), depth_err (1 / sqrt(D)),
    duration (T), ingress (ingress[b]), shift (c0), i_duration, i_ingress, i_shift (a, b, c), ses_box, duration_box, ses_vee,
    duration_vee (q and T of box and vee; NaN where that class has no valid unit).

Every step is one IEEE double operation and every sum runs in index order.  `shape_fit_loops` is the statement as loops over
Python floats; `shape_fit` is the vectorised form -- all units of a candidate advance through the members together, each
element on its own chain in member order, and the picks are numpy.argmax (the first of the largest) -- and the two are equal
bit for bit (tests/test_shape_fit_host.py)."""
import math

import numpy

FIELDS = ("status", "n_points", "n_in", "ses", "depth", "depth_err", "duration", "ingress", "shift", "i_duration",
          "i_ingress", "i_shift", "ses_box", "duration_box", "ses_vee", "duration_vee")
MAX_UNITS = 65536
NAN = math.nan

DEFAULT_RATIOS = numpy.geomspace(0.5, 2.0, 17)
DEFAULT_INGRESS = numpy.linspace(0.0, 0.5, 16)
DEFAULT_SHIFTS = numpy.linspace(-0.25, 0.25, 9)


def _div(a, b):
    """a / b as IEEE has it (Python raises on b == 0)."""
    with numpy.errstate(all="ignore"):
        return float(numpy.divide(numpy.float64(a), numpy.float64(b)))


def _floor(x):
    return float(math.floor(x)) if math.isfinite(x) else x


def pairs_of(y, dy):
    """(xw, w) of a curve."""
    y, dy = numpy.asarray(y, dtype=numpy.float64), numpy.asarray(dy, dtype=numpy.float64)
    w = 1.0 / (dy * dy)
    return (1.0 - y) * w, w


def candidate_ok(P, T0, d, window):
    """(ok, wd): whether the candidate has members at all, and its half window in days."""
    P, T0, d = float(P), float(T0), float(d)
    wd = float(window) * d
    ok = math.isfinite(P) and math.isfinite(T0) and math.isfinite(d) and P > 0.0 and d > 0.0 and wd < 0.5 * P
    return ok, wd


def _record(**fields):
    out = {k: NAN for k in FIELDS}
    out.update(fields)
    return [float(out[k]) for k in FIELDS]


def shape_fit_loops(t, y, dy, P, T0, d, ratio, ingress, shift, window=2.0, min_count=3, depth_min=0.0):
    """The record of one candidate, as loops over Python floats."""
    ok, wd = candidate_ok(P, T0, d, window)
    if not ok:
        return _record(status=1.0)
    P, T0, d, depth_min = float(P), float(T0), float(d), float(depth_min)
    ratio, ingress, shift = ([float(v) for v in table] for table in (ratio, ingress, shift))
    nT, nQ, nS = len(ratio), len(ingress), len(shift)
    members = []
    for i in range(len(t)):
        e = float(dy[i])
        w = _div(1.0, e * e)
        xw = (1.0 - float(y[i])) * w
        x = _div(float(t[i]) - T0, P)
        k = _floor(x + 0.5)
        tau = (x - k) * P
        if math.fabs(tau) <= wd:
            members.append((tau, xw, w))
    held = {"all": None, "box": None, "vee": None}
    for a in range(nT):
        T = d * ratio[a]
        ho = 0.5 * T
        for b in range(nQ):
            hb = ho * (1.0 - 2.0 * ingress[b])
            r = _div(1.0, ho - hb) if hb < ho else 0.0
            for c in range(nS):
                c0 = d * shift[c]
                cnt, N, D = 0, 0.0, 0.0
                for tau, xw, w in members:
                    u = math.fabs(tau - c0)
                    if u <= hb:
                        s = 1.0
                    elif u < ho:
                        s = (ho - u) * r
                    else:
                        continue
                    cnt += 1
                    N = N + xw * s
                    s2 = s * s
                    D = D + w * s2
                if not (cnt >= min_count and D > 0.0):
                    continue
                dep = _div(N, D)
                if not (dep > depth_min):
                    continue
                q = _div(N, math.sqrt(D))
                unit = dict(q=q, cnt=cnt, dep=dep, D=D, T=T, a=a, b=b, c=c, c0=c0)
                for name, member in (("all", True), ("box", b == 0), ("vee", b == nQ - 1)):
                    if member and (held[name] is None or q > held[name]["q"]):
                        held[name] = unit
    best, box, vee = held["all"], held["box"], held["vee"]
    if best is None:
        return _record(status=2.0, n_points=len(members))
    return _record(status=0.0, n_points=len(members), n_in=best["cnt"], ses=best["q"], depth=best["dep"],
                   depth_err=_div(1.0, math.sqrt(best["D"])), duration=best["T"], ingress=ingress[best["b"]],
                   shift=best["c0"], i_duration=best["a"], i_ingress=best["b"], i_shift=best["c"],
                   ses_box=NAN if box is None else box["q"], duration_box=NAN if box is None else box["T"],
                   ses_vee=NAN if vee is None else vee["q"], duration_vee=NAN if vee is None else vee["T"])


def members_of(t, P, T0, wd):
    """(indices, tau) of the members of a candidate that candidate_ok admits."""
    t = numpy.asarray(t, dtype=numpy.float64)
    with numpy.errstate(all="ignore"):
        x = (t - float(T0)) / float(P)
        k = numpy.floor(x + 0.5)
        tau = (x - k) * float(P)
    index = numpy.nonzero(numpy.fabs(tau) <= wd)[0]
    return index, tau[index]


def shape_fit(t, y, dy, P, T0, d, ratio, ingress, shift, window=2.0, min_count=3, depth_min=0.0, pairs=None):
    """The record of one candidate, vectorised over the units (pairs: pairs_of(y, dy), where the caller holds it)."""
    ok, wd = candidate_ok(P, T0, d, window)
    if not ok:
        return _record(status=1.0)
    d = float(d)
    ratio, ingress, shift = (numpy.asarray(table, dtype=numpy.float64) for table in (ratio, ingress, shift))
    nT, nQ, nS = len(ratio), len(ingress), len(shift)
    xw_all, w_all = pairs_of(y, dy) if pairs is None else pairs
    index, taus = members_of(t, P, T0, wd)
    ia, ib, ic = (v.reshape(-1) for v in numpy.meshgrid(numpy.arange(nT), numpy.arange(nQ), numpy.arange(nS), indexing="ij"))
    with numpy.errstate(all="ignore"):
        T = d * ratio[ia]
        ho = 0.5 * T
        hb = ho * (1.0 - 2.0 * ingress[ib])
        r = numpy.where(hb < ho, 1.0 / (ho - hb), 0.0)
        c0 = d * shift[ic]
        cnt = numpy.zeros(len(T), dtype=numpy.int64)
        N, D = numpy.zeros(len(T)), numpy.zeros(len(T))
        for tau, xw, w in zip(taus.tolist(), xw_all[index].tolist(), w_all[index].tolist()):
            u = numpy.fabs(tau - c0)
            inner = u <= hb
            counts = inner | (u < ho)
            s = numpy.where(inner, 1.0, (ho - u) * r)
            cnt += counts
            N = numpy.where(counts, N + xw * s, N)
            D = numpy.where(counts, D + w * (s * s), D)
        dep = N / D
        valid = (cnt >= min_count) & (D > 0.0) & (dep > float(depth_min))
        q = N / numpy.sqrt(D)
    if not valid.any():
        return _record(status=2.0, n_points=len(index))

    def pick(among):
        """The first unit of the largest q among the valid ones of a class (q > 0 there), or None."""
        if not among.any():
            return None
        return int(numpy.argmax(numpy.where(among, q, -1.0)))

    best, box, vee = pick(valid), pick(valid & (ib == 0)), pick(valid & (ib == nQ - 1))
    return _record(status=0.0, n_points=len(index), n_in=cnt[best], ses=q[best], depth=dep[best],
                   depth_err=1.0 / numpy.sqrt(D[best]), duration=T[best], ingress=ingress[ib[best]], shift=c0[best],
                   i_duration=ia[best], i_ingress=ib[best], i_shift=ic[best],
                   ses_box=NAN if box is None else q[box], duration_box=NAN if box is None else T[box],
                   ses_vee=NAN if vee is None else q[vee], duration_vee=NAN if vee is None else T[vee])


def shape_fit_batch(t, y_rows, dy_rows, period, T0, duration, curve, ratio, ingress, shift, window=2.0, min_count=3,
                    depth_min=0.0, fit=shape_fit):
    """The records [n_fits, 16] of the candidates (period[f], T0[f], duration[f]) on the rows curve[f]."""
    y_rows, dy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(dy_rows)
    out = numpy.empty((len(period), len(FIELDS)))
    for f in range(len(period)):
        out[f] = fit(t, y_rows[curve[f]], dy_rows[curve[f]], period[f], T0[f], duration[f], ratio, ingress, shift, window,
                     min_count, depth_min)
    return out
