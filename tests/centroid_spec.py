"""The centroid-shift test of survey.centroid_test (tls_centroid_test), stated in plain Python and numpy: what the device is
tested against bit for bit (include/tls_amd.h tls_centroid_record, DESIGN.md "Centroid test").

Inputs: t[n] ascending and finite; one curve's y[n] as survey._batch_inputs hands it out; the flux-weighted centroids cx[n] and
cy[n] of the same cadences, in any unit (a NaN or an infinite value skips the point); one candidate (P, T0, d in days); the
shape b[L], L >= 2: 1 - template.reference_transit(L, ...), 0 out of transit and 1 at the bottom; window W >= 1, min_in >= 1,
min_out >= 1, max_epochs >= 1.

    status 1 and NaN in every other field unless P, T0, d are finite, P > 0, d > 0 and wd = W * d < 0.5 * P
    points, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P
        member iff fabs(tau) <= wd and cx[i], cy[i] both finite;  its epoch is k
        v = tau / d + 0.5;  inside iff 0 <= v <= 1
        s = 0.0 if not inside, else  u = v * (L - 1);  j = min(floor(u), L - 2);  fr = u - j;  s = b[j] + (b[j+1] - b[j]) * fr
    status 2 (n_points = the members, the rest NaN) if the epochs holding a member are more than max_epochs
    epoch k, its members in index order:  m = count;  m_in = count(inside);  used iff m_in >= min_in and m - m_in >= min_out
        Ss = Ss + s;  sbar = Ss / m;  for each channel c in (1 - y, cx, cy):  Sc = Sc + c;  cbar = Sc / m           # pass 1
        ds = s - sbar;  De = De + ds * ds;  dc = c - cbar;  Ne[c] = Ne[c] + ds * dc;  Qe[c] = Qe[c] + dc * dc       # pass 2
    used epochs ascending:  D = D + De;  N[c] = N[c] + Ne[c];  Q[c] = Q[c] + Qe[c];  n_points += m;  n_in += m_in
    status 2 (n_epochs, n_skipped, n_points, n_in reported, the rest NaN) unless n_used >= 1 and D > 0
    A[c] = N[c] / D;  dof = n_points - n_used - 1
    var[c] = (Q[c] - A[c] * N[c]) / dof where dof >= 1 and that is > 0, else NaN
    err[c] = sqrt(var[c] / D);  rms[c] = sqrt(var[c])
    chi2[c] = sum over the used epochs with De > 0, ascending, of  r = Ne[c] / De - A[c];  (r * r) * De,  then / var[c]

    the record, 16 doubles: status, n_epochs (the used epochs), n_skipped (epochs with members that are not used), n_points,
    n_in, depth, depth_err (A, err of 1 - y), shift_x, shift_x_err (of cx), shift_y, shift_y_err (of cy), rms_x, rms_y,
    chi2_depth, chi2_x, chi2_y.

Every step is one IEEE double operation and every sum runs in the stated order.  `centroid_loops` is the statement as loops
over Python floats; `centroid` is the vectorised form -- all epochs of a candidate advance through their members together,
each on its own chain in index order -- and the two are equal bit for bit (tests/test_centroid_host.py)."""
import math

import numpy

FIELDS = ("status", "n_epochs", "n_skipped", "n_points", "n_in", "depth", "depth_err", "shift_x", "shift_x_err", "shift_y",
          "shift_y_err", "rms_x", "rms_y", "chi2_depth", "chi2_x", "chi2_y")
SHAPE_SAMPLES = 1025
MAX_EPOCHS = 65536
NAN = math.nan


def _div(a, b):
    """a / b as IEEE has it (Python raises on b == 0)."""
    with numpy.errstate(all="ignore"):
        return float(numpy.divide(numpy.float64(a), numpy.float64(b)))


def _floor(x):
    return float(math.floor(x)) if math.isfinite(x) else x


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN     # (NaN stays NaN: the comparison is false)


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


def _finish(epochs, min_in, min_out):
    """The record from the epochs' (m, m_in, De, Ne[3], Qe[3]) in ascending order: Python floats."""
    n_used = n_skipped = n_points = n_in = 0
    D, N, Q = 0.0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    used = []
    for m, m_in, De, Ne, Qe in epochs:
        if not (m_in >= min_in and m - m_in >= min_out):
            n_skipped += 1
            continue
        n_used += 1
        n_points += m
        n_in += m_in
        D = D + De
        for c in range(3):
            N[c] = N[c] + Ne[c]
            Q[c] = Q[c] + Qe[c]
        used.append((De, Ne))
    if not (n_used >= 1 and D > 0.0):
        return _record(status=2.0, n_epochs=n_used, n_skipped=n_skipped, n_points=n_points, n_in=n_in)
    dof = n_points - n_used - 1
    A, err, rms, chi2 = [], [], [], []
    for c in range(3):
        a = _div(N[c], D)
        var = NAN
        if dof >= 1:
            var = _div(Q[c] - a * N[c], float(dof))
            if not var > 0.0:
                var = NAN
        total = 0.0
        for De, Ne in used:
            if De > 0.0:
                r = _div(Ne[c], De) - a
                total = total + (r * r) * De
        A.append(a)
        err.append(_sqrt(_div(var, D)))
        rms.append(_sqrt(var))
        chi2.append(_div(total, var))
    return _record(status=0.0, n_epochs=n_used, n_skipped=n_skipped, n_points=n_points, n_in=n_in, depth=A[0], depth_err=err[0],
                   shift_x=A[1], shift_x_err=err[1], shift_y=A[2], shift_y_err=err[2], rms_x=rms[1], rms_y=rms[2],
                   chi2_depth=chi2[0], chi2_x=chi2[1], chi2_y=chi2[2])


def centroid_loops(t, y, cx, cy, P, T0, d, b, window=3.0, min_in=1, min_out=3, max_epochs=MAX_EPOCHS):
    """The record of one candidate, as loops over Python floats."""
    ok, wd = candidate_ok(P, T0, d, window)
    if not ok:
        return _record(status=1.0)
    P, T0, d = float(P), float(T0), float(d)
    b = [float(v) for v in b]
    L = len(b)
    top = float(L - 1)
    members = []                                     # per epoch: [k, [(s, inside, c0, c1, c2), ...]]
    count = 0
    for i in range(len(t)):
        x = _div(float(t[i]) - T0, P)
        k = _floor(x + 0.5)
        tau = (x - k) * P
        px, py = float(cx[i]), float(cy[i])
        if not (math.fabs(tau) <= wd and math.isfinite(px) and math.isfinite(py)):
            continue
        v = _div(tau, d) + 0.5
        inside = 0.0 <= v <= 1.0
        s = 0.0
        if inside:
            u = v * top
            j = min(int(math.floor(u)), L - 2)
            fr = u - float(j)
            s = b[j] + (b[j + 1] - b[j]) * fr
        if not members or members[-1][0] != k:
            members.append([k, []])
        members[-1][1].append((s, inside, 1.0 - float(y[i]), px, py))
        count += 1
    if len(members) > max_epochs:
        return _record(status=2.0, n_points=count)
    epochs = []
    for _, rows in members:
        m = len(rows)
        m_in = sum(1 for row in rows if row[1])
        Ss, Sc = 0.0, [0.0, 0.0, 0.0]
        for row in rows:
            Ss = Ss + row[0]
            for c in range(3):
                Sc[c] = Sc[c] + row[2 + c]
        sbar = _div(Ss, float(m))
        cbar = [_div(Sc[c], float(m)) for c in range(3)]
        De, Ne, Qe = 0.0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for row in rows:
            ds = row[0] - sbar
            De = De + ds * ds
            for c in range(3):
                dc = row[2 + c] - cbar[c]
                Ne[c] = Ne[c] + ds * dc
                Qe[c] = Qe[c] + dc * dc
        epochs.append((m, m_in, De, Ne, Qe))
    return _finish(epochs, min_in, min_out)


def members_of(t, cx, cy, P, T0, d, wd, b):
    """(indices, epoch k, inside, s) of the members of a candidate that candidate_ok admits, vectorised over the points."""
    t, cx, cy, b = (numpy.asarray(v, dtype=numpy.float64) for v in (t, cx, cy, b))
    L = len(b)
    with numpy.errstate(all="ignore"):
        x = (t - float(T0)) / float(P)
        k = numpy.floor(x + 0.5)
        tau = (x - k) * float(P)
        index = numpy.nonzero((numpy.fabs(tau) <= wd) & numpy.isfinite(cx) & numpy.isfinite(cy))[0]
        v = tau[index] / float(d) + 0.5
        inside = (v >= 0.0) & (v <= 1.0)
        u = numpy.where(inside, v, 0.0) * float(L - 1)
        j = numpy.minimum(numpy.floor(u).astype(numpy.int64), L - 2)
        fr = u - j.astype(numpy.float64)
        s = numpy.where(inside, b[j] + (b[j + 1] - b[j]) * fr, 0.0)
    return index, k[index], inside, s


def centroid(t, y, cx, cy, P, T0, d, b, window=3.0, min_in=1, min_out=3, max_epochs=MAX_EPOCHS):
    """The record of one candidate, vectorised over the points and over the epochs."""
    ok, wd = candidate_ok(P, T0, d, window)
    if not ok:
        return _record(status=1.0)
    index, k, inside, s = members_of(t, cx, cy, P, T0, d, wd, b)
    if len(index) == 0:
        return _finish([], min_in, min_out)
    start = numpy.concatenate(([0], numpy.nonzero(k[1:] != k[:-1])[0] + 1))
    if len(start) > max_epochs:
        return _record(status=2.0, n_points=len(index))
    m = numpy.diff(numpy.concatenate((start, [len(index)])))
    m_in = numpy.add.reduceat(inside.astype(numpy.int64), start)
    chan = numpy.stack([1.0 - numpy.asarray(y, dtype=numpy.float64)[index], numpy.asarray(cx, dtype=numpy.float64)[index],
                        numpy.asarray(cy, dtype=numpy.float64)[index]])
    E = len(start)
    Ss, Sc = numpy.zeros(E), numpy.zeros((3, E))
    for step in range(int(m.max())):                 # pass 1: every epoch's chain takes its member `step`
        live = numpy.nonzero(m > step)[0]
        at = start[live] + step
        Ss[live] = Ss[live] + s[at]
        Sc[:, live] = Sc[:, live] + chan[:, at]
    mf = m.astype(numpy.float64)
    sbar, cbar = Ss / mf, Sc / mf
    De, Ne, Qe = numpy.zeros(E), numpy.zeros((3, E)), numpy.zeros((3, E))
    for step in range(int(m.max())):                 # pass 2
        live = numpy.nonzero(m > step)[0]
        at = start[live] + step
        ds = s[at] - sbar[live]
        De[live] = De[live] + ds * ds
        dc = chan[:, at] - cbar[:, live]
        Ne[:, live] = Ne[:, live] + ds * dc
        Qe[:, live] = Qe[:, live] + dc * dc
    return _finish([(int(m[e]), int(m_in[e]), float(De[e]), Ne[:, e].tolist(), Qe[:, e].tolist()) for e in range(E)],
                   min_in, min_out)


def centroid_batch(t, y_rows, cx_rows, cy_rows, period, T0, duration, curve, b, window=3.0, min_in=1, min_out=3,
                   max_epochs=MAX_EPOCHS, fit=centroid):
    """The records [n_fits, 16] of the candidates (period[f], T0[f], duration[f]) on the rows curve[f]."""
    y_rows, cx_rows, cy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(cx_rows), numpy.atleast_2d(cy_rows)
    out = numpy.empty((len(period), len(FIELDS)))
    for f in range(len(period)):
        out[f] = fit(t, y_rows[curve[f]], cx_rows[curve[f]], cy_rows[curve[f]], period[f], T0[f], duration[f], b, window,
                     min_in, min_out, max_epochs)
    return out
