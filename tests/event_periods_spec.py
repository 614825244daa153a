"""The period aliases of a pair of single-transit events, survey.event_periods (tls_event_periods), stated in plain Python and
numpy: what the device is tested against bit for bit (include/tls_amd.h tls_event_pair and tls_event_alias, DESIGN.md "Event
periods").

Inputs: t[n] ascending and finite; one curve's y[n] and dy[n] as survey._batch_inputs hands them out; one pair (ca < cb sample
indices, row r, reach S >= 1, offset >= 0 days); row r has L in [3, 4096] samples, the shape b[j] = 1 - reference_transit(L,
**shape)[j] (0 out of transit, 1 at the bottom) and span_max in days; period_min > 0, max_aliases, min_ses, veto_sigma.

    w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb[j] = b[j]*b[j];  h = (L - 1) // 2

    window(c):  lo = c - h;  hi = lo + L - 1
                invalid if lo < 0 or hi > n-1 or not (t[hi] - t[lo] <= span_max)
                N = 0; D = 0; for j ascending:  N = N + xw[lo+j]*b[j];  D = D + w[lo+j]*bb[j]

    look(tc):   j = first index with t[j] >= tc (n-1 if there is none)
                if j > 0 and tc - t[j-1] <= t[j] - tc:  j = j - 1        # tls_transit_times' nearest sample
                for s = -S .. S ascending:
                    c = j + s
                    skip if c < 0 or c > n-1
                    skip if window(c) is invalid
                    skip if not (fabs(t[c] - tc) <= offset)              # a centre at the edge of a gap covers no epoch inside it
                    skip if not (D > 0)
                    q = N / sqrt(D)                                      # signed, NO depth_min test: a missing dip must count
                    hold (q, N, D) if nothing is held or q > held q      # the first shift wins ties
                nothing held: the epoch is uncovered

    ta = t[ca];  tb = t[cb];  dT = tb - ta
    status 1 unless dT > 0                                               # dT is reported, the rest is NaN
    A = look(ta);  B = look(tb)
    status 2 unless both are covered and N_A + N_B > 0                   # dT; pair_mes, pair_depth where both are covered
    pN = N_A + N_B;  pD = D_A + D_B;  pair_depth = pN / pD;  pair_mes = pN / sqrt(pD)
    k_hi = floor(dT / period_min);  n_aliases = k_hi
    status 3 if k_hi < 1                                                 # n_evaluated = n_allowed = 0, no alias
    n_evaluated = min(k_hi, max_aliases)

    alias k = 1 .. n_evaluated:
        P = dT / k;  e_first = ceil((t[0] - ta) / P);  e_last = floor((t[n-1] - ta) / P);  n_epochs = (e_last - e_first) + 1.0
        SN = 0; SD = 0; n_covered = 0; n_seen = 0; worst_sigma = NaN; worst_epoch = NaN
        for e = e_first + i, i = 0 .. n_epochs-1:
            tc = ta + e * P;  look(tc);  uncovered: next epoch
            n_covered += 1;  SN = SN + N;  SD = SD + D
            if q >= min_ses:  n_seen += 1
            if e != 0 and e != k:
                z = (pair_depth - N / D) * sqrt(D)
                if worst_sigma is NaN or z > worst_sigma:  worst_sigma = z;  worst_epoch = e
        mes = SN / sqrt(SD);  depth = SN / SD

    allowed(k) = not (worst_sigma > veto_sigma)                          # NaN: no other covered epoch, allowed
    best = the allowed alias with the largest non-NaN mes (the smallest k on ties, i.e. the longest period)
    longest / shortest = the smallest / largest allowed k;  n_allowed = their count

    records, all doubles: per pair the 16 of PAIR_FIELDS; per alias the 8 of ALIAS_FIELDS, NaN in every field at ranks past
    n_evaluated and for a pair of status != 0.  Everything that cannot be formed is NaN.

Every step is one IEEE double operation and every sum runs in the stated order.  `event_periods_loops` is the statement as loops
over Python floats; `event_periods` is the vectorised form -- the (N, D) of every centre of the row advance through j together,
each on its own left-to-right chain, every (alias, epoch) unit looks its shifts up side by side, and the sums over an alias's
epochs advance epoch by epoch with all aliases side by side -- and the two are equal bit for bit
(tests/test_event_periods_host.py)."""
import bisect
import math

import numpy

PAIR_FIELDS = ("status", "dT", "n_aliases", "n_evaluated", "n_allowed", "pair_mes", "pair_depth", "best_k", "best_period",
               "best_mes", "best_n_covered", "best_n_seen", "longest_k", "longest_period", "shortest_k", "shortest_period")
ALIAS_FIELDS = ("period", "n_epochs", "n_covered", "n_seen", "mes", "depth", "worst_sigma", "worst_epoch")
ALIAS_MAX, MAX_EPOCHS, MAX_POINTS = 4096, 65536, 1 << 20
NAN = math.nan
# the template planet of power()'s defaults (tls_amd/constants.py): the shape of the scenarios below
DEFAULT_SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")


def shapes_of(widths, **shape):
    """b of every width: 1 - reference_transit(L, **shape)."""
    from tls_amd.template import reference_transit
    return [1.0 - numpy.asarray(reference_transit(int(L), **shape), dtype=numpy.float64) for L in widths]


def _div(a, b):
    """a / b as IEEE has it (Python raises on b == 0)."""
    with numpy.errstate(all="ignore"):
        return float(numpy.divide(numpy.float64(a), numpy.float64(b)))


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else NAN


def _records(pair, aliases, max_aliases):
    """(pair [16], aliases [max_aliases, 8]) from a dict of the pair fields that were formed and the alias rows."""
    out = numpy.full(len(PAIR_FIELDS), numpy.nan)
    for k, name in enumerate(PAIR_FIELDS):
        if name in pair:
            out[k] = pair[name]
    table = numpy.full((int(max_aliases), len(ALIAS_FIELDS)), numpy.nan)
    if aliases is not None and len(aliases):
        table[:len(aliases)] = numpy.asarray(aliases, dtype=numpy.float64).reshape(-1, len(ALIAS_FIELDS))
    return out, table


def _summary(pair, rows, veto_sigma):
    """The pair's fields over its alias rows (a list of 8-tuples, alias k = index + 1)."""
    best = longest = shortest = None
    n_allowed = 0
    for i, row in enumerate(rows):
        worst = row[6]
        if worst > veto_sigma:                       # (NaN: allowed)
            continue
        n_allowed += 1
        if longest is None:
            longest = i
        shortest = i
        mes = row[4]
        if not math.isnan(mes) and (best is None or mes > rows[best][4]):
            best = i
    pair["n_allowed"] = float(n_allowed)
    if best is not None:
        pair.update(best_k=float(best + 1), best_period=rows[best][0], best_mes=rows[best][4],
                    best_n_covered=rows[best][2], best_n_seen=rows[best][3])
    if longest is not None:
        pair.update(longest_k=float(longest + 1), longest_period=rows[longest][0], shortest_k=float(shortest + 1),
                    shortest_period=rows[shortest][0])
    return pair


def event_periods_loops(t, y, dy, ca, cb, b, span_max, S, offset, period_min, max_aliases=256, min_ses=3.0, veto_sigma=3.0):
    """(pair [16], aliases [max_aliases, 8]) of one pair on one curve: the statement as loops over Python floats."""
    t = [float(v) for v in t]
    n = len(t)
    span_max, offset, period_min = float(span_max), float(offset), float(period_min)
    min_ses, veto_sigma, S, ca, cb = float(min_ses), float(veto_sigma), int(S), int(ca), int(cb)
    w = [_div(1.0, float(e) * float(e)) for e in dy]
    xw = [(1.0 - float(v)) * w[i] for i, v in enumerate(y)]
    b = [float(v) for v in b]
    bb = [v * v for v in b]
    L = len(b)
    h = (L - 1) // 2
    windows = {}

    def window(c):
        if c not in windows:
            lo = c - h
            hi = lo + L - 1
            if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max):
                windows[c] = None
            else:
                N = D = 0.0
                for j in range(L):
                    N = N + xw[lo + j] * b[j]
                    D = D + w[lo + j] * bb[j]
                windows[c] = (N, D)
        return windows[c]

    def look(tc):
        j = bisect.bisect_left(t, tc)
        if j > n - 1:
            j = n - 1
        if j > 0 and tc - t[j - 1] <= t[j] - tc:
            j = j - 1
        held = None
        for s in range(-S, S + 1):
            c = j + s
            if c < 0 or c > n - 1:
                continue
            v = window(c)
            if v is None:
                continue
            if not (math.fabs(t[c] - tc) <= offset):
                continue
            N, D = v
            if not (D > 0.0):
                continue
            q = _div(N, _sqrt(D))
            if held is None or q > held[0]:
                held = (q, N, D)
        return held

    ta, tb = t[ca], t[cb]
    dT = tb - ta
    pair = dict(status=1.0, dT=dT)
    if not (dT > 0.0):
        return _records(pair, None, max_aliases)
    A, B = look(ta), look(tb)
    pair["status"] = 2.0
    if A is None or B is None:
        return _records(pair, None, max_aliases)
    pN, pD = A[1] + B[1], A[2] + B[2]
    pair_depth, pair_mes = _div(pN, pD), _div(pN, _sqrt(pD))
    pair.update(pair_mes=pair_mes, pair_depth=pair_depth)
    if not (pN > 0.0):
        return _records(pair, None, max_aliases)
    k_hi = float(math.floor(_div(dT, period_min)))
    pair.update(status=3.0, n_aliases=k_hi, n_evaluated=0.0, n_allowed=0.0)
    if k_hi < 1.0:
        return _records(pair, None, max_aliases)
    n_eval = int(min(k_hi, float(max_aliases)))
    pair.update(status=0.0, n_evaluated=float(n_eval))
    rows = []
    for k in range(1, n_eval + 1):
        P = _div(dT, float(k))
        e_first = float(math.ceil(_div(t[0] - ta, P)))
        e_last = float(math.floor(_div(t[n - 1] - ta, P)))
        n_epochs = (e_last - e_first) + 1.0
        SN = SD = 0.0
        n_covered = n_seen = 0
        worst_sigma = worst_epoch = NAN
        for i in range(int(n_epochs)):
            e = e_first + float(i)
            tc = ta + e * P
            r = look(tc)
            if r is None:
                continue
            q, N, D = r
            n_covered += 1
            SN = SN + N
            SD = SD + D
            if q >= min_ses:
                n_seen += 1
            if e != 0.0 and e != float(k):
                z = (pair_depth - _div(N, D)) * _sqrt(D)
                if math.isnan(worst_sigma) or z > worst_sigma:
                    worst_sigma, worst_epoch = z, e
        rows.append((P, n_epochs, float(n_covered), float(n_seen), _div(SN, _sqrt(SD)), _div(SN, SD), worst_sigma, worst_epoch))
    return _records(_summary(pair, rows, veto_sigma), rows, max_aliases)


def plane_of(t, y, dy, b, span_max):
    """(N [n], D [n]) of every centre of one row on one curve, NaN where the window is invalid: the vectorised window()."""
    f8 = numpy.float64
    t, y, dy, b = (numpy.asarray(v, dtype=f8) for v in (t, y, dy, b))
    n, L = len(t), len(b)
    h = (L - 1) // 2
    with numpy.errstate(all="ignore"):
        w = 1.0 / (dy * dy)
        xw = (1.0 - y) * w
        bb = b * b
        c = numpy.arange(n)
        lo = c - h
        hi = lo + L - 1
        whole = (lo >= 0) & (hi <= n - 1)
        whole &= t[numpy.clip(hi, 0, n - 1)] - t[numpy.clip(lo, 0, n - 1)] <= f8(span_max)
        at = lo[whole]
        N, D = numpy.zeros(len(at)), numpy.zeros(len(at))
        for j in range(L):
            N = N + xw[at + j] * b[j]
            D = D + w[at + j] * bb[j]
    pN, pD = numpy.full(n, numpy.nan), numpy.full(n, numpy.nan)
    pN[whole], pD[whole] = N, D
    return pN, pD


def _look(t, pN, pD, tc, S, offset):
    """(covered, q, N, D) of the epochs tc [m]: the vectorised look()."""
    n = len(t)
    m = len(tc)
    with numpy.errstate(all="ignore"):
        j = numpy.minimum(numpy.searchsorted(t, tc, side="left"), n - 1)
        below = numpy.maximum(j - 1, 0)
        j = numpy.where((j > 0) & (tc - t[below] <= t[j] - tc), j - 1, j)
        held = numpy.zeros(m, dtype=bool)
        q, N, D = numpy.full(m, numpy.nan), numpy.full(m, numpy.nan), numpy.full(m, numpy.nan)
        for s in range(-S, S + 1):
            c = j + s
            inside = (c >= 0) & (c <= n - 1)
            cc = numpy.clip(c, 0, n - 1)
            Nc, Dc = pN[cc], pD[cc]
            ok = inside & (numpy.fabs(t[cc] - tc) <= offset) & (Dc > 0.0)     # (an invalid window has D NaN)
            qc = Nc / numpy.sqrt(Dc)
            take = ok & (~held | (qc > q))
            q[take], N[take], D[take] = qc[take], Nc[take], Dc[take]
            held |= take
    return held, q, N, D


def event_periods(t, y, dy, ca, cb, b, span_max, S, offset, period_min, max_aliases=256, min_ses=3.0, veto_sigma=3.0,
                  plane=None):
    """The same, vectorised; plane: plane_of(t, y, dy, b, span_max) where the caller holds it."""
    f8 = numpy.float64
    t = numpy.asarray(t, dtype=f8)
    n = len(t)
    S, ca, cb = int(S), int(ca), int(cb)
    offset, period_min, min_ses, veto_sigma = f8(offset), f8(period_min), f8(min_ses), float(veto_sigma)
    pN, pD = plane_of(t, y, dy, b, span_max) if plane is None else plane
    ta, tb = t[ca], t[cb]
    dT = tb - ta
    pair = dict(status=1.0, dT=float(dT))
    if not (dT > 0.0):
        return _records(pair, None, max_aliases)
    held, _, N2, D2 = _look(t, pN, pD, numpy.array([ta, tb]), S, offset)
    pair["status"] = 2.0
    if not held.all():
        return _records(pair, None, max_aliases)
    with numpy.errstate(all="ignore"):
        pNs, pDs = N2[0] + N2[1], D2[0] + D2[1]
        pair_depth, pair_mes = pNs / pDs, pNs / numpy.sqrt(pDs)
        pair.update(pair_mes=float(pair_mes), pair_depth=float(pair_depth))
        if not (pNs > 0.0):
            return _records(pair, None, max_aliases)
        k_hi = float(numpy.floor(dT / period_min))
        pair.update(status=3.0, n_aliases=k_hi, n_evaluated=0.0, n_allowed=0.0)
        if k_hi < 1.0:
            return _records(pair, None, max_aliases)
        n_eval = int(min(k_hi, float(max_aliases)))
        pair.update(status=0.0, n_evaluated=float(n_eval))
        k = numpy.arange(1, n_eval + 1, dtype=f8)
        P = dT / k
        e_first = numpy.ceil((t[0] - ta) / P)
        e_last = numpy.floor((t[n - 1] - ta) / P)
        n_epochs = (e_last - e_first) + 1.0
        count = n_epochs.astype(numpy.int64)
        # the (alias, epoch) units, alias after alias, and where each alias starts among them
        start = numpy.concatenate(([0], numpy.cumsum(count)))
        alias = numpy.repeat(numpy.arange(n_eval), count)
        i = numpy.arange(start[-1]) - start[alias]
        e = e_first[alias] + i.astype(f8)
        tc = ta + e * P[alias]
        covered, q, N, D = _look(t, pN, pD, tc, S, offset)
        z = (pair_depth - N / D) * numpy.sqrt(D)
        other = covered & (e != 0.0) & (e != k[alias])
        SN, SD = numpy.zeros(n_eval), numpy.zeros(n_eval)
        n_covered, n_seen = numpy.zeros(n_eval), numpy.zeros(n_eval)
        worst_sigma, worst_epoch = numpy.full(n_eval, numpy.nan), numpy.full(n_eval, numpy.nan)
        for step in range(int(count.max())):
            live = numpy.flatnonzero(count > step)
            u = start[live] + step
            cov = covered[u]
            a, u = live[cov], u[cov]
            SN[a] = SN[a] + N[u]
            SD[a] = SD[a] + D[u]
            n_covered[a] += 1.0
            seen = q[u] >= min_ses
            n_seen[a[seen]] += 1.0
            oth = other[u]
            a, u = a[oth], u[oth]
            take = numpy.isnan(worst_sigma[a]) | (z[u] > worst_sigma[a])
            worst_sigma[a[take]], worst_epoch[a[take]] = z[u[take]], e[u[take]]
        mes, depth = SN / numpy.sqrt(SD), SN / SD
    rows = [tuple(float(v) for v in r) for r in zip(P, n_epochs, n_covered, n_seen, mes, depth, worst_sigma, worst_epoch)]
    return _records(_summary(pair, rows, veto_sigma), rows, max_aliases)


PAIR_DTYPE = numpy.dtype([(f, "f8") for f in PAIR_FIELDS])
ALIAS_DTYPE = numpy.dtype([(f, "f8") for f in ALIAS_FIELDS])


def expected(t, y_rows, dy_rows, curve, index_a, index_b, row, reach, offset, shapes, span_max, period_min, max_aliases=256,
             min_ses=3.0, veto_sigma=3.0, loops=False):
    """(pairs [n_pairs], aliases [n_pairs, max_aliases]) as structured arrays, pair by pair; the vectorised form keeps the
    plane of a (curve, row) group for every pair that reads it."""
    y_rows, dy_rows = numpy.atleast_2d(y_rows), numpy.atleast_2d(dy_rows)
    pairs = numpy.zeros(len(curve), dtype=PAIR_DTYPE)
    aliases = numpy.zeros((len(curve), int(max_aliases)), dtype=ALIAS_DTYPE)
    planes = {}
    for f in range(len(curve)):
        c, r = int(curve[f]), int(row[f])
        args = (t, y_rows[c], dy_rows[c], index_a[f], index_b[f], shapes[r], span_max[r], reach[f], offset[f], period_min,
                max_aliases, min_ses, veto_sigma)
        if loops:
            a, b = event_periods_loops(*args)
        else:
            if (c, r) not in planes:
                planes[(c, r)] = plane_of(t, y_rows[c], dy_rows[c], shapes[r], span_max[r])
            a, b = event_periods(*args, plane=planes[(c, r)])
        pairs[f] = tuple(a)
        aliases.view(numpy.float64).reshape(len(curve), int(max_aliases), len(ALIAS_FIELDS))[f] = b
    return pairs, aliases


def allowed(aliases, n_evaluated, veto_sigma):
    """allowed(k) of every rank of an alias table [..., max_aliases]: False past n_evaluated."""
    ranks = numpy.arange(aliases.shape[-1])
    with numpy.errstate(invalid="ignore"):
        return (ranks < numpy.asarray(n_evaluated)[..., None]) & ~(aliases["worst_sigma"] > veto_sigma)


# ---- the two host scenarios of DESIGN.md "Event periods" --------------------------------------------------------------------
def _inject(t, flux, times, depth, b):
    """flux with depth * b (L samples) centred on the sample nearest each of `times`; the centres."""
    L = len(b)
    h = (L - 1) // 2
    centres = []
    for tc in times:
        c = int(numpy.argmin(numpy.abs(t - tc)))
        flux[c - h:c - h + L] -= depth * b
        centres.append(c)
    return centres


def scenario_two_sectors(seed, L=9, noise=3e-4, depth=2.5e-3, period=35.7, cadence=1.0 / 48.0):
    """Two 27-day sectors with 330 days between them, one transit of a P = 35.7 d planet in each (ten periods apart):
    (t, flux, dy, ca, cb, b, span_max, S, offset, true_k)."""
    rng = numpy.random.RandomState(seed)
    one = numpy.arange(int(round(27.0 / cadence))) * cadence
    t = numpy.concatenate((one, one + 27.0 + 330.0))
    b = shapes_of([L], **DEFAULT_SHAPE)[0]
    flux = 1.0 + noise * rng.standard_normal(len(t))
    ca, cb = _inject(t, flux, (13.0, 13.0 + 10 * period), depth, b)
    S = max(1, L // 4)
    return dict(t=t, flux=flux, dy=numpy.full(len(t), noise), ca=ca, cb=cb, b=b, span_max=(L - 1) * cadence * 1.5, S=S,
                offset=(S + 0.5) * cadence, true_k=10, period=period, cadence=cadence)


def scenario_three_transits(seed, L=9, noise=3e-4, depth=2.5e-3, period=11.0, cadence=1.0 / 48.0):
    """A 30-day window with a gap (days 16 to 18) and three transits of a P = 11 d planet (days 3, 14 and 25)."""
    rng = numpy.random.RandomState(seed)
    t = numpy.arange(int(round(30.0 / cadence))) * cadence
    t = t[(t < 16.0) | (t >= 18.0)]
    b = shapes_of([L], **DEFAULT_SHAPE)[0]
    flux = 1.0 + noise * rng.standard_normal(len(t))
    centres = _inject(t, flux, (3.0, 14.0, 25.0), depth, b)
    S = max(1, L // 4)
    return dict(t=t, flux=flux, dy=numpy.full(len(t), noise), centres=centres, b=b, span_max=(L - 1) * cadence * 1.5, S=S,
                offset=(S + 0.5) * cadence, period=period, cadence=cadence)
