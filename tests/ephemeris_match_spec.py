"""The ephemeris match of survey.ephemeris_match / power_batch(peaks=K, peak_fits=True, ephemeris_match=True)
(tls_ephemeris_match), stated in numpy: what the device is tested against bit for bit (include/tls_amd.h tls_match_record,
DESIGN.md "Ephemeris match").

Candidates on different stars that share a period (or an integer multiple of it) and an epoch are one signal seen more than
once -- a bright eclipsing binary and the faint stars its light spills into (Coughlin et al. 2014) -- and the strongest is its
source.  A period many stars show with no common epoch is a systematic.

    match(star[M] int64, period[M], T0[M], duration[M], strength[M], span, drift_tolerance=0.5, epoch_tolerance=0.5, max_ratio=3):
      good[f] = period, T0, duration, strength of f all finite, period[f] > 0, duration[f] > 0
      a bad f: status 1, every other field NaN; it is invisible to every other candidate
      for a good f and every good g != f with star[g] != star[f], (l, s) = the member of the longer / the shorter period:
          m     = rint(P_l / P_s)                                 (half to even)
          e     = m * P_s;   dP = fabs(P_l - e);   c = span / P_l;   drift = dP * c
          dmax  = fmax(d_f, d_g);   plim = drift_tolerance * dmax;   elim = epoch_tolerance * dmax
          period_match = (m <= max_ratio) and (drift <= plim)
          x     = (T0_l - T0_s) / P_s;   r = rint(x);   u = x - r;   dt = fabs(u) * P_s
          match = period_match and (dt <= elim)
      status = 0;  n_same = #{g: period_match and m == 1};  n_period = #{g: period_match};  n_match = #{g: match}
      best = the g of the match with the largest strength, the lowest index among equals; -1 without a match
      best_ratio = +m if P_best >= P_f else -m;  best_dt, best_drift: that pair's;  best_strength = strength[best]
      child = 1 if strength[best] > strength[f] else 0;  the last five are NaN without a match

Every step is one IEEE double operation (numpy's element-wise operations never contract), counts are integers and the
argmax takes no arithmetic: nothing depends on the order of evaluation.  On equal periods either choice of (l, s) gives the
same bits (m = 1, dP = 0, and x only changes its sign, which rint, fabs and the half-to-even rule do not see), so both
relations are symmetric in (f, g) bit for bit."""
import numpy

FIELDS = ("status", "n_same", "n_period", "n_match", "best", "best_ratio", "best_dt", "best_drift", "best_strength", "child")
DTYPE = numpy.dtype([(k, "f8") for k in FIELDS])
MATCHED, BAD = 0, 1
ROWS = 256      # candidates f evaluated at a time: the statement is all pairs, the working set is ROWS x M


def good(period, T0, duration, strength):
    with numpy.errstate(all="ignore"):
        return (numpy.isfinite(period) & numpy.isfinite(T0) & numpy.isfinite(duration) & numpy.isfinite(strength)
                & (period > 0) & (duration > 0))


def pairs(star, period, T0, duration, strength, span, drift_tolerance, epoch_tolerance, max_ratio, rows):
    """The pair test of the candidates `rows` (an index array [R]) against all M: a dict of [R, M] arrays -- visible (g is
    good, f is good, another star), m, drift, dt, period_match, match."""
    f = numpy.asarray(rows)[:, None]
    g = numpy.arange(len(period))[None, :]
    ok = good(period, T0, duration, strength)
    visible = ok[f] & ok[g] & (star[f] != star[g]) & (f != g)
    with numpy.errstate(all="ignore"):
        f_long = period[f] >= period[g]
        Pl = numpy.where(f_long, period[f], period[g])
        Ps = numpy.where(f_long, period[g], period[f])
        T0l = numpy.where(f_long, T0[f], T0[g])
        T0s = numpy.where(f_long, T0[g], T0[f])
        m = numpy.rint(Pl / Ps)
        e = m * Ps
        dP = numpy.fabs(Pl - e)
        c = span / Pl
        drift = dP * c
        dmax = numpy.fmax(duration[f], duration[g])
        plim = drift_tolerance * dmax
        elim = epoch_tolerance * dmax
        period_match = visible & (m <= max_ratio) & (drift <= plim)
        x = (T0l - T0s) / Ps
        r = numpy.rint(x)
        u = x - r
        dt = numpy.fabs(u) * Ps
        match = period_match & (dt <= elim)
    return dict(visible=visible, m=m, drift=drift, dt=dt, period_match=period_match, match=match)


def arrays(star, period, T0, duration, strength):
    star = numpy.ascontiguousarray(star, dtype=numpy.int64)
    period, T0, duration, strength = (numpy.ascontiguousarray(v, dtype=numpy.float64) for v in (period, T0, duration, strength))
    assert star.ndim == 1 and star.shape == period.shape == T0.shape == duration.shape == strength.shape
    return star, period, T0, duration, strength


def match(star, period, T0, duration, strength, span, drift_tolerance=0.5, epoch_tolerance=0.5, max_ratio=3):
    """The records [M] (DTYPE) of the statement above."""
    star, period, T0, duration, strength = arrays(star, period, T0, duration, strength)
    span, drift_tolerance, epoch_tolerance, max_ratio = float(span), float(drift_tolerance), float(epoch_tolerance), float(max_ratio)
    M = len(period)
    out = numpy.zeros(M, dtype=DTYPE)
    ok = good(period, T0, duration, strength)
    for lo in range(0, M, ROWS):
        rows = numpy.arange(lo, min(M, lo + ROWS))
        p = pairs(star, period, T0, duration, strength, span, drift_tolerance, epoch_tolerance, max_ratio, rows)
        rec = out[lo:lo + ROWS]
        rec["n_same"] = numpy.sum(p["period_match"] & (p["m"] == 1), axis=1)
        rec["n_period"] = numpy.sum(p["period_match"], axis=1)
        rec["n_match"] = numpy.sum(p["match"], axis=1)
        # the largest strength among the matches, the lowest index among equals (argmax takes the first)
        best = numpy.argmax(numpy.where(p["match"], strength[None, :], -numpy.inf), axis=1)
        found = rec["n_match"] > 0
        at = (numpy.arange(len(rows)), best)
        rec["best"] = numpy.where(found, best, -1)
        rec["best_ratio"] = numpy.where(found, numpy.where(period[best] >= period[rows], p["m"][at], -p["m"][at]), numpy.nan)
        rec["best_dt"] = numpy.where(found, p["dt"][at], numpy.nan)
        rec["best_drift"] = numpy.where(found, p["drift"][at], numpy.nan)
        rec["best_strength"] = numpy.where(found, strength[best], numpy.nan)
        rec["child"] = numpy.where(found, (strength[best] > strength[rows]).astype(numpy.float64), numpy.nan)
    for k in FIELDS[1:]:
        out[k][~ok] = numpy.nan
    out["status"] = numpy.where(ok, MATCHED, BAD)
    return out


def relation(star, period, T0, duration, strength, span, drift_tolerance=0.5, epoch_tolerance=0.5, max_ratio=3):
    """(period_match, match), each [M, M]: the two relations themselves, for small M."""
    star, period, T0, duration, strength = arrays(star, period, T0, duration, strength)
    p = pairs(star, period, T0, duration, strength, float(span), float(drift_tolerance), float(epoch_tolerance), float(max_ratio),
              numpy.arange(len(period)))
    return p["period_match"], p["match"]


def groups(records):
    """Every candidate's root: follow `best` while child == 1 (strength rises strictly along the chain, so it ends); itself
    where it has no stronger match."""
    root = numpy.arange(len(records))
    for f in range(len(records)):
        at = f
        while records["child"][at] == 1:
            at = int(records["best"][at])
        root[f] = at
    return root


# ---- the statement by hand: dyadic numbers, so that every comparison below is exact -----------------------------------------
NAN = float("nan")
ULP = 2.0 ** -53


def _expected(rows):
    out = numpy.zeros(len(rows), dtype=DTYPE)
    for f, row in enumerate(rows):
        out[f] = (BAD,) + (NAN,) * 9 if row is None else (MATCHED,) + tuple(row)
    return out


def _nothing():
    return (0, 0, 0, -1, NAN, NAN, NAN, NAN, NAN)


def by_hand():
    """[(name, arguments of match(), the records worked out by hand)]: span 32 and duration 0.25 throughout, so that with
    the default tolerances plim = elim = 0.125."""
    cases = []
    d4 = [0.25] * 4
    # P = 2, 4, 5, 7: 4 / 2 = 2 matches; 5 / 2 = 2.5 -> m = 2, dP = 1, drift = 32 / 5; 7 / 2 = 3.5 -> m = 4 > 3;
    # 5 / 4 -> 1, 7 / 4 -> 2, 7 / 5 -> 1, all with dP >= 1
    ratios = dict(star=[0, 1, 2, 3], period=[2.0, 4.0, 5.0, 7.0], T0=[1.0] * 4, duration=d4, strength=[4.0, 3.0, 2.0, 1.0], span=32.0)
    cases.append(("ratios", dict(ratios), _expected([
        (0, 1, 1, 1, 2.0, 0.0, 0.0, 3.0, 0), (0, 1, 1, 0, -2.0, 0.0, 0.0, 4.0, 1), _nothing(), _nothing()])))
    # the same with plim = 64 * 0.25 = 16: every drift passes, and rint's halves show in the ratios (2.5 -> 2)
    cases.append(("halves", dict(ratios, drift_tolerance=64.0), _expected([
        (0, 2, 2, 1, 2.0, 0.0, 0.0, 3.0, 0),
        (1, 3, 3, 0, -2.0, 0.0, 0.0, 4.0, 1),
        (2, 3, 3, 0, -2.0, 0.0, 32.0 / 5.0, 4.0, 1),
        (1, 2, 2, 1, -2.0, 0.0, 32.0 / 7.0, 3.0, 1)])))
    # ... and with max_ratio = 4: 3.5 -> 4 (half to even), so 2 and 7 match as well
    cases.append(("halves, max_ratio 4", dict(ratios, drift_tolerance=64.0, max_ratio=4), _expected([
        (0, 3, 3, 1, 2.0, 0.0, 0.0, 3.0, 0),
        (1, 3, 3, 0, -2.0, 0.0, 0.0, 4.0, 1),
        (2, 3, 3, 0, -2.0, 0.0, 32.0 / 5.0, 4.0, 1),
        (1, 3, 3, 0, -4.0, 0.0, 32.0 / 7.0, 4.0, 1)])))
    # drift exactly at plim: P = 4 and 4 - 1/64: m = 1, dP = 1/64, c = 8, drift = 0.125; one ulp of the shorter period below
    # that dP = 1/64 + 2^-51 and drift > plim.  Candidates 1 and 2 are ONE star: never matched with each other.
    short = 4.0 - 1.0 / 64
    cases.append(("drift edge", dict(star=[0, 1, 1], period=[4.0, short, numpy.nextafter(short, 0.0)], T0=[1.0] * 3,
                                     duration=[0.25] * 3, strength=[3.0, 2.0, 1.0], span=32.0), _expected([
        (1, 1, 1, 1, -1.0, 0.0, 0.125, 2.0, 0), (1, 1, 1, 0, 1.0, 0.0, 0.125, 3.0, 1), _nothing()])))
    # dt exactly at elim: P = 4 and 2, T0 = 1.125 and 1: x = 0.0625, dt = 0.125; against T0 = 1 - 2^-53, dt = 0.125 + 2^-53.
    # Candidates 1 and 2 have EQUAL periods: x = +-2^-54 by the order, dt = 2^-53 either way.
    cases.append(("epoch edge", dict(star=[0, 1, 2], period=[4.0, 2.0, 2.0], T0=[1.125, 1.0, 1.0 - ULP], duration=[0.25] * 3,
                                     strength=[1.0, 3.0, 2.0], span=32.0), _expected([
        (0, 2, 1, 1, -2.0, 0.125, 0.0, 3.0, 1), (1, 2, 2, 2, 1.0, ULP, 0.0, 2.0, 0), (1, 2, 1, 1, 1.0, ULP, 0.0, 3.0, 1)])))
    # m == max_ratio (6 / 2) and max_ratio + 1 (8 / 2); 8 / 6 -> 1 with dP = 2
    cases.append(("max_ratio", dict(star=[0, 1, 2], period=[2.0, 6.0, 8.0], T0=[1.0] * 3, duration=[0.25] * 3,
                                    strength=[1.0, 2.0, 3.0], span=32.0), _expected([
        (0, 1, 1, 1, 3.0, 0.0, 0.0, 2.0, 1), (0, 1, 1, 0, -3.0, 0.0, 0.0, 1.0, 0), _nothing()])))
    # equal strengths: the lowest index wins
    cases.append(("ties", dict(star=[0, 1, 2, 3], period=[4.0] * 4, T0=[1.0] * 4, duration=d4, strength=[1.0, 2.0, 2.0, 1.0],
                               span=32.0), _expected([
        (3, 3, 3, 1, 1.0, 0.0, 0.0, 2.0, 1), (3, 3, 3, 2, 1.0, 0.0, 0.0, 2.0, 0), (3, 3, 3, 1, 1.0, 0.0, 0.0, 2.0, 0),
        (3, 3, 3, 1, 1.0, 0.0, 0.0, 2.0, 1)])))
    # a bad candidate of each kind between two good ones: each would match both if it were seen
    bad = [("period", NAN), ("period", numpy.inf), ("period", 0.0), ("period", -4.0), ("T0", NAN), ("T0", -numpy.inf),
           ("duration", 0.0), ("duration", -0.25), ("duration", NAN), ("duration", numpy.inf), ("strength", NAN),
           ("strength", numpy.inf)]
    n = len(bad) + 2
    c = dict(star=list(range(n)), period=[4.0] * n, T0=[1.0] * n, duration=[0.25] * n, strength=[2.0] + [9.0] * len(bad) + [1.0],
             span=32.0)
    for i, (name, value) in enumerate(bad):
        c[name][i + 1] = value
    cases.append(("bad candidates", c, _expected(
        [(1, 1, 1, n - 1, 1.0, 0.0, 0.0, 1.0, 0)] + [None] * len(bad) + [(1, 1, 1, 0, 1.0, 0.0, 0.0, 2.0, 1)])))
    return cases


# ---- candidates for the tests ---------------------------------------------------------------------------------------------
def clustered(seed, n, n_stars=None, bases=24):
    """n candidates that match one another often: periods and epochs from a few bases with jitter of the order of the
    tolerances, ratios 1, 2 and 3 mixed in."""
    rng = numpy.random.RandomState(seed)
    base_P = rng.uniform(1.0, 6.0, bases)
    base_E = rng.uniform(0.0, 1.0, bases)
    pick = rng.randint(0, bases, n)
    period = base_P[pick] * rng.choice([1.0, 1.0, 2.0, 3.0], n) * (1 + 4e-4 * rng.uniform(-1, 1, n))
    T0 = base_E[pick] + base_P[pick] * rng.randint(0, 4, n) + 0.08 * rng.uniform(-1, 1, n)
    duration = rng.uniform(0.05, 0.2, n)
    strength = numpy.round(rng.uniform(0.0, 1.0, n), 2)        # (equal strengths occur)
    star = rng.randint(0, n_stars or max(2, n // 4), n)
    return star, period, T0, duration, strength, 80.0


def field(seed, n=40, span=80.0):
    """n stars with independent random ephemerides; three of them (`members`, the strongest first) are given ONE ephemeris
    with grid-sized errors -- relative period error 2e-4, epoch error 0.01 d -- the third at twice the period."""
    rng = numpy.random.RandomState(seed)
    period = rng.uniform(1.0, 20.0, n)
    T0 = rng.uniform(0.0, 1.0, n) * period
    duration = rng.uniform(0.06, 0.25, n)
    strength = rng.uniform(2e-4, 5e-3, n)
    members = rng.choice(n, 3, replace=False)
    P, E = 3.0 + 4.0 * rng.uniform(), 2.0 * rng.uniform()
    err = 2e-4 * rng.uniform(-1, 1, 3)
    shift = 0.01 * rng.uniform(-1, 1, 3)
    for k, f in enumerate(members):
        period[f] = (2.0 if k == 2 else 1.0) * P * (1 + err[k])
        T0[f] = E + shift[k] + (P if k == 2 else 0.0)          # (the one at 2 P has caught every other eclipse)
        duration[f] = 0.15
    strength[members] = [0.05, 0.004, 0.002]
    return (numpy.arange(n), period, T0, duration, strength, span), members
