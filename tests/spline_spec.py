"""Robust B-spline detrending as tls_spline_detrend states it (include/tls_amd.h), restated in Python for test_spline_host.py
and test_spline.py: `loops` in plain Python floats, one IEEE double operation a line, and `fit`, the same steps with numpy over
the points.  Every sum runs in ascending index from +0.0, so the two forms and the device agree bit for bit; the one function
that may differ on the device by an ulp is the log of the BIC.

Inputs: t [n] finite and non-decreasing; y [R, n] > 0; dy [R, n] or None (w = 1.0 / (dy * dy), else 1.0); mask [R, n] or None
(!= 0: protected); spacings [S], S in [1, MAX_SPACINGS].  A new segment starts behind every gap t[j] - t[j-1] > break_tolerance.

A (curve, segment, spacing), the segment's points a .. b, L = b - a + 1 of them, T = t[b] - t[a]:
  knots   T == 0: q = 0, m = 0 (no spline: status 1).  Else q = max(1, ceil(T / spacing)), h = T / q, m = q + 3.
  place   x = (t[i] - t[a]) / h;  j = min(int(x), q - 1);  u = x - j
  basis   u2 = u * u;  u3 = u2 * u;  o = 1.0 - u;  o2 = o * o;  o3 = o2 * o
          b0 = o3 / 6.0;  b1 = ((3.0 * u3 - 6.0 * u2) + 4.0) / 6.0;  b2 = (((-(3.0 * u3) + 3.0 * u2) + 3.0 * u) + 1.0) / 6.0
          b3 = u3 / 6.0;  point i touches the coefficients j .. j + 3
  F       the members: at first the unprotected points;  rounds = dropped = 0;  sigma = NaN
  fit:    nF = |F|;  nF == 0, or the last member's time stamp is not > the first one's: status 1, leave the loop
     A    W = sum_F w
          interval j, its members in ascending index, from +0.0:  wb_k = w * b_k;  S_j[k][l] += wb_k * b_l (k <= l);  R_j[k] += wb_k * y
          band entry A[c][c + d] (d = 0 .. 3, c + d < m) = 0.0 + the S_j[c - j][c + d - j] of j = max(0, c + d - 3) .. min(c, q - 1), j ascending
          g[c] = 0.0 + the R_j[c - j] of j = max(0, c - 3) .. min(c, q - 1), j ascending
          pw = W / q;  lam = penalty * pw;  A[c][c + d] = A[c][c + d] + lam * P[c][c + d] for d = 0 .. 2, P = D2^T D2 (whole numbers)
     B    Cholesky inside the band, j ascending:  s = A[j][j];  for k = max(0, j - 3) .. j - 1:  s = s - L[j][k] * L[j][k]
              not (s > PIVOT * A[j][j]): status 2, leave the loop;  L[j][j] = sqrt(s)
              for i = j + 1 .. min(j + 3, m - 1):  v = A[j][i];  for k = max(0, i - 3) .. j - 1:  v = v - L[i][k] * L[j][k];  L[i][j] = v / L[j][j]
          forward, j ascending:  s = g[j];  for k = max(0, j - 3) .. j - 1:  s = s - L[j][k] * z[k];  z[j] = s / L[j][j]
          back, j descending:    s = z[j];  for k = j + 1 .. min(j + 3, m - 1):  s = s - L[k][j] * c[k];  c[j] = s / L[j][j]
     C    trend at EVERY point of the segment:  p = c[j] * b0;  p = p + c[j+1] * b1;  p = p + c[j+2] * b2;  p = p + c[j+3] * b3
          a trend value not in (0, inf): status 2, leave the loop.  Else status 0.
  clip    rounds == n_iter: leave.  r = y - trend over F;  med = median(r);  sigma = 1.4826 * median(|r - med|)  (numpy.median)
          sigma == 0: leave.  up = sigma_upper * sigma;  down = -(sigma_lower * sigma);  out = the members with r > up or r < down
          rounds = rounds + 1;  nobody out: leave;  nF - |out| < 2: leave (the round is not applied)
          F = F without out;  dropped = dropped + |out|;  fit again
  status 1 or 2:  trend = mu = (sum w * y) / (sum w) over F, over all the points of the segment where F is empty
  flat = y / trend at every point;  weight = sum_F w (0.0 for no member);  r = y - trend;  ssr = sum_F (w * r) * r

The choice, for every curve where S > 1 (S == 1: the same record, choice 0):
  d = y[i+1] - y[i] of the neighbours i, i + 1 of one segment that are both unprotected;  none: sigma_pp = NaN
  sigma_pp = (1.4826 * median(|d - median(d)|)) / sqrt(2)
  spacing s, over its segments of status 0 in order, from 0:  K = sum m;  N = sum kept;  Q = sum ssr;  V = sum weight
  BIC_s = K * log(N) + (Q / (V / N)) / (sigma_pp * sigma_pp)
  the first index of the least finite BIC wins;  sigma_pp not > 0 or no BIC finite: the first spacing, flag = 1
  flat, trend and the segment records are those of the chosen spacing.

A segment record: SEGMENT_FIELDS, all doubles.  A curve record: CURVE_FIELDS, then the MAX_SPACINGS BIC values (NaN behind S)."""
import math

import numpy

MAX_SPACINGS = 16
MAX_ITER = 16
MAX_COEF = 512
LDS_POINTS = 5120
PIVOT = 1e-10
MAD_K = 1.4826
ROOT2 = 1.4142135623730951
SEGMENT_FIELDS = ("status", "intervals", "coefficients", "points", "kept", "rounds", "dropped", "sigma", "ssr", "weight")
CURVE_FIELDS = ("choice", "sigma_pp", "flag")
PAIR = ((0, 1, 2, 3), (None, 4, 5, 6), (None, None, 7, 8), (None, None, None, 9))     # S_j[k][l] in an interval's ten sums
D2 = (1.0, -2.0, 1.0)


def segment_starts(t, break_tolerance):
    """[0, ..., n]: a new segment starts behind every gap t[j] - t[j-1] > break_tolerance."""
    t = numpy.asarray(t, dtype=numpy.float64)
    return [0] + [int(j) + 1 for j in numpy.flatnonzero(t[1:] - t[:-1] > break_tolerance)] + [len(t)]


def knots(T, spacing):
    """(q, h) of a segment of span T."""
    if T == 0.0:
        return 0, float("nan")
    q = max(1, int(math.ceil(T / spacing)))
    return q, T / q


def basis(u):
    """The four uniform cubic B-spline values at u (a float or an array): the operations in the stated order."""
    u2 = u * u
    u3 = u2 * u
    o = 1.0 - u
    o2 = o * o
    o3 = o2 * o
    b0 = o3 / 6.0
    b1 = ((3.0 * u3 - 6.0 * u2) + 4.0) / 6.0
    b2 = (((-(3.0 * u3) + 3.0 * u2) + 3.0 * u) + 1.0) / 6.0
    b3 = u3 / 6.0
    return b0, b1, b2, b3


def penalty_entry(c, d, m):
    """(D2^T D2)[c][c + d] of m coefficients: a whole number."""
    p = 0.0
    for r in range(max(0, c + d - 2), min(c, m - 3) + 1):
        p += D2[c - r] * D2[c + d - r]
    return p


def assemble(S, q, W, penalty):
    """Step A behind the interval sums S [q][14]: (band [m][4], g [m])."""
    m = q + 3
    band = [[0.0] * 4 for _ in range(m)]
    g = [0.0] * m
    for c in range(m):
        for d in range(4):
            if c + d < m:
                s = 0.0
                for j in range(max(0, c + d - 3), min(c, q - 1) + 1):
                    s = s + S[j][PAIR[c - j][c + d - j]]
                band[c][d] = s
        s = 0.0
        for j in range(max(0, c - 3), min(c, q - 1) + 1):
            s = s + S[j][10 + c - j]
        g[c] = s
    pw = W / float(q)
    lam = penalty * pw
    for c in range(m):
        for d in range(3):
            if c + d < m:
                band[c][d] = band[c][d] + lam * penalty_entry(c, d, m)
    return band, g


def solve(band, g):
    """Step B: the coefficients, or None where a pivot fails.  band[c][d] = A[c][c + d]; L[i][j] replaces A[j][i] in place."""
    m = len(g)
    A = [row[:] for row in band]
    for j in range(m):
        ajj = A[j][0]
        s = ajj
        for k in range(max(0, j - 3), j):
            s = s - A[k][j - k] * A[k][j - k]
        if not (s > PIVOT * ajj):
            return None
        ljj = math.sqrt(s)
        A[j][0] = ljj
        for i in range(j + 1, min(j + 3, m - 1) + 1):
            v = A[j][i - j]
            for k in range(max(0, i - 3), j):
                v = v - A[k][i - k] * A[k][j - k]
            A[j][i - j] = v / ljj
    z = [0.0] * m
    for j in range(m):
        s = g[j]
        for k in range(max(0, j - 3), j):
            s = s - A[k][j - k] * z[k]
        z[j] = s / A[j][0]
    c = [0.0] * m
    for j in range(m - 1, -1, -1):
        s = z[j]
        for k in range(j + 1, min(j + 3, m - 1) + 1):
            s = s - A[j][k - j] * c[k]
        c[j] = s / A[j][0]
    return c


def _median(v):
    """numpy.median of a list of floats: the middle one, or the mean of the two middle ones."""
    s = sorted(v)
    k = len(s)
    return s[k // 2] if k % 2 else (s[k // 2 - 1] + s[k // 2]) / 2.0


def _div(a, b):
    with numpy.errstate(all="ignore"):
        return float(numpy.float64(a) / numpy.float64(b))


# ---- the plain form ---------------------------------------------------------------------------------------------------------
class Loops(object):
    """The point-wise steps on lists."""

    @staticmethod
    def place(tt, q, h):
        out = []
        for v in tt:
            x = (v - tt[0]) / h
            j = min(int(x), q - 1)
            out.append((j, x - j))
        return out

    @staticmethod
    def osum(v, member):
        s = 0.0
        for x, inside in zip(v, member):
            if inside:
                s = s + x
        return s

    @staticmethod
    def interval_sums(at, y, w, F, q):
        S = [[0.0] * 14 for _ in range(q)]
        for i in range(len(y)):
            if F[i]:
                j, u = at[i]
                b = basis(u)
                for k in range(4):
                    wb = w[i] * b[k]
                    for l in range(k, 4):
                        S[j][PAIR[k][l]] = S[j][PAIR[k][l]] + wb * b[l]
                    S[j][10 + k] = S[j][10 + k] + wb * y[i]
        return S

    @staticmethod
    def evaluate(at, c):
        out = []
        for j, u in at:
            b = basis(u)
            p = c[j] * b[0]
            p = p + c[j + 1] * b[1]
            p = p + c[j + 2] * b[2]
            p = p + c[j + 3] * b[3]
            out.append(p)
        return out

    @staticmethod
    def good(trend):
        return all(0.0 < v < math.inf for v in trend)

    @staticmethod
    def robust_sigma(y, trend, F):
        r = [a - b for a, b in zip(y, trend)]
        inside = [x for x, f in zip(r, F) if f]
        med = _median(inside)
        return r, MAD_K * _median([abs(x - med) for x in inside])

    @staticmethod
    def outside(r, F, up, down):
        return [f and (x > up or x < down) for x, f in zip(r, F)]

    @staticmethod
    def without(F, out):
        return [f and not o for f, o in zip(F, out)]

    @staticmethod
    def finish(y, w, trend, F):
        flat = [_div(a, b) for a, b in zip(y, trend)]
        s = 0.0
        for a, b, x, f in zip(y, trend, w, F):
            if f:
                r = a - b
                s = s + (x * r) * r
        return flat, s

    @staticmethod
    def products(w, y):
        return [a * b for a, b in zip(w, y)]

    @staticmethod
    def constant(mu, L):
        return [mu] * L


# ---- the numpy form ---------------------------------------------------------------------------------------------------------
class Arrays(object):
    """The same steps over the points at once."""

    @staticmethod
    def place(tt, q, h):
        x = (tt - tt[0]) / h
        j = numpy.minimum(x.astype(numpy.int64), q - 1)
        return j, x - j

    @staticmethod
    def osum(v, member):
        v = numpy.where(member, v, 0.0)                     # (a sum that starts at +0.0 never holds -0.0: + 0.0 changes no bit)
        return float(numpy.cumsum(numpy.concatenate([[0.0], v]))[-1])

    @staticmethod
    def interval_sums(at, y, w, F, q):
        j, u = at
        b = basis(u)
        rows = []
        for k in range(4):
            wb = w * b[k]
            rows.extend(wb * b[l] for l in range(k, 4))
        for k in range(4):
            rows.append((w * b[k]) * y)
        rows = numpy.where(F[None, :], numpy.array(rows), 0.0)
        lo, hi = numpy.searchsorted(j, numpy.arange(q), "left"), numpy.searchsorted(j, numpy.arange(q), "right")
        S = []
        for a, e in zip(lo, hi):
            part = numpy.concatenate([numpy.zeros((14, 1)), rows[:, a:e]], axis=1)
            S.append(numpy.cumsum(part, axis=1)[:, -1].tolist())
        return S

    @staticmethod
    def evaluate(at, c):
        j, u = at
        c = numpy.asarray(c)
        b = basis(u)
        p = c[j] * b[0]
        p = p + c[j + 1] * b[1]
        p = p + c[j + 2] * b[2]
        p = p + c[j + 3] * b[3]
        return p

    @staticmethod
    def good(trend):
        return bool(numpy.all((trend > 0.0) & (trend < numpy.inf)))

    @staticmethod
    def robust_sigma(y, trend, F):
        r = y - trend
        med = numpy.median(r[F])
        return r, float(MAD_K * numpy.median(numpy.abs(r[F] - med)))

    @staticmethod
    def outside(r, F, up, down):
        return F & ((r > up) | (r < down))

    @staticmethod
    def without(F, out):
        return F & ~out

    @staticmethod
    def finish(y, w, trend, F):
        with numpy.errstate(all="ignore"):
            flat = y / trend
        r = y - trend
        return flat, Arrays.osum((w * r) * r, F)

    @staticmethod
    def products(w, y):
        return w * y

    @staticmethod
    def constant(mu, L):
        return numpy.full(L, mu)


def _segment(ops, tt, y, w, open_, spacing, penalty, n_iter, up_k, down_k):
    """One (curve, segment, spacing): (flat, trend, record)."""
    L = len(y)
    q, h = knots(float(tt[-1]) - float(tt[0]), spacing)
    m = q + 3 if q else 0
    at = ops.place(tt, q, h) if q else None
    F = open_
    rounds = dropped = 0
    sigma = float("nan")
    trend = None
    while True:
        where = numpy.flatnonzero(F)
        nF = len(where)
        if nF == 0 or not (tt[where[-1]] > tt[where[0]]):
            status = 1
            break
        W = ops.osum(w, F)
        band, g = assemble(ops.interval_sums(at, y, w, F, q), q, W, penalty)
        c = solve(band, g)
        if c is None:
            status = 2
            break
        trend = ops.evaluate(at, c)
        if not ops.good(trend):
            status = 2
            break
        status = 0
        if rounds == n_iter:
            break
        r, sigma = ops.robust_sigma(y, trend, F)
        if sigma == 0.0:
            break
        up = up_k * sigma
        down = -(down_k * sigma)
        out = ops.outside(r, F, up, down)
        left = int(sum(out))
        rounds += 1
        if left == 0 or nF - left < 2:
            break
        F = ops.without(F, out)
        dropped += left
    if status != 0:
        member = F if nF else [True] * L
        mu = _div(ops.osum(ops.products(w, y), member), ops.osum(w, member))
        trend = ops.constant(mu, L)
    flat, ssr = ops.finish(y, w, trend, F)
    weight = ops.osum(w, F) if nF else 0.0
    record = (float(status), float(q), float(m), float(L), float(nF), float(rounds), float(dropped), sigma, ssr, weight)
    return flat, trend, record


def sigma_pp(y, open_, starts):
    """The point-to-point sigma of a curve (NaN without a pair)."""
    d = []
    for a, b in zip(starts[:-1], starts[1:]):
        for i in range(a, b - 1):
            if open_[i] and open_[i + 1]:
                d.append(float(y[i + 1]) - float(y[i]))
    if not d:
        return float("nan")
    med = _median(d)
    return (MAD_K * _median([abs(x - med) for x in d])) / ROOT2


def bic(records, sigma):
    """BIC of one spacing from its segment records [G, len(SEGMENT_FIELDS)]."""
    K = N = 0
    Q = V = 0.0
    for rec in records:
        if rec[0] == 0.0:
            K += int(rec[2])
            N += int(rec[4])
            Q = Q + float(rec[8])
            V = V + float(rec[9])
    with numpy.errstate(all="ignore"):
        lg = numpy.float64(math.log(N)) if N > 0 else numpy.float64(-numpy.inf)
        return float(numpy.float64(K) * lg + (numpy.float64(Q) / (numpy.float64(V) / numpy.float64(N))) / (numpy.float64(sigma) * numpy.float64(sigma)))


def _run(ops, t, y, dy, mask, spacings, break_tolerance, penalty, n_iter, sigma_upper, sigma_lower, as_lists):
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    if y.ndim == 1:
        y = y[None, :]
    R, n = y.shape
    spacings = [float(s) for s in numpy.atleast_1d(spacings)]
    S = len(spacings)
    assert 1 <= S <= MAX_SPACINGS and 0 <= int(n_iter) <= MAX_ITER
    starts = segment_starts(t, break_tolerance)
    G = len(starts) - 1
    with numpy.errstate(all="ignore"):
        w = numpy.ones((R, n)) if dy is None else 1.0 / (numpy.asarray(dy, dtype=numpy.float64).reshape(R, n) * numpy.asarray(dy, dtype=numpy.float64).reshape(R, n))
    open_ = numpy.ones((R, n), dtype=bool) if mask is None else numpy.asarray(mask).reshape(R, n) == 0
    flat, trend = numpy.empty((R, n)), numpy.empty((R, n))
    segment = numpy.zeros((R, G, len(SEGMENT_FIELDS)))
    curve = numpy.full((R, len(CURVE_FIELDS) + MAX_SPACINGS), numpy.nan)
    for i in range(R):
        tried = []
        for s in range(S):
            parts = []
            for a, b in zip(starts[:-1], starts[1:]):
                args = (t[a:b], y[i, a:b], w[i, a:b], open_[i, a:b])
                if as_lists:
                    args = tuple(v.tolist() for v in args)
                parts.append(_segment(ops, *args, spacings[s], float(penalty), int(n_iter), float(sigma_upper), float(sigma_lower)))
            tried.append(parts)
        pp = sigma_pp(y[i], open_[i], starts)
        values = [bic([p[2] for p in parts], pp) for parts in tried]
        finite = [k for k in range(S) if math.isfinite(values[k])]
        if pp > 0.0 and finite:
            choice, flag = min(finite, key=lambda k: (values[k], k)), 0.0
        else:
            choice, flag = 0, 1.0
        curve[i, :3] = (float(choice), pp, flag)
        curve[i, 3:3 + S] = values
        for k, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
            flat[i, a:b], trend[i, a:b], segment[i, k] = tried[choice][k]
    return {"flat": flat, "trend": trend, "segment": segment, "curve": curve, "starts": starts}


def loops(t, y, dy=None, mask=None, knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0):
    """The statement in plain Python floats: a dict with flat, trend [R, n], segment [R, G, len(SEGMENT_FIELDS)], curve
    [R, len(CURVE_FIELDS) + MAX_SPACINGS] and starts [G + 1]."""
    return _run(Loops, t, y, dy, mask, knot_spacing, break_tolerance, penalty, n_iter, sigma_upper, sigma_lower, True)


def fit(t, y, dy=None, mask=None, knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0):
    """The same statement with numpy over the points: equal to `loops` bit for bit."""
    return _run(Arrays, t, y, dy, mask, knot_spacing, break_tolerance, penalty, n_iter, sigma_upper, sigma_lower, False)


def normal_matrix(t, y, dy=None, knot_spacing=0.75, penalty=0.0):
    """The dense normal matrix and right-hand side of the statement's first fit of one gap-free, unmasked row (for the tests'
    condition number)."""
    t, y = numpy.asarray(t, dtype=numpy.float64), numpy.asarray(y, dtype=numpy.float64)
    w = numpy.ones(len(y)) if dy is None else 1.0 / (numpy.asarray(dy, dtype=numpy.float64) * numpy.asarray(dy, dtype=numpy.float64))
    q, h = knots(float(t[-1] - t[0]), float(knot_spacing))
    F = numpy.ones(len(y), dtype=bool)
    at = Arrays.place(t, q, h)
    band, g = assemble(Arrays.interval_sums(at, y, w, F, q), q, Arrays.osum(w, F), float(penalty))
    m = q + 3
    A = numpy.zeros((m, m))
    for c in range(m):
        for d in range(4):
            if c + d < m:
                A[c, c + d] = A[c + d, c] = band[c][d]
    return A, numpy.array(g), q, h
