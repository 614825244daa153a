"""Regression detrending as tls_decorrelate states it (include/tls_amd.h), restated in Python for test_decorrelate_host.py and
test_decorrelate.py: `loops` in plain Python floats, one IEEE double operation a line, and `fit`, the same steps with numpy
over the points and the columns.  Every sum runs over the points in ascending index from +0.0, a point outside F adding
+0.0, so the two forms and the device agree bit for bit.

Inputs: y [R, n]; dy [R, n] or None (w = 1 / (dy * dy), else 1.0); mask [R, n] or None (!= 0: protected); shared [n_shared, n];
own [R, n_own, n]; segments [S + 1] strictly ascending from 0 to n.  The columns of a curve are the shared ones, then its own:
m = n_shared + n_own in [1, MAX_TERMS].  Every (curve, segment) is fitted on its own; F starts as the segment's unprotected
points; clip rounds run = 0.

  fit:  nF = |F|
     A  W = sum_F w * 1.0;  Sy = sum_F w * y;  Sk = sum_F w * x_k                  (F empty: status 1, see below)
        mu = Sy / W;  mean_k = Sk / W
     B  d = x_k - mean_k;  Vk = sum_F (w * d) * d;  scale_k = sqrt(Vk / W)
        column k is live if 0 < scale_k < inf, else dropped (bit k)
        nF < live + 2: status 1
     C  z = y / mu - 1.0;  u_k = (x_k - mean_k) / scale_k (live), 0.0 (dropped)
        G_kl = sum_F (w * u_k) * u_l  for l <= k;  G_kk = G_kk + ridge * W;  b_k = sum_F (w * u_k) * z
     D  cholesky, j ascending over the live columns:
            s = G_jj;  for k < j live, ascending:  s = s - L_jk * L_jk
            not (s > PIVOT * G_jj): column j is dropped (bit j) and no longer live;  else L_jj = sqrt(s)
            for i > j live, ascending:  q = G_ij;  for k < j live, ascending:  q = q - L_ik * L_jk;  L_ij = q / L_jj
        forward, j ascending live:   s = b_j;  for k < j live, ascending:  s = s - L_jk * v_k;  v_j = s / L_jj
        back, j descending live:     s = v_j;  for k > j live, ascending:  s = s - L_kj * c_k;  c_j = s / L_jj
        c_k = 0.0 for a dropped column
     E  p = 0.0;  for k live, ascending:  p = p + c_k * u_k;  r = z - p
        Q = sum_F (w * r) * r;  sigma = sqrt(Q / W)
  clip (only while rounds < n_iter):  up = sigma_upper * sigma;  down = -(sigma_lower * sigma)
        a member of F leaves if r > up or r < down;  rounds = rounds + 1;  if any left: fit again
  status 1 (F holds fewer than live + 2 points, at any fit): every coefficient 0.0, no column live or dropped, mean_k = 0.0,
        scale_k = 1.0, sigma = NaN; mu = Sy / W of F, or of the whole segment where F is empty
  trend = mu * (1.0 + p);  flat = y / trend at every point of the segment
  status 2 (a trend value of the segment is not finite or not > 0): trend = mu, flat = y / mu; the rest of the record stays

The record of a (curve, segment), all doubles: FIELDS."""
import math

import numpy

MAX_TERMS = 16
MAX_ITER = 16
PIVOT = 1e-10
LDS_POINTS = 32768
FIELDS = ("status", "dropped", "n_fit", "n_clipped", "rounds", "mu", "sigma", "n_live")


# ---- the plain form ---------------------------------------------------------------------------------------------------------
def _cholesky_solve(G, b, live, m):
    """Step D on lists: (c, live, dropped bits)."""
    L = [[0.0] * m for _ in range(m)]
    live = list(live)
    bits = 0
    for j in range(m):
        if not live[j]:
            continue
        s = G[j][j]
        for k in range(j):
            if live[k]:
                s = s - L[j][k] * L[j][k]
        if not (s > PIVOT * G[j][j]):
            live[j] = False
            bits |= 1 << j
            continue
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, m):
            if live[i]:
                q = G[i][j]
                for k in range(j):
                    if live[k]:
                        q = q - L[i][k] * L[j][k]
                L[i][j] = q / L[j][j]
    v = [0.0] * m
    for j in range(m):
        if live[j]:
            s = b[j]
            for k in range(j):
                if live[k]:
                    s = s - L[j][k] * v[k]
            v[j] = s / L[j][j]
    c = [0.0] * m
    for j in range(m - 1, -1, -1):
        if live[j]:
            s = v[j]
            for k in range(j + 1, m):
                if live[k]:
                    s = s - L[k][j] * c[k]
            c[j] = s / L[j][j]
    return c, live, bits


def _div(a, b):
    """a / b as IEEE states it (Python raises where the divisor is 0)."""
    with numpy.errstate(all="ignore"):
        return float(numpy.float64(a) / numpy.float64(b))


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else float("nan")


def _segment_loops(y, w, open_, X, ridge, n_iter, up_k, down_k):
    """One (curve, segment): y, w [L] floats, open_ [L] bools, X [m][L]."""
    L, m = len(y), len(X)
    F = list(open_)
    rounds = n_clipped = 0
    while True:
        nF = sum(F)
        everyone = nF == 0
        W = Sy = 0.0
        S = [0.0] * m
        for j in range(L):
            if F[j] or everyone:
                W = W + w[j] * 1.0
                Sy = Sy + w[j] * y[j]
                for k in range(m):
                    S[k] = S[k] + w[j] * X[k][j]
        mu = _div(Sy, W)
        status, bits, sigma = 0, 0, float("nan")
        c, mean, scale, live = [0.0] * m, [0.0] * m, [1.0] * m, [False] * m
        if everyone:
            status = 1
        else:
            mean = [_div(S[k], W) for k in range(m)]
            for k in range(m):
                V = 0.0
                for j in range(L):
                    if F[j]:
                        d = X[k][j] - mean[k]
                        V = V + (w[j] * d) * d
                scale[k] = _sqrt(_div(V, W))
                live[k] = 0.0 < scale[k] < math.inf
                if not live[k]:
                    bits |= 1 << k
            if nF < sum(live) + 2:
                status, bits = 1, 0
                mean, scale, live = [0.0] * m, [1.0] * m, [False] * m
        if status == 1:
            break
        z = [_div(y[j], mu) - 1.0 for j in range(L)]
        U = [[_div(X[k][j] - mean[k], scale[k]) if live[k] else 0.0 for j in range(L)] for k in range(m)]
        G = [[0.0] * m for _ in range(m)]
        b = [0.0] * m
        for k in range(m):
            for l in range(k + 1):
                s = 0.0
                for j in range(L):
                    if F[j]:
                        s = s + (w[j] * U[k][j]) * U[l][j]
                G[k][l] = s
            G[k][k] = G[k][k] + ridge * W
            s = 0.0
            for j in range(L):
                if F[j]:
                    s = s + (w[j] * U[k][j]) * z[j]
            b[k] = s
        c, live, more = _cholesky_solve(G, b, live, m)
        bits |= more
        r = [0.0] * L
        Q = 0.0
        for j in range(L):
            p = 0.0
            for k in range(m):
                if live[k]:
                    p = p + c[k] * U[k][j]
            r[j] = z[j] - p
            if F[j]:
                Q = Q + (w[j] * r[j]) * r[j]
        sigma = _sqrt(_div(Q, W))
        if rounds == n_iter:
            break
        up = up_k * sigma
        down = -(down_k * sigma)
        left = 0
        for j in range(L):
            if F[j] and (r[j] > up or r[j] < down):
                F[j] = False
                left += 1
        rounds += 1
        n_clipped += left
        if left == 0:
            break
    trend, flat = [0.0] * L, [0.0] * L
    bad = False
    for j in range(L):
        p = 0.0
        for k in range(m):
            if live[k]:
                p = p + c[k] * _div(X[k][j] - mean[k], scale[k])
        trend[j] = mu * (1.0 + p)
        flat[j] = _div(y[j], trend[j])
        bad = bad or not (0.0 < trend[j] < math.inf)
    if bad:
        status = 2
        trend = [mu] * L
        flat = [_div(y[j], mu) for j in range(L)]
    record = (float(status), float(bits), float(sum(F)), float(n_clipped), float(rounds), mu, sigma, float(sum(live)))
    return flat, trend, record, c, mean, scale


# ---- the numpy form ---------------------------------------------------------------------------------------------------------
def _osum(v, member):
    """The ordered sums of v [..., L] along its last axis over the points of member [L], from +0.0."""
    v = numpy.where(member, v, 0.0)
    return numpy.cumsum(numpy.concatenate([numpy.zeros(v.shape[:-1] + (1,)), v], axis=-1), axis=-1)[..., -1]


def _segment_numpy(y, w, open_, X, ridge, n_iter, up_k, down_k):
    """_segment_loops with arrays: y, w [L], open_ [L] bool, X [m, L]."""
    L, m = len(y), len(X)
    F = open_.copy()
    rounds = n_clipped = 0
    with numpy.errstate(all="ignore"):
        while True:
            nF = int(F.sum())
            member = F if nF else numpy.ones(L, dtype=bool)
            W = _osum(w * 1.0, member)
            mu = _osum(w * y, member) / W
            status, bits, sigma = 0, 0, numpy.float64("nan")
            c, mean, scale, live = numpy.zeros(m), numpy.zeros(m), numpy.ones(m), numpy.zeros(m, dtype=bool)
            if nF == 0:
                status = 1
            else:
                mean = _osum(w[None, :] * X, F) / W
                d = X - mean[:, None]
                scale = numpy.sqrt(_osum((w[None, :] * d) * d, F) / W)
                live = (scale > 0.0) & (scale < numpy.inf)
                bits = int(sum(1 << k for k in range(m) if not live[k]))
                if nF < int(live.sum()) + 2:
                    status, bits = 1, 0
                    mean, scale, live = numpy.zeros(m), numpy.ones(m), numpy.zeros(m, dtype=bool)
            if status == 1:
                break
            z = y / mu - 1.0
            U = numpy.where(live[:, None], d / numpy.where(live, scale, 1.0)[:, None], 0.0)
            wU = w[None, :] * U
            G = _osum(wU[:, None, :] * U[None, :, :], F)
            G[numpy.arange(m), numpy.arange(m)] = numpy.diag(G) + ridge * W
            b = _osum(wU * z[None, :], F)
            c, live, more = _cholesky_solve(G.tolist(), b.tolist(), live.tolist(), m)
            c, live = numpy.array(c), numpy.array(live, dtype=bool)
            bits |= more
            p = numpy.zeros(L)
            for k in range(m):
                if live[k]:
                    p = p + c[k] * U[k]
            r = z - p
            sigma = numpy.sqrt(_osum((w * r) * r, F) / W)
            if rounds == n_iter:
                break
            up = up_k * sigma
            down = -(down_k * sigma)
            out = F & ((r > up) | (r < down))
            left = int(out.sum())
            F = F & ~out
            rounds += 1
            n_clipped += left
            if left == 0:
                break
        p = numpy.zeros(L)
        for k in range(m):
            if live[k]:
                p = p + c[k] * ((X[k] - mean[k]) / scale[k])
        trend = mu * (1.0 + p)
        flat = y / trend
        if not numpy.all((trend > 0.0) & (trend < numpy.inf)):
            status = 2
            trend = numpy.full(L, mu)
            flat = y / mu
    record = (float(status), float(bits), float(F.sum()), float(n_clipped), float(rounds), float(mu), float(sigma),
              float(live.sum()))
    return flat, trend, record, c, mean, scale


def _run(segment, y, dy, mask, shared, own, segments, ridge, n_iter, sigma_upper, sigma_lower, as_lists):
    y = numpy.asarray(y, dtype=numpy.float64)
    R, n = y.shape
    shared = numpy.zeros((0, n)) if shared is None else numpy.asarray(shared, dtype=numpy.float64).reshape(-1, n)
    own = numpy.zeros((R, 0, n)) if own is None else numpy.asarray(own, dtype=numpy.float64).reshape(R, -1, n)
    m = shared.shape[0] + own.shape[1]
    assert 1 <= m <= MAX_TERMS and 0 <= int(n_iter) <= MAX_ITER
    segments = [0, n] if segments is None else [int(s) for s in segments]
    assert segments[0] == 0 and segments[-1] == n and all(a < b for a, b in zip(segments, segments[1:]))
    S = len(segments) - 1
    with numpy.errstate(all="ignore"):
        w = numpy.ones((R, n)) if dy is None else 1.0 / (numpy.asarray(dy, dtype=numpy.float64) * numpy.asarray(dy, dtype=numpy.float64))
    open_ = numpy.ones((R, n), dtype=bool) if mask is None else numpy.asarray(mask) == 0
    flat, trend = numpy.empty((R, n)), numpy.empty((R, n))
    record = numpy.zeros((R, S, len(FIELDS)))
    coef, mean, scale = numpy.zeros((R, S, m)), numpy.zeros((R, S, m)), numpy.zeros((R, S, m))
    for i in range(R):
        X = numpy.concatenate([shared, own[i]], axis=0)
        for s in range(S):
            lo, hi = segments[s], segments[s + 1]
            args = (y[i, lo:hi], w[i, lo:hi], open_[i, lo:hi], X[:, lo:hi])
            if as_lists:
                args = tuple(a.tolist() for a in args)
            out = segment(*args, float(ridge), int(n_iter), float(sigma_upper), float(sigma_lower))
            flat[i, lo:hi], trend[i, lo:hi], record[i, s], coef[i, s], mean[i, s], scale[i, s] = out
    return {"flat": flat, "trend": trend, "record": record, "coef": coef, "mean": mean, "scale": scale}


def loops(y, dy=None, mask=None, shared=None, own=None, segments=None, ridge=0.0, n_iter=3, sigma_upper=5.0, sigma_lower=5.0):
    """The statement in plain Python floats: a dict with flat, trend [R, n], record [R, S, len(FIELDS)], coef, mean and scale
    [R, S, m]."""
    return _run(_segment_loops, y, dy, mask, shared, own, segments, ridge, n_iter, sigma_upper, sigma_lower, True)


def fit(y, dy=None, mask=None, shared=None, own=None, segments=None, ridge=0.0, n_iter=3, sigma_upper=5.0, sigma_lower=5.0):
    """The same statement with numpy over the points and the columns: equal to `loops` bit for bit."""
    return _run(_segment_numpy, y, dy, mask, shared, own, segments, ridge, n_iter, sigma_upper, sigma_lower, False)


def coefficients(out):
    """coef / scale: the coefficients in the units of the raw columns (0.0 where the column is not in the fit)."""
    with numpy.errstate(all="ignore"):
        return numpy.where(out["coef"] != 0.0, out["coef"] / out["scale"], 0.0)
