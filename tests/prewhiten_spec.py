"""Iterative sinusoid pre-whitening of survey.prewhiten_batch / tls_prewhiten, restated in Python: the definition the kernels
are tested against (include/tls_amd.h, DESIGN.md "Pre-whitening" and the docstrings state the same lines).  It shares no code
with the library; the periodogram's pieces come from gls_spec.

For a curve y [n] (weights from dy [n], or uniform) over the shared ascending t [n] and the grid f [F]; r starts as y, trend
as 0.0.  Iteration j = 0 .. K - 1, while the curve runs:

    spectrum: power [F] of r: gls_spec.prologue (index order), the six sums, gls_spec.epilogue.  C, S, C2, S2 depend on the
        weights alone.  ybar_0 = the mean of the first prologue.
    pick: k = the first index of the largest finite power; none: status 2, stop; power[k] < min_power: status 1, stop.
    refine: if 0 < k < F - 1, both neighbours finite and den = p[k-1] - 2.0 * p[k] + p[k+1] < 0:
        half = 0.5 * (f[k+1] - f[k-1]);  f* = f[k] + 0.5 * half * (p[k-1] - p[k+1]) / den;      otherwise f* = f[k]
    for h = 1 .. H, each on the row the harmonic before left:  fh = h * f*
        the sine test's statement with no mask: W, ybar, YY as ordered 256-lane sums (gls_spec.lanes_sum), the six sums at fh
        and 2.0 * fh as ordered lane sums of the rounded products, the epilogue with ca and sa
        NaN: the harmonic is skipped (term status 1); otherwise, for every i:
            u = cos phi_i - C;  v = sin phi_i - S;  q = ca * u + sa * v;  r_i = r_i - q;  trend_i = trend_i + q

At the end trend_i = ybar_0 + trend_i and flat_i = y_i / trend_i.  Every step is one IEEE double operation.

What the device may differ by.  The sums of the spectrum and of the fit are dot products: gls_spec.sum_bound.  The pick is
compared only where the statement's highest power stands clear of every other by a relative gap of 1e-6 (the tests assert that
of their inputs; the sums' bound moves a power by about 1e-13 of itself).  In the subtraction phi_i is formed by three IEEE
operations and is bit-equal; cos and sin of the device's library differ from numpy's by a few ulp of a value of at most 1, so
u and v differ by at most 4 * 2^-52 each (a generous 4 ulp of 1 for the function, the rounding of the difference being the
same operation on both sides up to that), and q by that times |ca| and |sa| plus the roundings of two products and a sum of
terms bounded by 2 |ca| + 2 |sa| -- together below 8 * 2^-52 * (|ca| + |sa|), the trigonometry's share of sum_bound's
"+ 8".  The final r_i = r_i - q is then rounded once more, which can land on the neighbouring double: one ulp of r_i.  Where
the subtraction carries r_i across a power of two (a flux next to 1.0 does that all the time) the neighbouring doubles of the
result are spaced by the ulp of the larger binade, so the ulp is taken of the larger of r_i before and r_i after.

    subtract_bound_i = 8 * 2^-52 * (|ca| + |sa|) + ulp(max(|r_i before|, |r_i after|))
"""
import numpy

import gls_spec

TERM_FIELDS = ("status", "index", "frequency_grid", "power_left", "power_peak", "power_right", "frequency", "mean", "variance",
               "ca", "sa", "C", "S", "power", "amplitude", "phase")


def weights(n, dy=None):
    """w [n] with the sine test's ordered lane sum of the inverse variances."""
    if dy is None:
        return numpy.full(n, numpy.float64(1.0) / numpy.float64(n))
    dy = numpy.asarray(dy, dtype=numpy.float64)
    v = 1.0 / (dy * dy)
    return v / gls_spec.lanes_sum(v, numpy.ones(n, dtype=bool))


def lane_prologue(row, dy=None):
    """(w, a, ybar, YY) of a row with ordered 256-lane sums."""
    row = numpy.asarray(row, dtype=numpy.float64)
    used = numpy.ones(len(row), dtype=bool)
    w = weights(len(row), dy)
    ybar = gls_spec.lanes_sum(w * row, used)
    d = row - ybar
    a = w * d
    return w, a, ybar, gls_spec.lanes_sum(a * d, used)


def lane_six_sums(t, w, a, f):
    """(YC, YS, C, S, C2, S2) at the frequency f as ordered lane sums of the rounded products (numpy's cos and sin)."""
    used = numpy.ones(len(w), dtype=bool)
    phi, phi2 = gls_spec.phases(t, f), gls_spec.phases(t, 2.0 * numpy.float64(f))
    c1, s1, c2, s2 = numpy.cos(phi), numpy.sin(phi), numpy.cos(phi2), numpy.sin(phi2)
    return numpy.array([gls_spec.lanes_sum(q, used) for q in (a * c1, a * s1, w * c1, w * s1, w * c2, w * s2)])


def exact_six_sums(t, w, a, f):
    """The same six sums exact (to bound the device's)."""
    return gls_spec.six_sums(t, w, a, numpy.array([f], dtype=numpy.float64))[0]


def fit_epilogue(sums, YY):
    """(power, amplitude, phase, ca, sa) of six sums: gls_spec.epilogue's steps, ca and sa kept."""
    YC, YS, C, S, C2, S2 = (numpy.float64(v) for v in sums)
    YY = numpy.float64(YY)
    nan = numpy.float64(numpy.nan)
    with numpy.errstate(all="ignore"):
        CC = 0.5 * (1.0 + C2) - C * C
        SS = 0.5 * (1.0 - C2) - S * S
        CS = 0.5 * S2 - C * S
        D = CC * SS - CS * CS
        if not (D > 0.0) or not (YY > 0.0):
            return nan, nan, nan, nan, nan
        power = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D)
        ca = (YC * SS - YS * CS) / D
        sa = (YS * CC - YC * CS) / D
        return power, numpy.sqrt(ca * ca + sa * sa), numpy.arctan2(sa, ca) / gls_spec.TWO_PI, ca, sa


def pick(power):
    """The first index of the largest finite power, or -1."""
    power = numpy.asarray(power, dtype=numpy.float64)
    finite = numpy.isfinite(power)
    if not finite.any():
        return -1
    return int(numpy.argmax(numpy.where(finite, power, -numpy.inf)))


def refine(f, k, left, peak, right):
    """f* from the grid f, the pick k and the three powers (left, right: NaN where the grid ends)."""
    f = numpy.asarray(f, dtype=numpy.float64)
    left, peak, right = numpy.float64(left), numpy.float64(peak), numpy.float64(right)
    if 0 < k < len(f) - 1 and numpy.isfinite(left) and numpy.isfinite(right):
        den = left - 2.0 * peak + right
        if den < 0.0:
            half = 0.5 * (f[k + 1] - f[k - 1])
            return f[k] + 0.5 * half * (left - right) / den
    return f[k]


def subtraction(t, row, fh, ca, sa, C, S):
    """(the row behind the subtraction, q) for the coefficients of a fit."""
    phi = gls_spec.phases(t, fh)
    u = numpy.cos(phi) - numpy.float64(C)
    v = numpy.sin(phi) - numpy.float64(S)
    q = numpy.float64(ca) * u + numpy.float64(sa) * v
    return numpy.asarray(row, dtype=numpy.float64) - q, q


def subtract_bound(row, after, ca, sa):
    """The bound [n] on |device - statement| of a row behind one subtraction (the module's docstring): `row` enters the
    subtraction, `after` is the statement's result."""
    largest = numpy.maximum(numpy.abs(numpy.asarray(row, dtype=numpy.float64)), numpy.abs(numpy.asarray(after, dtype=numpy.float64)))
    return 8.0 * 2.0 ** -52 * (abs(float(ca)) + abs(float(sa))) + numpy.spacing(largest)


def spectrum(t, row, f, dy=None, weight_sums=None):
    """(power [F], ybar, YY, weight sums) of a row on the grid: the periodogram's statement with _fast_sums; weight_sums
    (C, S, C2, S2 [F] each) may be handed on from an earlier call, since they depend on the weights alone."""
    f = numpy.asarray(f, dtype=numpy.float64)
    w, a, ybar, YY = gls_spec.prologue(row, dy)
    if weight_sums is None:
        cs = _fast_sums(t, w, f)
        cs2 = _fast_sums(t, w, 2.0 * f)
        weight_sums = (cs[:, 0], cs[:, 1], cs2[:, 0], cs2[:, 1])
    ya = _fast_sums(t, a, f)
    power = gls_spec.epilogue(ya[:, 0], ya[:, 1], *weight_sums, YY)[0]
    return power, ybar, YY, weight_sums


def _fast_sums(t, a, f):
    """[F, 2] the sums of a row in numpy's pairwise order: within sum_bound of the exact ones, and far closer than the gap the
    tests demand between the highest power and the rest."""
    t = numpy.asarray(t, dtype=numpy.float64)
    out = numpy.empty((len(f), 2))
    for lo in range(0, len(f), 256):
        x = numpy.outer(f[lo:lo + 256], t - t[0])
        phi = gls_spec.TWO_PI * (x - numpy.floor(x))
        out[lo:lo + 256, 0] = numpy.cos(phi) @ a
        out[lo:lo + 256, 1] = numpy.sin(phi) @ a
    return out


def prewhiten(t, y, f, dy=None, n_terms=3, harmonics=1, min_power=0.0):
    """dict(flat, trend, r, status, n_iterations, mean0, terms [K][H] of dicts (TERM_FIELDS, plus sums), powers (the spectrum
    of every iteration that was formed), gaps (the relative gap between the highest power and every other, an iteration)) of
    one curve."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    f = numpy.asarray(f, dtype=numpy.float64)
    r = y.copy()
    trend = numpy.zeros(len(y))
    out = dict(status=0.0, n_iterations=0, terms=[], powers=[], gaps=[], steps=[])
    weight_sums = None
    for j in range(n_terms):
        power, ybar, _, weight_sums = spectrum(t, r, f, dy, weight_sums)
        if j == 0:
            out["mean0"] = ybar
        out["powers"].append(power)
        k = pick(power)
        if k < 0:
            out["status"] = 2.0
            break
        others = numpy.delete(power, k)
        others = others[numpy.isfinite(others)]
        out["gaps"].append(numpy.inf if not len(others) else float((power[k] - others.max()) / power[k]))
        if power[k] < min_power:
            out["status"] = 1.0
            break
        left = power[k - 1] if k > 0 else numpy.nan
        right = power[k + 1] if k < len(f) - 1 else numpy.nan
        fstar = refine(f, k, left, power[k], right)
        row_terms = []
        for h in range(1, harmonics + 1):
            fh = numpy.float64(h) * fstar
            out["steps"].append(r.copy())
            w, a, mean, YY = lane_prologue(r, dy)
            sums = lane_six_sums(t, w, a, fh)
            p, amplitude, phase, ca, sa = fit_epilogue(sums, YY)
            term = dict(status=0.0 if numpy.isfinite(p) else 1.0, index=float(k), frequency_grid=f[k], power_left=left,
                        power_peak=power[k], power_right=right, frequency=fh, mean=mean, variance=YY, ca=ca, sa=sa, C=sums[2],
                        S=sums[3], power=p, amplitude=amplitude, phase=phase, sums=sums)
            if term["status"] == 0.0:
                r, q = subtraction(t, r, fh, ca, sa, sums[2], sums[3])
                trend = trend + q
            row_terms.append(term)
        out["terms"].append(row_terms)
        out["n_iterations"] = j + 1
    trend = out["mean0"] + trend
    out.update(r=r, trend=trend, flat=y / trend)
    return out
