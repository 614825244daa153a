"""The generalised Lomb-Scargle periodogram of survey.lomb_scargle / tls_lomb_scargle and the sine test of survey.sine_test /
tls_sine_test (Zechmeister & Kuerster 2009), restated in Python: the definition the kernels are tested against
(include/tls_amd.h, DESIGN.md "Variability periodogram" and the docstrings state the same lines).  It shares no code with
the library.

    prologue(y[n], dy[n] or None), every sum in index order:
        v_i = 1.0 / (dy_i * dy_i);  W = sum v_i;  w_i = v_i / W                (without dy: w_i = 1.0 / n)
        ybar = sum (w_i * y_i);  d_i = y_i - ybar;  a_i = w_i * d_i;  YY = sum (a_i * d_i)
    phase of (frequency f, point i):  e = t_i - t_0;  x = f * e;  r = x - floor(x);  phi = 6.283185307179586 * r
    six sums, EXACT (math.fsum over numpy's double cos / sin of phi):
        YC, YS = sum a_i cos phi, sum a_i sin phi;  C, S = sum w_i cos phi, sum w_i sin phi;  C2, S2 = the same of w at 2.0 * f
    epilogue, one IEEE double operation a step:
        CC = 0.5 * (1.0 + C2) - C * C;  SS = 0.5 * (1.0 - C2) - S * S;  CS = 0.5 * S2 - C * S;  D = CC * SS - CS * CS
        power = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D)
        ca = (YC * SS - YS * CS) / D;  sa = (YS * CC - YC * CS) / D
        amplitude = sqrt(ca * ca + sa * sa);  phase = atan2(sa, ca) / 6.283185307179586
        NaN in all three where D <= 0 or YY <= 0

The device forms the six sums in fp64 FMAs; an n-term dot product in any order, the rounding of the phase carried through
the trigonometry and a few ulp of the trigonometry itself bound its distance from the exact sums by

    sum_bound = (n + 2 pi max|f (t - t_0)| + 8) * 2^-52 * sum_i |A[r, i]|.

sine_test states the per-candidate version: ordered sums over 256 lanes instead of sums in index order."""
import math

import numpy

TWO_PI = 6.283185307179586
LANES = 256


def ordered(values):
    """The sum of `values` in index order, one IEEE addition a term, from 0.0."""
    total = numpy.float64(0.0)
    for v in numpy.asarray(values, dtype=numpy.float64):
        total = total + v
    return total


def prologue(y, dy=None):
    """(w [n], a [n], ybar, YY) of one curve."""
    y = numpy.asarray(y, dtype=numpy.float64)
    n = len(y)
    if dy is None:
        w = numpy.full(n, numpy.float64(1.0) / numpy.float64(n))
    else:
        dy = numpy.asarray(dy, dtype=numpy.float64)
        v = 1.0 / (dy * dy)
        w = v / ordered(v)
    ybar = ordered(w * y)
    d = y - ybar
    a = w * d
    return w, a, ybar, ordered(a * d)


def phases(t, f):
    """phi [n] of frequency f."""
    t = numpy.asarray(t, dtype=numpy.float64)
    x = numpy.float64(f) * (t - t[0])
    r = x - numpy.floor(x)
    return TWO_PI * r


def exact_sums(t, rows, frequencies):
    """[R, F, 2]: (sum_i rows[r, i] cos phi_ki, sum_i rows[r, i] sin phi_ki), each sum exact and then rounded once."""
    rows = numpy.atleast_2d(numpy.asarray(rows, dtype=numpy.float64))
    out = numpy.zeros((len(rows), len(frequencies), 2))
    for k, f in enumerate(frequencies):
        phi = phases(t, f)
        c, s = numpy.cos(phi), numpy.sin(phi)
        for r, row in enumerate(rows):
            out[r, k, 0] = math.fsum(row * c)
            out[r, k, 1] = math.fsum(row * s)
    return out


def sum_bound(t, rows, frequencies):
    """The bound [R] on |device - exact| of every sum of a row."""
    t = numpy.asarray(t, dtype=numpy.float64)
    rows = numpy.atleast_2d(numpy.asarray(rows, dtype=numpy.float64))
    reach = float(numpy.max(numpy.abs(numpy.outer(frequencies, t - t[0]))))
    return (len(t) + 2.0 * numpy.pi * reach + 8.0) * 2.0 ** -52 * numpy.abs(rows).sum(axis=1)


def epilogue(YC, YS, C, S, C2, S2, YY):
    """(power, amplitude, phase) of arrays of sums, elementwise."""
    YC, YS, C, S, C2, S2, YY = numpy.broadcast_arrays(*(numpy.asarray(v, dtype=numpy.float64) for v in (YC, YS, C, S, C2, S2, YY)))
    with numpy.errstate(all="ignore"):
        CC = 0.5 * (1.0 + C2) - C * C
        SS = 0.5 * (1.0 - C2) - S * S
        CS = 0.5 * S2 - C * S
        D = CC * SS - CS * CS
        power = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D)
        ca = (YC * SS - YS * CS) / D
        sa = (YS * CC - YC * CS) / D
        amplitude = numpy.sqrt(ca * ca + sa * sa)
        phase = numpy.arctan2(sa, ca) / TWO_PI
        bad = ~((D > 0.0) & (YY > 0.0))
    return numpy.where(bad, numpy.nan, power), numpy.where(bad, numpy.nan, amplitude), numpy.where(bad, numpy.nan, phase)


def six_sums(t, w, a, frequencies):
    """[F, 6] (YC, YS, C, S, C2, S2) of one curve, exact."""
    frequencies = numpy.asarray(frequencies, dtype=numpy.float64)
    ya = exact_sums(t, a, frequencies)[0]
    cs = exact_sums(t, w, frequencies)[0]
    cs2 = exact_sums(t, w, 2.0 * frequencies)[0]
    return numpy.concatenate([ya, cs, cs2], axis=1)


def lomb_scargle(t, y, frequencies, dy=None):
    """dict(power, amplitude, phase [F], mean, variance, sums [F, 6], w, a) of one curve."""
    w, a, ybar, YY = prologue(y, dy)
    sums = six_sums(t, w, a, frequencies)
    power, amplitude, phase = epilogue(*sums.T, YY)
    return dict(power=power, amplitude=amplitude, phase=phase, mean=ybar, variance=YY, sums=sums, w=w, a=a)


# ---- the sine test -------------------------------------------------------------------------------------------------------------
def lanes_sum(terms, used):
    """The ordered sum of the sine test: lane j = i mod 256 adds terms[i] (0.0 where not used[i]) over its i ascending, from
    0.0; the lanes are added in lane order."""
    terms = numpy.where(used, numpy.asarray(terms, dtype=numpy.float64), 0.0)
    pad = (-len(terms)) % LANES
    grid = numpy.concatenate([terms, numpy.zeros(pad)]).reshape(-1, LANES)
    part = numpy.zeros(LANES)
    for row in grid:
        part = part + row
    total = part[0]
    for j in range(1, LANES):
        total = total + part[j]
    return total


def used_points(t, P, T0, d, mask):
    """The points that stay in the fit: all of them without a mask (T0 None)."""
    t = numpy.asarray(t, dtype=numpy.float64)
    if T0 is None:
        return numpy.ones(len(t), dtype=bool)
    hw = 0.5 * numpy.float64(mask) * numpy.float64(d)
    x = (t - numpy.float64(T0)) / numpy.float64(P)
    k = numpy.floor(x + 0.5)
    tau = (x - k) * numpy.float64(P)
    return ~(numpy.fabs(tau) <= hw)


def sine_test(t, y, P, dy=None, T0=None, d=None, mask=1.5, harmonics=(0.5, 1.0, 2.0)):
    """dict(status, n_used, mean, variance, w, a, used, frequencies [nH], exact [nH, 6]) of one candidate: the prologue with
    ordered sums, and the six sums of every harmonic EXACT (to bound the device's)."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    nan = numpy.nan
    good = numpy.isfinite(P) and P > 0 and (T0 is None or (numpy.isfinite(T0) and numpy.isfinite(d) and d > 0))
    if not good:
        return dict(status=1.0, n_used=nan, mean=nan, variance=nan)
    used = used_points(t, P, T0, d, mask)
    n_used = int(used.sum())
    if n_used < 4:
        return dict(status=2.0, n_used=float(n_used), mean=nan, variance=nan)
    if dy is None:
        w = numpy.full(len(t), numpy.float64(1.0) / numpy.float64(n_used))
    else:
        dy = numpy.asarray(dy, dtype=numpy.float64)
        v = 1.0 / (dy * dy)
        w = v / lanes_sum(v, used)
    ybar = lanes_sum(w * y, used)
    dd = y - ybar
    a = w * dd
    YY = lanes_sum(a * dd, used)
    freqs = numpy.array([1.0 / (numpy.float64(h) * numpy.float64(P)) for h in harmonics])
    exact = six_sums(t, numpy.where(used, w, 0.0), numpy.where(used, a, 0.0), freqs)
    return dict(status=0.0, n_used=float(n_used), mean=ybar, variance=YY, w=w, a=a, used=used, frequencies=freqs, exact=exact)


def sine_harmonics(sums, YY, n_used):
    """(power, amplitude, phase, amplitude_err, significance) [nH] from the sums [nH, 6]."""
    power, amplitude, phase = epilogue(*numpy.asarray(sums, dtype=numpy.float64).T, YY)
    with numpy.errstate(all="ignore"):
        err = numpy.sqrt(2.0 * numpy.float64(YY) * (1.0 - power) / (numpy.float64(n_used) - 3.0))
        return power, amplitude, phase, err, amplitude / err
