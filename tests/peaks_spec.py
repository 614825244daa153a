"""The peak selection of tls_find_peaks / power_batch(peaks=K), restated in numpy: the definition the kernel is tested
against bit for bit (include/tls_amd.h, DESIGN.md "Periodogram peaks", survey.find_peaks state the same lines).

    find_peaks(power[n], periods[n], k, sep, ratios, min_power):
      cand[j] = (j == 0   or power[j] >  power[j-1])
            and (j == n-1 or power[j] >= power[j+1])
            and power[j] >= min_power
      alive = cand
      repeat at most k times, stop when no index is alive:
          j = lowest index of the largest power among alive indices   # numpy.argmax
          take j;  P = periods[j]
          for r in (1.0,) + ratios:
              c = r * P;  w = sep * c
              alive[i] = False for every i with fabs(periods[i] - c) <= w

A NaN makes every comparison false; nothing assumes that `periods` is sorted; c, w and periods[i] - c are one IEEE double
operation each (numpy never contracts them)."""
import numpy

HARMONICS = (0.5, 2.0, 1 / 3, 3.0, 2 / 3, 1.5)


def candidates(power, min_power=-numpy.inf):
    power = numpy.asarray(power, dtype=numpy.float64)
    n = len(power)
    with numpy.errstate(invalid="ignore"):
        left = numpy.ones(n, dtype=bool)
        left[1:] = power[1:] > power[:-1]
        right = numpy.ones(n, dtype=bool)
        right[:-1] = power[:-1] >= power[1:]
        return left & right & (power >= min_power)


def windows(periods, P, sep, ratios):
    """True where an index lies in one of the windows of a peak taken at period P."""
    periods = numpy.asarray(periods, dtype=numpy.float64)
    inside = numpy.zeros(len(periods), dtype=bool)
    with numpy.errstate(invalid="ignore", over="ignore"):
        for r in (1.0,) + tuple(float(x) for x in ratios):
            c = numpy.float64(r) * numpy.float64(P)
            w = numpy.float64(sep) * c
            inside |= numpy.fabs(periods - c) <= w
    return inside


def find_peaks(power, periods, k, sep=0.02, ratios=HARMONICS, min_power=None):
    """The indices taken, in the order taken (at most k)."""
    power = numpy.asarray(power, dtype=numpy.float64)
    periods = numpy.asarray(periods, dtype=numpy.float64)
    alive = candidates(power, -numpy.inf if min_power is None else min_power)
    taken = []
    for _ in range(int(k)):
        if not alive.any():
            break
        j = int(numpy.argmax(numpy.where(alive, power, -numpy.inf)))
        if not alive[j]:   # (every alive power is -inf: the lowest alive index)
            j = int(numpy.argmax(alive))
        taken.append(j)
        alive &= ~windows(periods, periods[j], sep, ratios)
    return numpy.array(taken, dtype=numpy.int64)


def expected(power, periods, k, sep=0.02, ratios=HARMONICS, min_power=None, chi2=None, row=None, depth=None):
    """(records [k], n_peaks) as the device returns them for one row: the fields of tls_peak, NaN / -1 past n_peaks and where
    a field has no source."""
    dtype = numpy.dtype([("period", "f8"), ("power", "f8"), ("chi2", "f8"), ("depth", "f8"), ("index", "i8"), ("row", "i8")])
    out = numpy.zeros(int(k), dtype=dtype)
    for name in ("period", "power", "chi2", "depth"):
        out[name] = numpy.nan
    out["index"] = -1
    out["row"] = -1
    j = find_peaks(power, periods, k, sep, ratios, min_power)
    m = len(j)
    out["index"][:m] = j
    out["period"][:m] = numpy.asarray(periods, dtype=numpy.float64)[j]
    out["power"][:m] = numpy.asarray(power, dtype=numpy.float64)[j]
    if chi2 is not None:
        out["chi2"][:m] = numpy.asarray(chi2)[j]
    if depth is not None:
        out["depth"][:m] = numpy.asarray(depth)[j]
    if row is not None:
        out["row"][:m] = numpy.asarray(row)[j]
    return out, m
