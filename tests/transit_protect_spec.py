"""Transit-protected detrending (tls_transit_mask, tls_biweight_detrend_masked, tls_prewhiten_masked of include/tls_amd.h)
restated in numpy: the definition the kernels are tested against.  It shares no code with the library; the unmasked pieces
come from biweight_spec and prewhiten_spec.  Every step is one IEEE double operation in the order written, so the mask, the
masked biweight's trend, flat and status are the device's bit for bit; masked pre-whitening is compared as
test_prewhiten.py compares the unmasked call (prewhiten_spec's bounds).  Slow by design.

    transit_mask: point i of curve c is protected if any candidate k of curve c with a finite period, T0 and duration,
        period > 0 and duration > 0 has
            d = t[i] - T0_k;  e = floor(d / P_k + 0.5);  r = d - e * P_k;  |r| <= 0.5 * (factor * duration_k)

    biweight_masked: the windows of biweight_spec.windows (t alone; a protected i keeps its window).  Members of window i =
        its unprotected j, m_i their number.
            m_i >= min(min_points, the window's length): trend_i = biweight_spec.location(members), status 0 (a window of
                fewer than min_points points is fitted when none of them is protected, so that an empty mask is the unmasked call)
            otherwise open; a, b = the nearest status-0 points left and right in i's segment:
                both: trend_i = ta + (tb - ta) * ((t[i] - t[a]) / (t[b] - t[a])), ta where t[b] == t[a]; status 1
                one: its trend; status 1
                none: biweight_spec.location of the whole window, the mask ignored; status 2
        flat = y / trend

    prewhiten_masked: prewhiten_spec.prewhiten with v_i = 0.0 where protected, elsewhere 1 / (dy_i dy_i) or 1.0 without dy,
        W = the ordered sum of the v_i (index order in the spectrum's prologue, 256 lanes in the fit), w_i = v_i / W, in the
        mean, the variance, the periodogram and the fit; the subtraction and the trend cover every point.  A row with fewer
        than 3 unprotected points has nothing removed: status 2, trend = its mean with the mask ignored.
"""
import numpy

import biweight_spec
import gls_spec
import prewhiten_spec


def transit_mask(t, period, T0, duration, curve=None, n_curves=None, factor=1.5):
    """uint8 [n_curves, n], 1 = protected."""
    t = numpy.asarray(t, dtype=numpy.float64)
    period, T0, duration = (numpy.atleast_1d(numpy.asarray(v, dtype=numpy.float64)) for v in (period, T0, duration))
    m = len(period)
    curve = numpy.arange(m) if curve is None else numpy.asarray(curve, dtype=numpy.int64)
    if n_curves is None:
        n_curves = int(curve.max()) + 1 if m else 0
    out = numpy.zeros((n_curves, len(t)), dtype=numpy.uint8)
    factor = numpy.float64(factor)
    with numpy.errstate(all="ignore"):
        for k in range(m):
            P, T, D = period[k], T0[k], duration[k]
            if not (numpy.isfinite(P) and numpy.isfinite(T) and numpy.isfinite(D) and P > 0 and D > 0):
                continue
            d = t - T
            e = numpy.floor(d / P + 0.5)
            r = d - e * P
            out[curve[k]] |= (numpy.abs(r) <= 0.5 * (factor * D)).astype(numpy.uint8)
    return out


def segments(t, break_tolerance):
    """seg [n]: the number of every point's segment (a new one starts at every j with t[j] - t[j-1] > break_tolerance)."""
    t = numpy.asarray(t, dtype=numpy.float64)
    new = numpy.zeros(len(t), dtype=bool)
    new[1:] = (t[1:] - t[:-1]) > break_tolerance
    return numpy.cumsum(new)


def interpolate(t, i, a, b, ta, tb):
    """The trend of the open point i between the fitted points a and b."""
    t = numpy.asarray(t, dtype=numpy.float64)
    den = t[b] - t[a]
    if den == 0.0:
        return numpy.float64(ta)
    return numpy.float64(ta) + (numpy.float64(tb) - numpy.float64(ta)) * ((t[i] - t[a]) / den)


def biweight_masked(t, y, mask, window_length, break_tolerance, min_points=3):
    """(flat, trend, status uint8) of y [n] or [n_rows, n] with the mask of the same shape (!= 0: protected)."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    rows = y[None, :] if y.ndim == 1 else y
    masks = numpy.asarray(mask).reshape(rows.shape) != 0
    n = len(t)
    lo, hi = biweight_spec.windows(t, window_length, break_tolerance)
    seg = segments(t, break_tolerance)
    trend = numpy.empty(rows.shape)
    status = numpy.empty(rows.shape, dtype=numpy.uint8)
    for r, (row, prot) in enumerate(zip(rows, masks)):
        fitted = numpy.zeros(n, dtype=bool)
        for i in range(n):
            members = row[lo[i]:hi[i]][~prot[lo[i]:hi[i]]]
            if len(members) >= min(min_points, hi[i] - lo[i]):
                trend[r, i] = biweight_spec.location(members)
                fitted[i] = True
        status[r] = numpy.where(fitted, 0, 1)
        for i in numpy.flatnonzero(~fitted):
            left = numpy.flatnonzero(fitted[:i] & (seg[:i] == seg[i]))
            right = i + 1 + numpy.flatnonzero(fitted[i + 1:] & (seg[i + 1:] == seg[i]))
            if len(left) and len(right):
                a, b = left[-1], right[0]
                trend[r, i] = interpolate(t, i, a, b, trend[r, a], trend[r, b])
            elif len(left) or len(right):
                trend[r, i] = trend[r, left[-1] if len(left) else right[0]]
            else:
                trend[r, i] = biweight_spec.location(row[lo[i]:hi[i]])
                status[r, i] = 2
    flat = rows / trend
    return (flat[0], trend[0], status[0]) if y.ndim == 1 else (flat, trend, status)


# ---- masked pre-whitening -------------------------------------------------------------------------------------------------
def inverse_variances(n, dy, prot):
    """v [n]: 0.0 where protected, elsewhere 1 / (dy dy), or 1.0 without dy."""
    v = numpy.ones(n) if dy is None else 1.0 / (numpy.asarray(dy, dtype=numpy.float64) * numpy.asarray(dy, dtype=numpy.float64))
    return numpy.where(prot, 0.0, v)


def index_prologue(row, v):
    """(w, a, ybar, YY) of a row with sums in index order (the spectrum's prologue)."""
    w = v / gls_spec.ordered(v)
    ybar = gls_spec.ordered(w * row)
    d = row - ybar
    a = w * d
    return w, a, ybar, gls_spec.ordered(a * d)


def lane_prologue(row, v):
    """(w, a, ybar, YY) of a row with ordered 256-lane sums (the fit's prologue)."""
    used = numpy.ones(len(row), dtype=bool)
    w = v / gls_spec.lanes_sum(v, used)
    ybar = gls_spec.lanes_sum(w * row, used)
    d = row - ybar
    a = w * d
    return w, a, ybar, gls_spec.lanes_sum(a * d, used)


def prewhiten_masked(t, y, f, mask, dy=None, n_terms=3, harmonics=1, min_power=0.0):
    """prewhiten_spec.prewhiten's dict for one curve with the masked weights; `weights` (w of the spectrum's prologue) added."""
    t = numpy.asarray(t, dtype=numpy.float64)
    y = numpy.asarray(y, dtype=numpy.float64)
    f = numpy.asarray(f, dtype=numpy.float64)
    prot = numpy.asarray(mask).reshape(y.shape) != 0
    n = len(y)
    out = dict(status=0.0, n_iterations=0, terms=[], powers=[], gaps=[], steps=[])
    if int((~prot).sum()) < 3:
        ybar = index_prologue(y, inverse_variances(n, dy, numpy.zeros(n, dtype=bool)))[2]
        trend = ybar + numpy.zeros(n)
        out.update(status=2.0, mean0=ybar, r=y.copy(), trend=trend, flat=y / trend, weights=None)
        return out
    v = inverse_variances(n, dy, prot)
    r = y.copy()
    trend = numpy.zeros(n)
    weight_sums = None
    for j in range(n_terms):
        w, a, ybar, YY = index_prologue(r, v)
        if weight_sums is None:
            cs, cs2 = prewhiten_spec._fast_sums(t, w, f), prewhiten_spec._fast_sums(t, w, 2.0 * f)
            weight_sums = (cs[:, 0], cs[:, 1], cs2[:, 0], cs2[:, 1])
            out["weights"] = w
        ya = prewhiten_spec._fast_sums(t, a, f)
        power = gls_spec.epilogue(ya[:, 0], ya[:, 1], *weight_sums, YY)[0]
        if j == 0:
            out["mean0"] = ybar
        out["powers"].append(power)
        k = prewhiten_spec.pick(power)
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
        fstar = prewhiten_spec.refine(f, k, left, power[k], right)
        row_terms = []
        for h in range(1, harmonics + 1):
            fh = numpy.float64(h) * fstar
            out["steps"].append(r.copy())
            lw, la, mean, lYY = lane_prologue(r, v)
            sums = prewhiten_spec.lane_six_sums(t, lw, la, fh)
            p, amplitude, phase, ca, sa = prewhiten_spec.fit_epilogue(sums, lYY)
            term = dict(status=0.0 if numpy.isfinite(p) else 1.0, index=float(k), frequency_grid=f[k], power_left=left,
                        power_peak=power[k], power_right=right, frequency=fh, mean=mean, variance=lYY, ca=ca, sa=sa, C=sums[2],
                        S=sums[3], power=p, amplitude=amplitude, phase=phase, sums=sums, w=lw, a=la)
            if term["status"] == 0.0:
                r, q = prewhiten_spec.subtraction(t, r, fh, ca, sa, sums[2], sums[3])   # (every point, protected ones included)
                trend = trend + q
            row_terms.append(term)
        out["terms"].append(row_terms)
        out["n_iterations"] = j + 1
    trend = out["mean0"] + trend
    out.update(r=r, trend=trend, flat=y / trend)
    return out
