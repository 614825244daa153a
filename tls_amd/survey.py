"""Survey mode (BASELINE config 5): many light curves on the SAME time stamps, grids and
template searched back to back on one GPU by ONE C-ABI call (`tls_search_batch`).  The plan (period
list, duration windows, template rows, work queue order) is prepared once; per light curve only
the flux (and weights) are re-uploaded before the search kernel runs again.

Across GPUs the light curves are simply dealt out: one process per GPU (bench.py), or `devices=[0, 1, ...]` / `devices="auto"`
(every visible GPU) on the calls below -- contiguous slices of the batch to the contexts of a `tls_amd.search.DeviceGroup`, one host thread each, no
collective (every light curve's results come back over its own GPU's copy engine).
"""
import collections
import contextlib
import inspect
import numbers
import operator

import numpy

from . import _checks
from . import search as _search
from .planning import search_inputs


def _batch_inputs(t, flux_batch, dy_batch, power_kwargs):
    """(inp, y_rows, dy_rows): the plan inputs of the first curve and every curve's (y, dy) exactly as
    validate.py would hand them to a single search (validate.py:18,39-40)."""
    flux_batch = numpy.asarray(flux_batch, dtype=numpy.float64)
    if flux_batch.ndim != 2 or flux_batch.shape[1] != len(t):
        raise ValueError("flux_batch must have shape [n_curves, len(t)]")
    first_dy = None if dy_batch is None else numpy.asarray(dy_batch[0], dtype=numpy.float64)
    inp = search_inputs(t, flux_batch[0], first_dy, **power_kwargs)
    if len(inp["t"]) != len(t):
        raise ValueError("light curves must be cleaned before a batched search")
    dy_rows = numpy.empty_like(flux_batch)
    dy_rows[0] = inp["dy"]
    for k in range(1, len(flux_batch)):
        # (the first curve went through validate.py; a point cleaned_array would drop from any other is an error here)
        if not numpy.all(numpy.isfinite(flux_batch[k]) & (flux_batch[k] > 0)):
            raise ValueError("light curve %d has a NaN, infinite or non-positive flux: clean it before a batched search" % k)
        if dy_batch is None:
            dy_rows[k] = numpy.std(flux_batch[k])
        else:
            dy = numpy.asarray(dy_batch[k], dtype=numpy.float64)
            if dy.shape != (len(t),) or not numpy.all(numpy.isfinite(dy) & (dy > 0)):
                raise ValueError("dy of light curve %d is not %d finite positive values" % (k, len(t)))
            dy_rows[k] = dy / numpy.mean(dy)
    y_rows = flux_batch.copy()
    y_rows[0] = inp["y"]
    return inp, y_rows, dy_rows


def _slices(n_curves, n_parts):
    """Contiguous, near-equal slices of the batch (whole launch groups of 32 where the batch allows it)."""
    groups = -(-n_curves // 32)
    bounds = [min(n_curves, 32 * ((groups * r) // n_parts)) for r in range(n_parts)] + [n_curves]
    if groups < n_parts:
        bounds = [(n_curves * r) // n_parts for r in range(n_parts)] + [n_curves]
    return bounds


def _resolve(devices, device, context, n_curves):
    """("group", DeviceGroup) or ("one", device id / None): search.resolve_devices, with "auto" = every visible GPU when
    the batch has at least two light curves for each."""
    kind, what = _search.resolve_devices(devices, device, context)
    if kind == "auto":
        from . import _lib
        n = _lib.device_count()
        kind, what = ("list", list(range(n))) if n > 1 and n_curves >= 2 * n else ("one", None)
    if kind == "list":
        kind, what = "group", _search.device_group(what)
    return kind, what


def _on_devices(group, call, n_curves):
    """call(context, lo, hi) for every device's slice of the batch, on the group's host threads; the slices' results."""
    with group._lock:   # (the group's contexts are not re-entrant: one batch or search at a time)
        bounds = _slices(n_curves, len(group.contexts))
        parts = [None] * len(group.contexts)

        def work(r):
            if bounds[r + 1] > bounds[r]:
                parts[r] = call(group.contexts[r], bounds[r], bounds[r + 1])

        group._threads(work)
    return [p for p in parts if p is not None]


def _run_batch(devices, device, context, n_curves, call):
    """call(context, lo, hi) -> dict of arrays on the resolved context (the given one, or the device's default context) or on
    every device's slice of the batch, the slices joined key by key (None stays None).  One part is returned as it is: the
    padded model rows of a large batch run to hundreds of MB."""
    kind, what = _resolve(devices, device, context, n_curves)
    if kind == "group":
        parts = _on_devices(what, call, n_curves)
    else:
        parts = [call(context if context is not None else _search.default_context(what), 0, n_curves)]
    if len(parts) == 1:
        return parts[0]
    return {k: None if v is None else numpy.concatenate([p[k] for p in parts]) for k, v in parts[0].items()}


def _max_epochs(t, periods):
    """Most transit epochs any pick on this grid can have (all_transit_times from a T0 in [min t, min t + period])."""
    return int(numpy.ceil((numpy.max(t) - numpy.min(t)) / numpy.min(periods))) + 2


def _fap(sde):
    """stats.FAP of every entry of `sde`, vectorised: fap[argmax(threshold > SDE)]."""
    from .stats import _fap_table
    fap, thr = _fap_table()
    sde = numpy.asarray(sde, dtype=numpy.float64)
    if numpy.all(thr[1:] >= thr[:-1]):
        # (ascending thresholds: the first one above SDE is a binary search; none above -- inf or NaN SDE -- gives 0, like argmax)
        idx = numpy.searchsorted(thr, sde, side="right")
        idx[(idx >= len(thr)) | numpy.isnan(sde)] = 0
    else:
        idx = numpy.argmax(thr[None, :] > sde[:, None], axis=1)
    return fap[idx]


def _lc_cap(n, max_epochs):
    """Entries of a model light curve row that no curve of this grid exceeds.  With E epochs and s = int(n / E) * 5 samples a
    grid, the crop to (min t, max t] keeps at most (E + 1) s + 1 grid points (the span is at most E + 1 periods, T0 lies in
    [min t, min t + period]), a few more where rounding makes neighbouring grids overlap; never more than the (E + 2) s of all
    grids."""
    from . import constants as C
    E = numpy.arange(1, max(int(max_epochs), 1) + 1)
    s = (n / E).astype(numpy.int64) * C.OVERSAMPLE_MODEL_LIGHT_CURVE
    return max(1, int(numpy.max(numpy.minimum((E + 2) * s, (E + 1) * s + 2 * E + 8))))


def _model_template(inp):
    """_lib.ModelTemplate of the search's template shape: the in-transit slice of the supersampled curve, as
    template.reference_transit takes it (cached per shape), and maxw = int(max(durations) * n) (api.py:140)."""
    from ._lib import ModelTemplate
    from .template import _supersampled_curve
    t_s, f_s, first = _supersampled_curve(**inp["shape"])
    maxw = int(numpy.max(inp["durations"]) * numpy.size(inp["t"]))
    return ModelTemplate(t_s[first: -first + 1], f_s[first: -first + 1], t_s[first], t_s[-first - 1], maxw)


# ---- detrending: a median filter on the device ----------------------------------------------------------------------------
def detrend_batch(flux_batch, kernel_size=25, return_trend=False, context=None, device=None, devices=None):
    """flat = flux / scipy.signal.medfilt(flux, kernel_size) for every row of flux_batch ([n] or [n_curves, n]), on the device
    (tls_medfilt_detrend): the step in front of TLS in the reference's own workflow (its tutorials' y / medfilt(y, 25)).

    The trend is the median of the kernel_size SAMPLES centred on each point -- a window in samples, not in time, blind to
    gaps -- with the row padded by zeros at both ends, as scipy pads it (ndimage.rank_filter(y, k // 2, size=k,
    mode="constant")); flat is one IEEE division per point.  Both are bit-equal to scipy's.  kernel_size must be an odd integer
    in [1, min(n, MEDFILT_MAX_KERNEL)] and every flux value finite and > 0: a kernel longer than the row is an error here
    (scipy only warns and returns zeros in the trend).  The arguments are checked before any device work.  A median filter of
    k samples absorbs the middle of any transit longer than about k / 2 samples: keep kernel_size well above the longest
    duration searched for.

    devices=[...] deals the rows out over several GPUs, as the other survey calls.  Returns flat, or (flat, trend), in the
    shape of flux_batch."""
    from ._lib import medfilt_arguments
    rows, k = medfilt_arguments(flux_batch, kernel_size)

    def call(ctx, lo, hi):
        out = ctx.medfilt_detrend(rows[lo:hi], k, return_trend=return_trend)
        return dict(flat=out[0], trend=out[1]) if return_trend else dict(flat=out, trend=None)

    out = _run_batch(devices, device, context, len(rows), call)
    flat, trend = out["flat"], out["trend"]
    if numpy.ndim(flux_batch) == 1:
        flat, trend = flat[0], None if trend is None else trend[0]
    return (flat, trend) if return_trend else flat


# ---- detrending: a time-windowed biweight on the device ------------------------------------------------------------------
class Biweight(collections.namedtuple("Biweight", ("window_length", "break_tolerance"))):
    """detrend=Biweight(window_length, break_tolerance=0.5) on the survey calls: Tukey's biweight over windows of
    window_length days, split at gaps > break_tolerance days (biweight_batch).  An immutable value; its fields are checked
    where it is used."""
    __slots__ = ()

    def __new__(cls, window_length, break_tolerance=0.5):
        return super(Biweight, cls).__new__(cls, window_length, break_tolerance)


def biweight_batch(t, flux_batch, window_length=0.5, break_tolerance=0.5, return_trend=False, context=None, device=None,
                   devices=None, mask=None, min_points=3, return_status=False):
    """flat = flux / trend for every row of flux_batch ([n] or [n_curves, n], at the shared time stamps t), with trend Tukey's
    biweight location over a window in TIME, on the device (tls_biweight_detrend): the robust filter the detrending comparison
    of Hippke et al. 2019 (AJ 158, 143) recommends in front of a transit search, with window_length about three times the
    longest transit duration searched for.

    A new segment starts behind every gap t[j] - t[j-1] > break_tolerance (days; inf: never), and the window of point i is
    every point of i's segment with |t[j] - t[i]| <= window_length / 2 (days), so no window reaches across a gap and the ends
    of a row carry no padding.  Inside the window the location starts at the median and is reweighted up to
    BIWEIGHT_MAX_ITER = 50 times with the biweight of tuning constant C = 5 around the MAD, until it moves by at most
    FTOL = 1e-6 of itself (a relative tolerance: rows near 1e-300 and 1e300 behave like rows near 1) or the MAD is 0.  The
    exact steps are in include/tls_amd.h; each is one IEEE double operation, so the result is bit-equal to a numpy
    restatement of them.  t must be finite and non-decreasing, window_length finite and > 0, break_tolerance > 0, no window
    may hold more than BIWEIGHT_MAX_WINDOW = 4095 points, and every flux value must be finite and > 0.  The arguments are
    checked before any device work.

    mask (uint8 or bool, flux_batch's shape, anything but 0: protected; None: today's call, untouched) leaves the protected
    points -- the transits of a first search, transit_mask -- out of every fit (tls_biweight_detrend_masked).  The windows
    stay those of t; the members of a window are its unprotected points.  A window with at least min_points (>= 1) members
    -- or with all of its points, where it holds fewer than min_points -- gets their biweight location by the same loop
    (status 0).  Any other point is open: its trend is interpolated linearly in
    t between the nearest status-0 points to its left and right inside its segment, or taken from the one there is (status 1);
    where the whole segment is open the point gets the plain biweight of its own window, the mask ignored (status 2), so the
    trend is always defined.  flat = flux / trend at every point, the protected ones included.  An all-zero mask returns the
    unmasked call's bits.  return_status=True (with a mask) appends the status rows (uint8).

    devices=[...] deals the rows out over several GPUs, as the other survey calls (the mask rows with them).  Returns flat, or
    (flat[, trend][, status]), in the shape of flux_batch."""
    from ._lib import biweight_arguments, biweight_masked_arguments
    if mask is None:
        if return_status:
            raise ValueError("return_status=True needs a mask")
        t, rows, wl, bt = biweight_arguments(t, flux_batch, window_length, break_tolerance)

        def call(ctx, lo, hi):
            out = ctx.biweight_detrend(t, rows[lo:hi], wl, bt, return_trend=return_trend)
            return dict(flat=out[0], trend=out[1]) if return_trend else dict(flat=out, trend=None)

        out = _run_batch(devices, device, context, len(rows), call)
        flat, trend = out["flat"], out["trend"]
        if numpy.ndim(flux_batch) == 1:
            flat, trend = flat[0], None if trend is None else trend[0]
        return (flat, trend) if return_trend else flat
    t, rows, mk, wl, bt, low = biweight_masked_arguments(t, flux_batch, mask, window_length, break_tolerance, min_points)

    def call(ctx, lo, hi):
        flat, trend, status = ctx.biweight_detrend_masked(t, rows[lo:hi], mk[lo:hi], wl, bt, low, return_trend=True,
                                                          return_status=True)
        return dict(flat=flat, trend=trend, status=status)

    out = _run_batch(devices, device, context, len(rows), call)
    res = (out["flat"],) + ((out["trend"],) if return_trend else ()) + ((out["status"],) if return_status else ())
    if numpy.ndim(flux_batch) == 1:
        res = tuple(v[0] for v in res)
    return res[0] if len(res) == 1 else res


# ---- detrending with the transits protected: the in-transit flags of a batch ----------------------------------------------
def transit_mask(t, period, T0, duration, curve=None, n_curves=None, factor=1.5, context=None, device=None):
    """The in-transit flags of a batch, uint8 [n_curves, len(t)] with 1 = protected, on the device (tls_transit_mask): what
    biweight_batch(mask=), prewhiten_batch(mask=) and detrend_mask= of the survey calls take.  Candidate k -- period[k], T0[k],
    duration[k] (days), of curve curve[k] (None: candidate k belongs to curve k) -- protects the points of its curve with

        d = t[i] - T0;  e = floor(d / period + 0.5);  r = d - e * period;  abs(r) <= 0.5 * (factor * duration)

    one IEEE double operation a step, so the flags equal tests/transit_protect_spec.py's bit for bit.  A curve may have any
    number of candidates, in any order, or none; a candidate whose period, T0 or duration is not finite, or whose period or
    duration is not > 0, is skipped silently (the NaN rows of a peaks array can be passed as they are).  n_curves None: the
    number of candidates without curve, max(curve) + 1 with.  ValueError, before any device work, for shapes that disagree, a
    non-finite t, a curve outside [0, n_curves) and a factor that is not finite and > 0."""
    from ._lib import transit_mask_arguments
    a = transit_mask_arguments(t, period, T0, duration, curve, n_curves, factor)
    ctx = context if context is not None else _search.default_context(device)
    return ctx.transit_mask(a["t"], a["period"], a["T0"], a["duration"], a["curve"], a["n_curves"], a["factor"])


# ---- detrending: SysRem, the systematics the batch shares, fitted across its rows on the device ---------------------------
class SysRem(collections.namedtuple("SysRem", ("n_components", "max_iter", "tol"))):
    """detrend=SysRem(n_components=1, max_iter=50, tol=1e-6) on search_batch, power_batch and power_results: the shared
    systematics of the WHOLE batch fitted across its rows and divided out (sysrem_batch).  An immutable value; its fields
    are checked where it is used."""
    __slots__ = ()

    def __new__(cls, n_components=1, max_iter=50, tol=1e-6):
        return super(SysRem, cls).__new__(cls, n_components, max_iter, tol)


def sysrem_batch(flux_batch, n_components=1, dy_batch=None, max_iter=50, tol=1e-6, return_trend=False,
                 return_components=False, context=None, device=None):
    """flat = flux / trend for the rows of flux_batch [n_curves, n] on shared epochs, with trend the systematics the rows
    SHARE, fitted across them on the device (tls_sysrem): SysRem (Tamuz, Mazeh & Zucker 2005), the ensemble step of WASP, HAT,
    NGTS and the Kepler / TESS cotrending.  Pointing jitter, momentum dumps, thermal ramps and airmass reach every star at the
    same epochs, each with its own strength; a per-row filter (detrend_batch, biweight_batch) cannot tell such an event from
    a transit of the same length, a fit across the rows can.

    With x_ij = flux_ij / mean_i - 1, every component is a rank-1 term c_i a_j (star coefficient times epoch profile) fitted
    by alternating weighted least squares from c = 1 -- a_j = sum_i x c w / sum_i c c w, then c_i = sum_j x a w / sum_j a a w
    -- until a moves by at most tol of its largest value, or max_iter iterations; it is subtracted from x before the next
    one.  The weights are 1 / (dy / mean)^2 with a dy_batch, otherwise one weight a row, 1 / mean(x_i^2) (a constant row
    carries none and comes out as flux / mean).  trend_ij = mean_i (1 + sum_k c_ik a_kj).  The exact steps and both summation
    orders are in include/tls_amd.h; each step is one IEEE double operation, so the result is bit-equal to a numpy restatement
    of them, the iteration counts included.  n_components is in [1, min(SYSREM_MAX_COMPONENTS = 8, n_curves - 1)], max_iter
    in [1, SYSREM_MAX_ITER = 1000], tol finite and >= 0, and every flux and dy value finite and > 0; the arguments are checked
    before any device work.  A star's own variability is not modelled: a strongly variable star pulls a component towards
    itself.

    The fit spans the batch, so it runs on ONE device (context, or device's default context) and takes no devices=.  Returns
    flat[, trend][, (c [n_curves, K], a [K, n], iters [K])]."""
    from ._lib import sysrem_arguments
    rows, dy, k, iters, tol = sysrem_arguments(flux_batch, n_components, dy_batch, max_iter, tol)
    ctx = context if context is not None else _search.default_context(device)
    return ctx.sysrem(rows, k, dy=dy, max_iter=iters, tol=tol, return_trend=return_trend, return_components=return_components)


# ---- detrending: iterative sinusoid pre-whitening on the device -------------------------------------------------------------
class Prewhiten(collections.namedtuple("Prewhiten", ("n_terms", "harmonics", "min_power", "f_min", "f_max"))):
    """detrend=Prewhiten(n_terms=3, harmonics=1, min_power=None, f_min=None, f_max=None) on the survey calls: the n_terms
    strongest sinusoids of every row (each with `harmonics` harmonics) fitted and divided out (prewhiten_batch) on the part
    [f_min, f_max] (cycles a day; None: no cut) of variability_frequencies(t).  An immutable value; its fields are checked
    where it is used."""
    __slots__ = ()

    def __new__(cls, n_terms=3, harmonics=1, min_power=None, f_min=None, f_max=None):
        return super(Prewhiten, cls).__new__(cls, n_terms, harmonics, min_power, f_min, f_max)


def gls_power_threshold(n, n_freq, fap, oversampling=5):
    """The periodogram power that white noise exceeds somewhere on the grid with probability fap (Zechmeister & Kuerster 2009,
    eqs. 24-25, in the approximation fap = M Prob(p > P) for small values): 1 - (fap / M)^(2 / (n - 3)) with
    M = n_freq / oversampling independent frequencies among the n_freq of a grid oversampled `oversampling` times.  Host
    only; a min_power for prewhiten_batch.  ValueError unless n > 3 is an integer, n_freq >= 1, oversampling is finite and > 0
    and 0 < fap <= M."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n <= 3:
        raise ValueError("gls_power_threshold: n must be an integer > 3, got %r" % (n,))
    if isinstance(n_freq, bool) or not isinstance(n_freq, numbers.Integral) or n_freq < 1:
        raise ValueError("gls_power_threshold: n_freq must be an integer >= 1, got %r" % (n_freq,))
    if isinstance(oversampling, bool) or not isinstance(oversampling, numbers.Real) or not (0.0 < float(oversampling) < numpy.inf):
        raise ValueError("gls_power_threshold: oversampling must be finite and > 0, got %r" % (oversampling,))
    m = float(n_freq) / float(oversampling)
    if isinstance(fap, bool) or not isinstance(fap, numbers.Real) or not (0.0 < float(fap) <= m):
        raise ValueError("gls_power_threshold: fap must lie in (0, n_freq / oversampling], got %r" % (fap,))
    return 1.0 - (float(fap) / m) ** (2.0 / (int(n) - 3.0))


PREWHITEN_FAP = 1e-3   # the false-alarm probability behind prewhiten_batch's default min_power


def prewhiten_term_fields():
    """The fields of a pre-whitening term, in order (tls_prewhiten_term of include/tls_amd.h): what
    prewhiten_batch(..., return_terms=True) returns for every (curve, iteration, harmonic)."""
    from ._lib import PREWHITEN_FIELDS
    return PREWHITEN_FIELDS


def _prewhiten_grid(t, f_min=None, f_max=None):
    """variability_frequencies(t) cut to [f_min, f_max] (None: no cut).  ValueError for a bound that is not a finite number
    > 0, and for a cut that leaves no frequency."""
    grid = variability_frequencies(t)
    for name, bound in (("f_min", f_min), ("f_max", f_max)):
        if bound is not None and (isinstance(bound, bool) or not isinstance(bound, numbers.Real) or not (0.0 < float(bound) < numpy.inf)):
            raise ValueError("prewhiten: %s must be None or finite and > 0, got %r" % (name, bound))
    if f_min is not None:
        grid = grid[grid >= float(f_min)]
    if f_max is not None:
        grid = grid[grid <= float(f_max)]
    if not len(grid):
        raise ValueError("prewhiten: no frequency of variability_frequencies(t) lies in [f_min, f_max] = [%r, %r]" % (f_min, f_max))
    return grid


def _prewhiten_step(t, step, n):
    """(frequencies, n_terms, harmonics, min_power) of a Prewhiten step on rows of n points over t: the grid cut, and the
    default min_power (gls_power_threshold at PREWHITEN_FAP) where the step names none."""
    grid = _prewhiten_grid(t, step.f_min, step.f_max)
    low = step.min_power
    if low is None:
        low = gls_power_threshold(n, len(grid), PREWHITEN_FAP) if n > 3 else 1.0
    return grid, step.n_terms, step.harmonics, low


def prewhiten_batch(t, flux_batch, n_terms=3, harmonics=1, min_power=None, frequencies=None, dy_batch=None, return_trend=False,
                    return_terms=False, context=None, device=None, devices=None, mask=None):
    """flat = flux / trend for every row of flux_batch ([n] or [n_curves, n], at the shared ascending time stamps t), with
    trend the row's mean plus its n_terms strongest sinusoids, found and fitted one after the other on the device
    (tls_prewhiten): iterative pre-whitening, the harmonic remover of the Kepler TPS and of Period04.  It is the detrender
    for variability FASTER than a transit -- delta Scuti and gamma Dor pulsations, a contact binary next door, rapid
    rotation -- which no median or biweight window can follow without flattening the transit too.

        r = flux; iteration j = 0 .. n_terms - 1, while the row runs:
            the periodogram of lomb_scargle of r on `frequencies` (None: variability_frequencies(t))
            k = the first index of the highest finite power; none (a constant row): status 2, stop;
            power[k] < min_power: status 1, stop
            f* = the vertex of the parabola through the powers at k - 1, k, k + 1 (f[k] itself at the ends of the grid, next
            to a NaN, and where the three do not curve downwards)
            for h = 1 .. harmonics: the weighted least-squares sinusoid with a floating mean at h f* (the sine test's sums
            over 256 lanes) is fitted to r and subtracted from it:  r_i -= ca (cos phi_i - C) + sa (sin phi_i - S)
        trend = ybar_0 + everything subtracted;  flat = flux / trend

    The exact steps are in include/tls_amd.h and tests/prewhiten_spec.py; each is one IEEE double operation.  The rows stay on
    the device for the whole call: an iteration is one dense product of the rows, the periodogram's epilogue and one step
    kernel, and the host reads a single count per iteration to stop when no row runs any more.

    min_power None: gls_power_threshold(n, F, fap=PREWHITEN_FAP = 1e-3), the power white noise reaches on the grid once in a
    thousand curves, so that noise alone has nothing removed.  WITHOUT A MASK THE TRANSIT IS NOT PROTECTED: a box transit is itself periodic
    (a 0.5 % transit of 3.3 d in 30 d of 3e-4 noise has periodogram power 0.07, well above that default), and once the
    stellar terms are gone the next term lands on the transit's period or a harmonic of it and removes part of the depth.
    Keep n_terms at the number of stellar signals, or keep the grid away from planetary periods with `frequencies` (or
    Prewhiten's f_min); DESIGN.md "Pre-whitening" has the measured depth kept in each case.  dy_batch: per-point errors (None:
    uniform weights).

    mask (uint8 or bool, flux_batch's shape, anything but 0: protected; None: the call above, untouched) is the remedy where
    the transits are known from a first search (transit_mask): a protected point has weight 0.0 in the mean, the variance, the
    periodogram, the pick and the sinusoid fit (tls_prewhiten_masked; elsewhere 1 / dy^2, or 1.0, normalised to sum 1), so no
    term can land on the transit; the subtraction and the trend still cover EVERY point.  A row with fewer than 3 unprotected
    points has nothing removed (status 2).  The default min_power keeps using n = len(t).

    ValueError, before any device work, for non-finite input, a t that is not ascending, frequencies that are not finite and
    > 0, n < 3, n_terms outside [1, 32], harmonics outside [1, 8], min_power outside [0, 1] and shapes that disagree.
    devices=[...] deals the rows out over several GPUs, as the other survey calls.  Returns flat[, trend][, info] in the shape
    of flux_batch; info (return_terms=True) is a dict: terms (a record array [n_curves, n_terms, harmonics] with the fields of
    prewhiten_term_fields(); status 0 fitted, 1 skipped, 2 not reached), n_iterations and status [n_curves]."""
    from ._lib import prewhiten_arguments
    if frequencies is None:
        frequencies = variability_frequencies(t)
    n = numpy.shape(flux_batch)[-1] if numpy.ndim(flux_batch) else 0
    if min_power is None:
        min_power = gls_power_threshold(int(n), len(frequencies), PREWHITEN_FAP) if n > 3 else 1.0
    a = prewhiten_arguments(t, flux_batch, dy_batch, frequencies, n_terms, harmonics, min_power)
    if mask is not None:
        from ._lib import detrend_mask_rows
        mask = detrend_mask_rows(mask, a["y"].shape)

    def call(ctx, lo, hi):
        dy = None if a["dy"] is None else a["dy"][lo:hi]
        if mask is None:
            out = ctx.prewhiten(a["t"], a["y"][lo:hi], a["frequencies"], a["n_terms"], a["harmonics"], a["min_power"], dy=dy,
                                return_trend=True, return_terms=True)
        else:
            out = ctx.prewhiten_masked(a["t"], a["y"][lo:hi], mask[lo:hi], a["frequencies"], a["n_terms"], a["harmonics"],
                                       a["min_power"], dy=dy, return_trend=True, return_terms=True)
        return dict(flat=out[0], trend=out[1], **out[2])

    out = _run_batch(devices, device, context, len(a["y"]), call)
    flat, trend = out["flat"], out["trend"]
    info = dict(terms=out["terms"], n_iterations=out["n_iterations"], status=out["status"])
    if numpy.ndim(flux_batch) == 1:
        flat, trend = flat[0], trend[0]
        info = {k: v[0] for k, v in info.items()}
    res = (flat,) + ((trend,) if return_trend else ()) + ((info,) if return_terms else ())
    return res[0] if len(res) == 1 else res


# ---- detrending: regression against centroids and basis vectors on the device -----------------------------------------------
class Decorrelate(collections.namedtuple("Decorrelate", ("own", "shared", "segments", "ridge", "n_iter", "sigma_upper",
                                                         "sigma_lower"))):
    """detrend=Decorrelate(own=None, shared=None, segments=None, ridge=0.0, n_iter=3, sigma_upper=5.0, sigma_lower=5.0) on
    the survey calls: every row regressed on its own columns own [n_curves, n_own, n] (centroid_regressors) and on the shared
    columns shared [n_shared, n] (basis vectors) and divided by the fit (decorrelate_batch), weighted with dy_batch where one
    is given and with detrend_mask as its mask.  An immutable value; its fields are checked where it is used."""
    __slots__ = ()

    def __new__(cls, own=None, shared=None, segments=None, ridge=0.0, n_iter=3, sigma_upper=5.0, sigma_lower=5.0):
        return super(Decorrelate, cls).__new__(cls, own, shared, segments, ridge, n_iter, sigma_upper, sigma_lower)


def decorrelate_fields():
    """The fields of a decorrelation record, in order (tls_decor_fit of include/tls_amd.h): what
    decorrelate_batch(..., return_fit=True) returns as `record` for every (curve, segment)."""
    from ._lib import DECOR_FIELDS
    return DECOR_FIELDS


def centroid_regressors(cx_batch, cy_batch, order=2):
    """The columns a centroid regression takes as `own`: [n_curves, n_terms, n] (one row [n]: [n_terms, n]) monomials
    x^a y^b with 1 <= a + b <= order of x = cx - median(cx) and y = cy - median(cy), each row's own medians.  The terms run
    by total degree, and within a degree from the highest power of x down: x, y | x^2, x y, y^2 | x^3, x^2 y, x y^2, y^3;
    order (1, 2 or 3) gives 2, 5 or 9 of them.  ValueError unless cx_batch and cy_batch are finite and of one shape [n] or
    [n_curves, n].  Host only."""
    order = _checks.integer("centroid regressors", "order", order, 1, 3)
    try:
        cx, cy = numpy.asarray(cx_batch, dtype=numpy.float64), numpy.asarray(cy_batch, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise _checks.refusal("centroid regressors", "cx_batch and cy_batch must hold numbers")
    if cx.ndim not in (1, 2) or cx.shape != cy.shape or cx.shape[-1] < 1:
        raise _checks.refusal("centroid regressors", "cx_batch and cy_batch must share one shape [n] or [n_curves, n], got %s "
                              "and %s" % (cx.shape, cy.shape))
    if not (numpy.all(numpy.isfinite(cx)) and numpy.all(numpy.isfinite(cy))):
        raise _checks.refusal("centroid regressors", "cx_batch and cy_batch must be finite")
    x = cx - numpy.median(cx, axis=-1, keepdims=True)
    y = cy - numpy.median(cy, axis=-1, keepdims=True)
    terms = [x ** a * y ** (d - a) for d in range(1, order + 1) for a in range(d, -1, -1)]
    return numpy.ascontiguousarray(numpy.stack(terms, axis=-2))


def decorrelate_segments(t, break_tolerance=0.5, window_length=None):
    """The index boundaries decorrelate_batch takes as `segments` (int64, from 0 to len(t)): a new segment starts behind every
    gap t[i] - t[i - 1] > break_tolerance; with a window_length every segment of span D = t[last] - t[first] is further cut
    into k = ceil(D / window_length) parts of equal duration D / k (part i starts at the first stamp >= t[first] + i D / k;
    a part without a stamp is left out).  ValueError unless t is [n], n >= 1, finite and non-decreasing, break_tolerance is
    a number > 0 and window_length is None or finite and > 0.  Host only."""
    what = "decorrelation segments"
    t = _checks.times(what, t, _checks.MAX_ROW_POINTS)
    _checks.positive(what, "break_tolerance", break_tolerance)
    if window_length is not None:
        window_length = _checks.finite_positive(what, "window_length", window_length, "must be None or finite and > 0")
    n = len(t)
    starts = numpy.concatenate([[0], 1 + numpy.flatnonzero(t[1:] - t[:-1] > break_tolerance), [n]])
    edges = []
    for a, b in zip(starts[:-1], starts[1:]):
        edges.append(int(a))
        span = t[b - 1] - t[a]
        if window_length is not None and span > window_length:
            k = int(numpy.ceil(span / window_length))
            cuts = a + numpy.searchsorted(t[a:b], t[a] + numpy.arange(1, k) * (span / k), side="left")
            edges.extend(int(c) for c in cuts)
    return numpy.unique(numpy.array(edges + [n], dtype=numpy.int64))


def decorrelate_batch(flux_batch, own=None, shared=None, dy_batch=None, mask=None, segments=None, ridge=0.0, n_iter=3,
                      sigma_upper=5.0, sigma_lower=5.0, return_trend=False, return_fit=False, context=None, device=None,
                      devices=None):
    """flat = flux / trend for every row of flux_batch [n_curves, n] (one row [n] is accepted, with own [n_own, n]), with
    trend a weighted, robust linear least-squares fit of the row against series that are KNOWN to drive its systematics
    (tls_decorrelate): the regression of K2SFF, K2SC and EVEREST on the centroids, and of the Kepler / TESS pipelines on
    their cotrending basis vectors.  The K2 roll moves the photocentre over the pixel sensitivity in a six-hour sawtooth as
    long as a transit, with a shape of its own for every star: no per-row window (detrend_batch, biweight_batch) can follow
    it without flattening the transit and no rank-1 term (sysrem_batch) describes it; a polynomial in the centroids does.

    The columns of a row are shared [n_shared, n] (every row takes them: basis vectors, or the profiles
    sysrem_batch(return_components=True) returned for another ensemble) and then its own, own [n_curves, n_own, n]
    (centroid_regressors); at least one of the two, and n_shared + n_own in [1, DECOR_MAX_TERMS = 16].  The mean is always
    free.  segments (decorrelate_segments; None: one segment) are index boundaries from 0 to n shared by all rows: every
    (row, segment) is fitted on its own.  The fit: z = flux / mu - 1 against the standardised columns by the normal equations
    (ridge * sum(w) added to the diagonal) and a Cholesky factorisation that drops a constant column and one collinear with
    those before it (pivot <= DECOR_PIVOT = 1e-10 of its diagonal entry); then up to n_iter (in [0, DECOR_MAX_ITER = 16])
    rounds in which the points with a residual above sigma_upper or below -sigma_lower weighted rms leave the fit and it is
    repeated (inf switches a side off).  dy_batch gives the weights 1 / dy^2 (None: 1).  mask ([n_curves, n] uint8 or bool,
    != 0: protected; transit_mask) keeps points out of the fit; trend and flat cover EVERY point, protected and clipped ones
    included, and a mask of zeros changes no bit.  The exact steps are in include/tls_amd.h and tests/decorrelate_spec.py;
    each is one IEEE double operation and every sum runs left to right, so the result equals the Python statement bit for bit.
    The arguments are checked before any device work (ValueError).

    devices=[...] deals the rows out, with their own, dy and mask rows beside them; every device gets shared.  Returns
    flat[, trend][, fit]: fit is a dict with `record` ([n_curves, n_seg] of decorrelate_fields(): status 0 fitted, 1 too few
    points (trend = mu), 2 the trend left (0, inf) (trend = mu); dropped, a bit a dropped column; n_fit, n_clipped, rounds, mu,
    sigma, n_live), `coef`, `mean` and `scale` [n_curves, n_seg, m] of the standardised columns, `coefficients` = coef / scale
    in the units of the raw columns, and `segments`."""
    from ._lib import decorrelate_arguments
    a = decorrelate_arguments(flux_batch, own, shared, dy_batch, mask, segments, ridge, n_iter, sigma_upper, sigma_lower)

    def call(ctx, lo, hi):
        flat, trend, fit = ctx.decorrelate(
            a["y"][lo:hi], a["own"][lo:hi] if a["own"].shape[1] else None, a["shared"] if len(a["shared"]) else None,
            None if a["dy"] is None else a["dy"][lo:hi], None if a["mask"] is None else a["mask"][lo:hi], a["segments"],
            a["ridge"], a["n_iter"], a["sigma_upper"], a["sigma_lower"], return_trend=True, return_fit=True)
        del fit["segments"]
        return dict(flat=flat, trend=trend, **fit)

    out = _run_batch(devices, device, context, len(a["y"]), call)
    flat, trend = out["flat"], out["trend"]
    fit = {k: out[k] for k in ("record", "coef", "mean", "scale", "coefficients")}
    fit["segments"] = a["segments"]
    if a["single"]:
        flat, trend = flat[0], trend[0]
        fit = {k: (v if k == "segments" else v[0]) for k, v in fit.items()}
    res = (flat,) + ((trend,) if return_trend else ()) + ((fit,) if return_fit else ())
    return res[0] if len(res) == 1 else res


# ---- detrending: a robust B-spline with a BIC-chosen knot spacing on the device ----------------------------------------------
class Spline(collections.namedtuple("Spline", ("knot_spacing", "break_tolerance", "penalty", "n_iter", "sigma_upper",
                                               "sigma_lower"))):
    """detrend=Spline(knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0) on the
    survey calls: a penalised cubic B-spline fitted robustly to every gap-free segment of every row and divided out
    (spline_batch), weighted with dy_batch where one is given and with detrend_mask as its mask.  knot_spacing may be a
    sequence: every row then takes the spacing of its own least BIC.  An immutable value; its fields are checked where it is
    used."""
    __slots__ = ()

    def __new__(cls, knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0):
        return super(Spline, cls).__new__(cls, knot_spacing, break_tolerance, penalty, n_iter, sigma_upper, sigma_lower)


def spline_fields():
    """(the fields of a segment record, the fields of a curve record) of spline_batch(..., return_fit=True), in order
    (tls_spline_segment and tls_spline_curve of include/tls_amd.h); `bic` holds SPLINE_MAX_SPACINGS values."""
    from ._lib import SPLINE_CURVE_FIELDS, SPLINE_SEGMENT_FIELDS
    return SPLINE_SEGMENT_FIELDS, SPLINE_CURVE_FIELDS


def spline_spacings(t, shortest=0.5, longest=20.0, count=8):
    """The logarithmic ladder of knot spacings of Shallue & Vanderburg (2018): `count` values from `shortest` to `longest`
    days, the longest cut to the span of t.  ValueError unless t is finite and non-decreasing, 0 < shortest <= longest < inf
    and count is an integer in [1, SPLINE_MAX_SPACINGS].  Host only."""
    from ._lib import SPLINE_MAX_SPACINGS
    what = "spline spacings"
    t = _checks.times(what, t, _checks.MAX_ROW_POINTS)
    shortest = _checks.finite_positive(what, "shortest", shortest)
    longest = _checks.finite_positive(what, "longest", longest)
    if longest < shortest:
        raise _checks.refusal(what, "longest must be >= shortest, got %r < %r" % (longest, shortest))
    count = _checks.integer(what, "count", count, 1, SPLINE_MAX_SPACINGS)
    span = float(t[-1] - t[0])
    if span > shortest:
        longest = min(longest, span)
    return numpy.logspace(numpy.log10(shortest), numpy.log10(longest), count)


def spline_batch(t, flux_batch, knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0,
                 dy_batch=None, mask=None, return_trend=False, return_fit=False, context=None, device=None, devices=None):
    """flat = flux / trend for every row of flux_batch ([n] or [n_curves, n], at the shared time stamps t), with trend a cubic
    B-spline on uniform knots fitted to every gap-free segment by penalised, iteratively sigma-clipped least squares, on the
    device (tls_spline_detrend): the "Kepler spline" of Vanderburg & Johnson (2014) and Shallue & Vanderburg (2018), the
    detrender of the TESS Quick-Look Pipeline, wotan's pspline / rspline.  A smooth basis over the whole segment follows a
    star that rotates in a few days without being shortened until it eats the transit, which a sliding window cannot.

    A new segment starts behind every gap t[j] - t[j-1] > break_tolerance (days; inf: never).  A segment of span T takes
    q = max(1, ceil(T / knot_spacing)) equal intervals and q + 3 coefficients (at most SPLINE_MAX_COEF = 512).  The normal
    equations are banded (half-bandwidth 3); penalty * (sum w / q) times the squared second differences of the coefficients is
    added, so that empty intervals (a short gap, a masked transit) leave the system positive definite; a banded Cholesky
    solves it.  Then up to n_iter (in [0, SPLINE_MAX_ITER = 16]) clip rounds: sigma = 1.4826 MAD of the members' residuals,
    members above sigma_upper sigma or below -sigma_lower sigma leave (inf switches a side off), and the segment is fitted
    again, until a round drops nobody or would leave fewer than two members.  dy_batch gives the weights 1 / dy^2 (None: 1).
    mask ([n_curves, n] uint8 or bool, != 0: protected; transit_mask) keeps points out of every fit; trend and flat cover EVERY
    point, and a mask of zeros changes no bit.  A segment without two members at distinct time stamps (status 1), or whose
    band has no pivot or whose trend leaves (0, inf) (status 2), gets the weighted mean as its trend, so the trend is always
    finite and > 0.

    knot_spacing may be a sequence of at most SPLINE_MAX_SPACINGS = 16 (spline_spacings): every row then gets the spacing
    whose fit has the least Bayesian information criterion K log(N) + SSR / sigma_pp^2, with K the coefficients, N the
    members left, SSR the weighted residual sum over the mean weight and sigma_pp the point-to-point scatter of the row.  The
    exact steps are in include/tls_amd.h and tests/spline_spec.py; each but the BIC's log is one IEEE double operation in a
    stated order, so flat, trend and the segment records equal the Python statement bit for bit.  The arguments are checked
    before any device work (ValueError).

    devices=[...] deals the rows out, with their dy and mask rows.  Returns flat[, trend][, fit]: fit is a dict with `segment`
    ([n_curves, n_seg] of spline_fields()[0]: status, intervals, coefficients, points, kept, rounds, dropped, sigma, ssr,
    weight), `curve` ([n_curves] of spline_fields()[1]: choice, sigma_pp, flag, bic [16]), `segments` (index boundaries) and
    `spacings`."""
    from ._lib import spline_arguments
    a = spline_arguments(t, flux_batch, knot_spacing, break_tolerance, penalty, n_iter, sigma_upper, sigma_lower, dy_batch, mask)
    spacing = float(a["spacings"][0]) if a["one_spacing"] else a["spacings"]

    def call(ctx, lo, hi):
        flat, trend, fit = ctx.spline_detrend(
            a["t"], a["y"][lo:hi], spacing, a["break_tolerance"], a["penalty"], a["n_iter"], a["sigma_upper"], a["sigma_lower"],
            None if a["dy"] is None else a["dy"][lo:hi], None if a["mask"] is None else a["mask"][lo:hi], return_trend=True,
            return_fit=True)
        return dict(flat=flat, trend=trend, segment=fit["segment"], curve=fit["curve"])

    out = _run_batch(devices, device, context, len(a["y"]), call)
    flat, trend = out["flat"], out["trend"]
    fit = {"segment": out["segment"], "curve": out["curve"], "segments": a["segments"], "spacings": a["spacings"]}
    if a["single"]:
        flat, trend = flat[0], trend[0]
        fit["segment"], fit["curve"] = fit["segment"][0], fit["curve"][0]
    res = (flat,) + ((trend,) if return_trend else ()) + ((fit,) if return_fit else ())
    return res[0] if len(res) == 1 else res


# ---- cleaning: missing points and outliers flagged and repaired on the device -----------------------------------------------
class Clean(collections.namedtuple("Clean", ("window_length", "sigma_upper", "sigma_lower", "max_run", "n_iter", "min_points",
                                             "break_tolerance"))):
    """detrend=Clean(window_length=None, sigma_upper=4.0, sigma_lower=inf, max_run=1, n_iter=3, min_points=3,
    break_tolerance=0.5) on the survey calls: the bad points of every row flagged and repaired (clean_batch), the repaired rows
    handed on.  As the FIRST step it admits rows with NaN, infinite and non-positive values, which every other call and step
    refuses.  It hands on no flags: later steps see the repaired rows and the caller's detrend_mask alone, and with
    detrend_mask it runs unmasked, as SysRem does.  For stars with trends: (Clean(sigma_upper=inf), <detrender>,
    Clean(None, 4.0)) -- repair, flatten, clip.  An immutable value; its fields are checked where it is used."""
    __slots__ = ()

    def __new__(cls, window_length=None, sigma_upper=4.0, sigma_lower=float("inf"), max_run=1, n_iter=3, min_points=3,
                break_tolerance=0.5):
        return super(Clean, cls).__new__(cls, window_length, sigma_upper, sigma_lower, max_run, n_iter, min_points,
                                         break_tolerance)


def _clean_step(step):
    """The keywords of clean_batch and Context.clean_rows of a Clean step."""
    return dict(window_length=step.window_length, break_tolerance=step.break_tolerance, sigma_upper=step.sigma_upper,
                sigma_lower=step.sigma_lower, max_run=step.max_run, n_iter=step.n_iter, min_points=step.min_points)


def clean_fields():
    """The fields of a record of clean_batch(..., return_record=True), in order (tls_clean_record of include/tls_amd.h)."""
    from ._lib import CLEAN_FIELDS
    return CLEAN_FIELDS


def clean_batch(t, flux_batch, window_length=None, break_tolerance=0.5, sigma_upper=4.0, sigma_lower=float("inf"), max_run=1,
                n_iter=3, min_points=3, bad=None, return_flags=False, return_record=False, context=None, device=None,
                devices=None):
    """The rows of flux_batch ([n] or [n_curves, n], at the shared time stamps t) with their bad points flagged and replaced
    with defined values, on the device (tls_clean_rows): the counterpart of the reference's cleaned_array and of a sigma clip
    that keeps every row on the shared time stamps, so that everything downstream keeps its plans.  flux_batch MAY hold NaN,
    infinities, zeros and negative values; bad ([n_curves, n] uint8 or bool, != 0) is the caller's quality flag.

    Flags (uint8 a point): 1 missing, not (isfinite(y) and y > 0), cleaned_array's conditions; 2 the caller's bad; 4 high
    outlier; 8 low outlier.  A point is valid while its flags are 0.  Up to n_iter (in [0, CLEAN_MAX_ITER = 16]) clip rounds
    run, none when both sigmas are inf.  A round forms a centre for every valid point -- window_length None: the median of the
    row's valid points; else the median of the valid points of its window OTHER THAN ITSELF (the biweight's windows: inside
    the segment, a new one behind every gap > break_tolerance days, within half a window_length; with fewer than min_points
    such members the point has no residual and cannot be flagged) -- the residuals r, c0 = median(r) and sigma = 1.4826
    median(|r - c0|).  Points with r - c0 > sigma_upper sigma are flagged high.  Points with r - c0 < -sigma_lower sigma are
    low candidates, and a candidate is flagged low only when its run -- the candidates that are neighbours among the valid
    points of one segment -- holds at most max_run of them: a single-sample glitch goes, a transit of many samples stays, and
    a missing sample inside a transit does not split it.  The rounds end after one that flags nothing; a round that would
    leave fewer than two valid points is not applied.  inf switches a side off (sigma_lower's default: a dip is what a
    search looks for).

    Repair: a flagged point between two valid points of its segment is interpolated linearly in time; with one valid
    neighbour it takes that value; a segment without a valid point takes the row's median of valid points; a row without one
    becomes all 1.0.  Valid points keep their bits, and the result is finite and > 0.  The exact steps are in
    include/tls_amd.h and tests/clean_spec.py; each is one IEEE double operation and the medians are selections, so rows,
    flags and records equal the Python statement bit for bit.

    A sliding centre on an UNDETRENDED fast rotator eats the shoulders of its transits (the centre lags the curvature there;
    DESIGN.md "Cleaning" has the counts): repair first, flatten, and clip the flattened rows --
    detrend=(Clean(sigma_upper=inf), <detrender>, Clean(None, 4.0)).  An interpolated point carries no noise: a row whose
    transits are mostly missing gains no depth, but its SDE is that of a slightly quieter row.

    devices=[...] deals the rows out, with their bad rows.  The arguments are checked before any device work (ValueError).
    Returns rows[, flags][, record]: record is a structured array [n_curves] of clean_fields() -- status (|= 1: a segment
    was filled from the row's median; 2: no valid point), n_missing, n_bad, n_high, n_low, n_filled, longest_run (consecutive
    filled indices), rounds, center and sigma of the last round (NaN: none)."""
    from ._lib import clean_arguments
    a = clean_arguments(t, flux_batch, window_length, break_tolerance, sigma_upper, sigma_lower, max_run, n_iter, min_points, bad)

    def call(ctx, lo, hi):
        rows, flags, record = ctx.clean_rows(
            a["t"], a["y"][lo:hi], a["window_length"], a["break_tolerance"], a["sigma_upper"], a["sigma_lower"], a["max_run"],
            a["n_iter"], a["min_points"], None if a["bad"] is None else a["bad"][lo:hi], return_flags=True, return_record=True)
        return dict(rows=rows, flags=flags, record=record)

    out = _run_batch(devices, device, context, len(a["y"]), call)
    rows, flags, record = out["rows"], out["flags"], out["record"]
    if a["single"]:
        rows, flags, record = rows[0], flags[0], record[0]
    res = (rows,) + ((flags,) if return_flags else ()) + ((record,) if return_record else ())
    return res[0] if len(res) == 1 else res


def align_rows(times, fluxes, t, tolerance=None):
    """Per-star series snapped onto a shared grid, on the host: the way from "my stars have their own time stamps and gaps" to
    clean_batch and power_batch.  times and fluxes: one (t_k, y_k) a star, t_k sorted (non-decreasing) and finite, y_k of its
    length (NaN allowed); t [n]: the shared grid, finite and strictly ascending.  Every sample goes to the nearest grid stamp
    if that lies within `tolerance` days (default: half the median step of t; the lower index wins a tie), else it is
    dropped.  A grid point takes the mean of its samples -- their sum in index order from 0.0, over their count -- and NaN
    where it has none.

    The time error: the samples are searched AT THE GRID'S time stamps.  Stars of one field share cadence numbers but not
    barycentric times: across a TESS camera the correction spreads by about 100 s, against a cadence of 120 s to 1800 s, across
    a Kepler module far less.  offset_mean is each star's mean t_sample - t_grid over the samples kept -- add it to a T0 found
    on the grid -- and offset_max the largest |t_sample - t_grid|, the error left in a single point.

    Returns (flux_batch [n_stars, n] with NaN where a star has no sample, n_dropped [n_stars] int64, offset_mean [n_stars],
    offset_max [n_stars]; NaN offsets for a star without a sample kept).  ValueError for shapes that disagree, a grid that is
    not finite and strictly ascending, time stamps of a star that are not finite and sorted, and a tolerance that is not
    finite and >= 0."""
    what = "align_rows"
    t = _checks.times(what, t, _checks.MAX_ROW_POINTS)
    n = len(t)
    if n > 1 and not numpy.all(t[1:] > t[:-1]):
        raise _checks.refusal(what, "the grid t must ascend strictly")
    if tolerance is None:
        tolerance = 0.5 * float(numpy.median(numpy.diff(t))) if n > 1 else 0.0
    tolerance = _checks.finite_at_least(what, "tolerance", tolerance)
    try:
        n_stars = len(times)
        same = n_stars == len(fluxes)
    except TypeError:
        raise _checks.refusal(what, "times and fluxes must be sequences with one entry a star")
    if not same:
        raise _checks.refusal(what, "times and fluxes must have one entry a star each, got %d and %d" % (n_stars, len(fluxes)))
    out = numpy.full((n_stars, n), numpy.nan)
    n_dropped = numpy.zeros(n_stars, dtype=numpy.int64)
    offset_mean, offset_max = numpy.full(n_stars, numpy.nan), numpy.full(n_stars, numpy.nan)
    for k in range(n_stars):
        tk = numpy.asarray(times[k], dtype=numpy.float64)
        yk = numpy.asarray(fluxes[k], dtype=numpy.float64)
        if tk.ndim != 1 or yk.shape != tk.shape:
            raise _checks.refusal(what, "star %d: time stamps and flux must be 1-d and of one length" % k)
        if not numpy.all(numpy.isfinite(tk)) or not numpy.all(tk[1:] >= tk[:-1]):
            raise _checks.refusal(what, "star %d: the time stamps must be finite and sorted" % k)
        if len(tk) == 0:
            continue
        right = numpy.clip(numpy.searchsorted(t, tk, side="left"), 0, n - 1)
        left = numpy.maximum(right - 1, 0)
        at = numpy.where(numpy.abs(tk - t[left]) <= numpy.abs(t[right] - tk), left, right)   # (the lower index wins a tie)
        off = tk - t[at]
        keep = numpy.abs(off) <= tolerance
        n_dropped[k] = int((~keep).sum())
        if not keep.any():
            continue
        at, off, y = at[keep], off[keep], yk[keep]
        total, count = numpy.zeros(n), numpy.zeros(n)
        numpy.add.at(total, at, y)                   # (unbuffered: a grid point's samples are added in index order)
        numpy.add.at(count, at, 1.0)
        hit = count > 0
        out[k, hit] = total[hit] / count[hit]
        offset_mean[k] = float(off.mean())
        offset_max[k] = float(numpy.abs(off).max())
    return out, n_dropped, offset_mean, offset_max


def _clean_first(t, flux_batch, detrend, context, device, devices):
    """(rows, the steps left) of the calls that check their rows before they detrend them: a Clean at the head of detrend is
    run here, so that the check sees the repaired rows; anything else comes back as it is."""
    steps = _detrend_steps(detrend)
    if not steps or not isinstance(steps[0], Clean):
        return flux_batch, detrend
    rows = clean_batch(t, flux_batch, context=context, device=device, devices=devices, **_clean_step(steps[0]))
    return rows, (steps[1:] or None)


def _detrend_steps(detrend):
    """The steps of a detrend= argument, left to right: () for None, the one step of an int, a Biweight, a SysRem or a
    Prewhiten, a Decorrelate, a Spline or a Clean, and the elements of a tuple or list of those."""
    if detrend is None:
        return ()
    if isinstance(detrend, (Biweight, SysRem, Prewhiten, Decorrelate, Spline, Clean)) or not isinstance(detrend, (tuple, list)):
        return (detrend,)
    for step in detrend:
        if step is None or (isinstance(step, (tuple, list)) and not isinstance(step, (Biweight, SysRem, Prewhiten, Decorrelate, Spline, Clean))):
            raise ValueError("a step of detrend must be a kernel size, a Biweight or a SysRem, got %r" % (step,))
    return tuple(detrend)


def _no_ensemble_step(detrend, caller):
    """ValueError for a SysRem among the steps of detrend, in the calls whose rows all come from ONE star."""
    if any(isinstance(step, SysRem) for step in _detrend_steps(detrend)):
        raise ValueError("%s forms its rows from ONE star, so a fit across the rows is meaningless there: detrend=SysRem "
                         "belongs on search_batch, power_batch and power_results" % caller)


def _no_regression_step(detrend, caller):
    """ValueError for a Decorrelate among the steps of detrend, in the calls that form their rows on the device from ONE
    star: a step's own columns belong to the rows of a batch the caller holds."""
    if any(isinstance(step, Decorrelate) for step in _detrend_steps(detrend)):
        raise ValueError("%s forms its rows on the device from ONE star and has no columns for them: detrend=Decorrelate "
                         "belongs on search_batch, power_batch, power_results and lomb_scargle; decorrelate the star's flux "
                         "with decorrelate_batch first" % caller)


def _detrend_of_rows(detrend, rows):
    """detrend as the curves `rows` (an index array) of the batch it was written for take it: every Decorrelate with the own
    columns of those curves, every other step as it is."""
    if not any(isinstance(step, Decorrelate) and step.own is not None for step in _detrend_steps(detrend)):
        return detrend
    steps = tuple(step._replace(own=numpy.asarray(step.own)[rows]) if isinstance(step, Decorrelate) and step.own is not None
                  else step for step in _detrend_steps(detrend))
    return steps[0] if isinstance(detrend, Decorrelate) else steps


def _first_context(context, device, devices, n_curves):
    """(context, lock) of the one device an ensemble step runs on: the given context, the first device of `devices` (with
    its group's lock), or device's default context."""
    kind, what = _resolve(devices, device, context, n_curves)
    if kind == "group":
        return what.contexts[0], what._lock
    return (context if context is not None else _search.default_context(what)), contextlib.nullcontext()


def _detrended(t, flux_batch, detrend, context, device, devices, dy_batch=None, detrend_mask=None):
    """flux_batch as it is (detrend None), or taken through the steps of detrend left to right on the call's devices for
    [n_curves, len(t)]: biweight_batch for a Biweight, the whole batch through SysRem on the first device (weighted with
    dy_batch where one is given) for a SysRem, prewhiten_batch (on variability_frequencies(t) cut to the step's range, weighted
    with dy_batch where one is given) for a Prewhiten, decorrelate_batch (weighted with dy_batch where one is given) for a
    Decorrelate, spline_batch (weighted likewise) for a Spline, detrend_batch(flux_batch, step) otherwise.  detrend_mask
    ([n_curves, len(t)], uint8 or bool) goes to every Biweight, Prewhiten, Decorrelate and Spline step as its mask; a SysRem step
    and a Clean step (clean_batch: the repaired rows go on, the flags do not) run unmasked, a median-filter
    step with a mask is a ValueError (before any step runs)."""
    steps = _detrend_steps(detrend)
    if detrend_mask is not None:
        from ._lib import detrend_mask_rows
        if numpy.ndim(flux_batch) != 2:
            raise ValueError("flux_batch must have shape [n_curves, len(t)]")
        detrend_mask = detrend_mask_rows(detrend_mask, numpy.shape(flux_batch), "detrend_mask")
        for step in steps:
            if not isinstance(step, (Biweight, SysRem, Prewhiten, Decorrelate, Spline, Clean)):
                raise ValueError("detrend_mask: the median filter (detrend=%r) is defined by its sample count and zero padding "
                                 "and has no masked form; use Biweight or Prewhiten steps with a mask" % (step,))
    if not steps:
        return flux_batch
    if numpy.ndim(flux_batch) != 2 or numpy.shape(flux_batch)[1] != len(t):
        raise ValueError("flux_batch must have shape [n_curves, len(t)]")
    for step in steps:
        if isinstance(step, SysRem):
            from ._lib import sysrem_arguments
            rows, dy, k, iters, tol = sysrem_arguments(flux_batch, step.n_components, dy_batch, step.max_iter, step.tol)
            ctx, lock = _first_context(context, device, devices, len(rows))
            with lock:
                flux_batch = ctx.sysrem(rows, k, dy=dy, max_iter=iters, tol=tol)
        elif isinstance(step, Biweight):
            flux_batch = biweight_batch(t, flux_batch, step.window_length, step.break_tolerance, context=context,
                                        device=device, devices=devices, mask=detrend_mask)
        elif isinstance(step, Prewhiten):
            grid, k, h, low = _prewhiten_step(t, step, len(t))
            flux_batch = prewhiten_batch(t, flux_batch, k, h, low, frequencies=grid, dy_batch=dy_batch, context=context,
                                         device=device, devices=devices, mask=detrend_mask)
        elif isinstance(step, Decorrelate):
            flux_batch = decorrelate_batch(flux_batch, step.own, step.shared, dy_batch, detrend_mask, step.segments, step.ridge,
                                           step.n_iter, step.sigma_upper, step.sigma_lower, context=context, device=device,
                                           devices=devices)
        elif isinstance(step, Spline):
            flux_batch = spline_batch(t, flux_batch, step.knot_spacing, step.break_tolerance, step.penalty, step.n_iter,
                                      step.sigma_upper, step.sigma_lower, dy_batch, detrend_mask, context=context, device=device,
                                      devices=devices)
        elif isinstance(step, Clean):                # (unmasked, and its flags are no mask for the steps behind it)
            flux_batch = clean_batch(t, flux_batch, context=context, device=device, devices=devices, **_clean_step(step))
        else:
            flux_batch = detrend_batch(flux_batch, step, context=context, device=device, devices=devices)
    return flux_batch


def _detrend_rows(ctx, t, rows, detrend):
    """rows as they are (detrend None), or taken through the per-row steps of detrend on ctx: the biweight for a Biweight,
    pre-whitening with uniform weights for a Prewhiten, the spline with uniform weights and no mask for a Spline, the
    cleaning stage for a Clean, the
    median filter of kernel size step otherwise (the rows formed on the device by injection_recovery and null_sde, chunk by
    chunk)."""
    for step in _detrend_steps(detrend):
        if isinstance(step, Biweight):
            rows = ctx.biweight_detrend(t, rows, step.window_length, step.break_tolerance)
        elif isinstance(step, Prewhiten):
            grid, k, h, low = _prewhiten_step(t, step, len(t))
            rows = ctx.prewhiten(t, rows, grid, k, h, low)
        elif isinstance(step, Spline):
            rows = ctx.spline_detrend(t, rows, *step)
        elif isinstance(step, Clean):
            rows = ctx.clean_rows(t, rows, **_clean_step(step))
        else:
            rows = ctx.medfilt_detrend(rows, step)
    return rows


def _candidate_rows(what, t, flux_batch, dy_batch=None):
    """(t as float64, flux_batch, dy_batch) of a stand-alone candidate entry: one row [n] brought to [1, n]; ValueError
    unless flux_batch is [n_curves, n] over t [n] and t is finite and non-decreasing (that message headed `what`)."""
    t = numpy.asarray(t, dtype=numpy.float64)
    if numpy.ndim(flux_batch) == 1:
        flux_batch = numpy.asarray(flux_batch)[None, :]
        dy_batch = None if dy_batch is None else numpy.asarray(dy_batch)[None, :]
    if numpy.ndim(flux_batch) != 2 or t.ndim != 1 or numpy.shape(flux_batch)[1] != len(t):
        raise _checks.over_t(None, "flux_batch")
    _checks.time_values(what, t)
    return t, flux_batch, dy_batch


def _candidate_inputs(t, flux_batch, dy_batch, detrend, context, device, template_kwargs):
    """(inp, y_rows, dy_rows, ctx) of a stand-alone candidate entry, behind its argument checks: the rows detrended on the
    call's device, the plan inputs a search of them gets (_batch_inputs) and the context."""
    flux_batch = _detrended(t, flux_batch, detrend, context, device, None, dy_batch)
    kwargs = dict(template_kwargs)
    kwargs.setdefault("oversampling_factor", 1)      # (the period grid of the plan inputs is not used: the coarsest will do)
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, kwargs)
    return inp, y_rows, dy_rows, context if context is not None else _search.default_context(device)


# the period ratios whose neighbourhoods a taken peak suppresses by default: its first harmonics and sub-harmonics
HARMONICS = (0.5, 2.0, 1 / 3, 3.0, 2 / 3, 1.5)


def power_batch(t, flux_batch, dy_batch=None, context=None, device=None, with_arrays=False, devices=None, statistics=False,
                per_transit=False, models=False, detrend=None, peaks=None, peak_separation=0.02, peak_ratios=HARMONICS,
                peak_min_power=None, peak_fits=False, phase_scan=False, phase_scan_max_bins=4096, phase_scan_min_count=3,
                transit_times=False, transit_times_search=1.0, transit_times_min_ses=3.0, shape_fit=False,
                shape_fit_window=2.0, shape_fit_min_count=3, sine_test=False, sine_test_mask=1.5,
                sine_test_harmonics=(0.5, 1.0, 2.0), ephemeris_match=False, ephemeris_match_drift=0.5,
                ephemeris_match_epoch=0.5, ephemeris_match_max_ratio=3, views=False, views_global_bins=2001,
                views_local_bins=201, views_local_durations=4.0, views_local_width=0.16, event_vetting=False,
                event_vetting_search=1.0, event_vetting_chase_window=0.1, event_vetting_guard=1.5, event_vetting_min_ses=3.0,
                event_vetting_chase_fraction=0.6, event_vetting_chase_min=0.5, event_vetting_point_fraction=0.5,
                event_vetting_step_fraction=0.5, centroids=None, centroid_window=3.0, centroid_min_in=1,
                centroid_min_out=3, noise=None, detrend_mask=None, transit_fit=False, **power_kwargs):
    """Survey-mode power(): for every light curve of `flux_batch` what `transitleastsquares(t, flux).power(**kwargs)`
    reports as SDE, SDE_raw, chi2_min, period, T0, depth and duration (fractional, lc_cache_overview["duration"] of
    the template row at the chi^2 minimum, main.py:199-200) -- search, SDE spectra and final T0 fit all on the
    device (tls_power_batch), one record of 80 bytes back per light curve.

    statistics=True adds power()'s per-transit vetting statistics, computed on the device behind the final T0 fit
    (tls_power_batch_stats): the fields of tls_transit_stats (period_uncertainty, duration_days = results.duration in
    days, depth_mean[_std], depth_mean_even[_std], depth_mean_odd[_std], snr, odd_even_mismatch and the transit counts),
    plus rp_rs, FAP and chi2red_min formed on the host.  Every field equals the results key of the same name (the tuples
    split into _std fields); a curve without a fit reports what power() reports then.  per_transit=True (implies
    statistics) also returns a dict of [n_curves, max_epochs] arrays -- transit_times, per_transit_count, transit_depths,
    transit_depths_uncertainties, snr_per_transit, snr_pink_per_transit, NaN past a curve's epochs -- and n_epochs.
    The statistics need ascending t.

    models=True (implies statistics and per_transit) also returns the arrays power() returns for plotting, computed on the
    device behind the statistics (tls_power_batch_models), as a dict: folded_phase, folded_y, folded_dy and model_folded_model
    [n_curves, n]; model_lightcurve_time and model_lightcurve_model [n_curves, lc_cap], NaN past lc_len[k] entries; lc_len;
    model_folded_phase [n] (one numpy.linspace, shared).  The phases are sorted in the STABLE order (equal phases by index);
    power()'s numpy.argsort leaves the order of equal phases open, for distinct phases the two are the same.  A curve without
    a fit has NaN rows and lc_len 0.

    detrend=k (an odd kernel size) searches flux_batch / medfilt(flux_batch, k) instead (detrend_batch, on the device; the
    rows come back to the host and go through the search unchanged), so the result equals power_batch on the rows detrended
    beforehand; dy_batch is passed through as it is.  detrend=Biweight(window_length, break_tolerance) searches
    biweight_batch(t, flux_batch, window_length, break_tolerance) the same way.  detrend=SysRem(n_components) first removes
    the systematics the rows SHARE (sysrem_batch: fitted over the WHOLE batch on one device -- the given context, or the
    first of `devices` -- and weighted with dy_batch where one is given; the rows are then dealt out as before), and a tuple
    or list applies its steps left to right, e.g. (SysRem(2), Biweight(0.5)).  detrend=None searches flux_batch as given.
    detrend_mask ([n_curves, n], uint8 or bool, anything but 0: protected -- transit_mask) is given to every Biweight and
    Prewhiten step of detrend as its mask (biweight_batch, prewhiten_batch): the protected points are left out of the fits, the
    rows that are searched keep every point.  A SysRem step runs UNMASKED (its fit spans the rows and has no masked form here);
    a median-filter step together with a mask raises ValueError before any device work (that filter is defined by its sample
    count and zero padding, equal to scipy, and gets no masked form).  power_batch_protected is the two-pass flow in one call.

    peaks=K (1 to 32) also returns the K highest harmonic-aware peaks of every curve's detrended power -- the runners-up of the
    one pick: a second planet, a binary under its alias -- selected on the device from the spectrum it already holds
    (tls_power_batch_peaks; 48 K + 8 bytes more per curve, no per-period array comes back), as a dict: `peaks`, a structured
    array [n_curves, K] with period, power, chi2, depth, index, row (the search's values at the peak's index) and duration
    (table.duration[row]); `n_peaks` [n_curves].  Entries past a curve's n_peaks are NaN / -1; a curve without a fit has
    none.  The selection is greedy non-maximum suppression (find_peaks below states it exactly; tests/peaks_spec.py is its
    numpy restatement): candidates are the local maxima of the power at or above peak_min_power (None: all); the highest
    one alive is taken (the lowest index among equals, so the first peak is index_power) and every candidate within
    peak_separation * r * P of r * P leaves, for the taken period P, r = 1 and every r of peak_ratios -- by default
    HARMONICS, without which ranks 2 to 4 of a strong planet are its own harmonics.  peaks combines with with_arrays,
    statistics, per_transit, detrend and devices; peaks with models=True raises ValueError (no entry point carries both).
    Bad peak arguments raise ValueError before any device work.

    peak_fits=True (with peaks=K; needs ascending t) gives every peak what the one pick has: the final T0 fit and the
    vetting statistics, on the device behind the group's peaks (tls_power_batch_peak_fits), 144 bytes more per peak in the
    same copy.  The `peaks` array gains T0, status (0 fitted; 1 no such peak; 2 the search fitted nothing at the index), every
    field of tls_transit_stats (duration_days, snr, odd_even_mismatch, depth_mean_odd / _even, the counts, ...) and rp_rs;
    all NaN where status != 0.  A candidate takes period, depth AND template row from its own index (the pick takes its row
    from argmin(chi2)), and its period uncertainty is walked from its own index: rank 0 equals the summary's T0 and statistics
    wherever index_best == index_power.  Summary, statistics and the other peak fields do not change.  peak_fits without
    peaks, or with models=True, raises ValueError before any device work.

    phase_scan=True (with peak_fits=True) adds the secondary-eclipse phase scan of every peak -- the test against an
    eclipsing binary found at its true period, as odd_even_mismatch is the test against one found at half of it -- on the
    device behind each slab's fits (tls_power_batch_phase_scan), from the period, T0 and duration_days of the fit records
    there, 96 bytes more per peak in the same copy.  The `peaks` array gains the fields phase_scan_fields() (phase_scan below
    states the scan): scan_status is 1 and the others NaN where status != 0.  phase_scan_max_bins and phase_scan_min_count are
    phase_scan's max_bins and min_count.  Everything else of the result stays as it is, bit for bit.  phase_scan without
    peak_fits, or with a bad max_bins or min_count, raises ValueError before any device work.

    transit_times=True (with peak_fits=True) times every transit of every fitted peak on its own and refits the ephemeris
    through the times (transit_times below states it), in one call of tls_transit_times behind the search, on the device
    that searched the curve and on the rows it searched, from the period of the peak and T0 and duration_days of its fit
    record, with transit_times' defaults for gap_tolerance and transit_depth_min; transit_times_search and
    transit_times_min_ses are its search and min_ses.  The `peaks` array gains tt_status, tt_n_timed, tt_period,
    tt_period_err, tt_T0, tt_T0_err, tt_chi2, tt_rms and tt_max_sigma (tt_status 1 and the others NaN where status != 0), and
    the peaks dict `transit_times`, a structured array [n_curves, K, max_epochs] with the fields transit_time_fields()
    (max_epochs: the most epochs a period of the grid can have).  Everything else of the result stays as it is, bit for
    bit.  transit_times without peak_fits, or with a bad search or min_ses, raises ValueError before any device work.

    shape_fit=True (with peak_fits=True) fits a trapezoid to the dip of every fitted peak -- flat-bottomed like a planet or
    V-shaped like a grazing binary (shape_fit below states it) -- in one call of tls_shape_fit behind the search, on the
    device that searched the curve and on the rows it searched, from the period of the peak and T0 and duration_days of its
    fit record, over shape_fit's default tables; shape_fit_window and shape_fit_min_count are its window and min_count.  The
    `peaks` array gains the fields shape_fit_fields() (shape_status 1 and the others NaN where status != 0).  Everything else
    of the result stays as it is, bit for bit.  shape_fit without peak_fits, or with a bad window or min_count, raises
    ValueError before any device work.

    sine_test=True (with peak_fits=True) asks of every fitted peak whether it is the star's own variability -- a sinusoid at
    the peak's period, half of it or twice it, as a contact binary, an ellipsoidal variable or a spotted star gives (sine_test
    below states it) -- in one call of tls_sine_test behind the search, on the device that searched the curve and on the rows
    it searched, from the period of the peak and T0 and duration_days of its fit record, whose transits are masked out
    (sine_test_mask durations wide) before the sinusoid is measured; sine_test_harmonics are the period ratios.  The `peaks`
    array gains the fields sine_test_fields() (sine_status 1 and the others NaN where status != 0).  Everything else of the
    result stays as it is, bit for bit.  sine_test without peak_fits, or with a bad mask or harmonics, raises ValueError
    before any device work.

    ephemeris_match=True (with peak_fits=True) is the one test that looks ACROSS the batch: the curves of a batch share their
    time stamps -- one field, camera and sector -- and so contaminate one another and share instrumental periods.  Every
    fitted peak of every curve is matched against the fitted peaks of every OTHER curve for a common period (or an integer
    multiple up to ephemeris_match_max_ratio) and epoch (ephemeris_match below states it; ephemeris_match_drift and
    ephemeris_match_epoch are its two tolerances), in one call of tls_ephemeris_match on one device -- the given context, or
    the first of `devices` -- after the slices of all devices are joined.  The candidates are the peaks of status 0 with
    star = the curve's index, the peak's period, T0 and duration_days of its fit record, strength = 1 - depth and
    span = max t - min t.  The `peaks` array gains the fields ephemeris_match_peak_fields(): match_status (1, and the others
    NaN or -1, where status != 0), match_n_same, match_n_period, match_n_match, match_curve and match_rank (the strongest match
    as an index into `peaks`, -1 without one), match_ratio, match_dt, match_drift, match_strength and match_child (1: the
    match is deeper, this peak is its diluted copy).  Everything else of the result stays as it is, bit for bit.
    ephemeris_match without peak_fits, or with a bad tolerance or max_ratio, raises ValueError before any device work.

    views=True (with peak_fits=True) folds and median-bins every fitted peak into the five views a vetter reads -- global,
    local, local_even, local_odd and secondary (folded_views below states them) -- in one call of tls_folded_views behind the
    search, on the device that searched the curve and on the rows it searched, from the period of the peak and T0 and
    duration_days of its fit record; views_global_bins, views_local_bins, views_local_durations and views_local_width are
    folded_views' n_global, n_local, local_durations and local_width.  With phase_scan=True the secondary view is centred on
    the scan's secondary_phase; without it that view is NaN / 0.  The peaks dict gains `views`, the dict of arrays of
    folded_views shaped [n_curves, K, bins], and the `peaks` array views_status (1, and NaN / 0 in the arrays, where
    status != 0) and views_n_global, views_n_local, views_n_local_even, views_n_local_odd, views_n_secondary.  Everything else
    of the result stays as it is, bit for bit.  views without peak_fits, or with a bad table, raises ValueError before any
    device work.

    event_vetting=True (with peak_fits=True) vets the INDIVIDUAL events of every fitted peak -- is each unique in its
    neighbourhood, does it rest on one sample, does the flux come back to the baseline, does the candidate survive without
    its bad events or its strongest one (event_vetting below states it) -- in one call of tls_event_vetting behind the
    search, on the device that searched the curve and on the rows it searched, from the period of the peak and T0 and
    duration_days of its fit record, with event_vetting's defaults for gap_tolerance and transit_depth_min;
    event_vetting_search, _chase_window, _guard, _min_ses, _chase_fraction, _chase_min, _point_fraction and _step_fraction
    are its parameters of those names.  The `peaks` array gains, behind every other group, the fields event_summary_fields()
    with the prefix ev_ (ev_status 1 and the others NaN where status != 0), and the peaks dict `events`, a structured array
    [n_curves, K, max_epochs] with the fields event_fields() (max_epochs: the most epochs a period of the grid can have).
    Everything else of the result stays as it is, bit for bit.  event_vetting without peak_fits, or with a bad parameter,
    raises ValueError before any device work.

    centroids=(cx_batch, cy_batch) (with peak_fits=True) -- the flux-weighted centroids of the apertures, of flux_batch's
    shape and on its time stamps, in any unit, NaN where a cadence has none -- measures the in-transit shift of the
    photocentre of every fitted peak (centroid_test below states it): WHICH star dims.  One call of tls_centroid_test behind
    the search, on the device that searched the curve, on the flux rows it searched and the centroid rows of the same curves
    (they are never detrended), from the period of the peak and T0 and duration_days of its fit record, with the search's
    template; centroid_window, centroid_min_in and centroid_min_out are centroid_test's window, min_in and min_out.  The
    `peaks` array gains, behind every other group, the fields centroid_fields() (cen_status 1 and the others NaN where
    status != 0).  Everything else of the result stays as it is, bit for bit.  centroids without peak_fits, of another shape
    than flux_batch, or with a bad parameter, raises ValueError before any device work.

    noise=True (with peak_fits=True), or noise=widths (samples), measures the noise profile of every curve -- a robust CDPP at
    the Kepler pulse durations (noise_widths(t)) or at the given widths (noise_profile below states it, with its defaults for
    the clips, gap_tolerance and min_count) -- in one call of tls_noise_profile behind the search, on the device that searched
    the curve and on the rows it searched.  The peaks dict gains `noise`, the dict noise_profile returns, and the `peaks`
    array, behind every other group, noise_width (the profile width nearest duration_days / cadence, the smaller one on a
    tie), noise_sigma (robust at that width) and noise_mes = depth_mean * sqrt(transit_count) / noise_sigma, formed on the
    host; NaN, and noise_width -1, where status != 0 or noise_sigma is NaN.  Everything else of the result stays as it is,
    bit for bit.  noise without peak_fits, or with bad widths, raises ValueError before any device work.

    transit_fit=True (with peak_fits=True), or transit_fit=dict(...) with keywords of transit_fit below (impacts, ratios,
    shifts, exposure, n_sub, window, min_count, delta, profile), fits a limb-darkened, exposure-integrated transit to every
    fitted peak -- planet size, impact parameter, T14 and their profile-likelihood ranges (transit_fit below states it) -- in
    one call of tls_transit_fit behind the search, on the device that searched the curve and on the rows it searched, from
    the period and depth of the peak and T0 and duration_days of its fit record, with the search's u / limb_dark.  The `peaks`
    array gains, behind every other group, the fields transit_fit_fields() (fit_status 1 and the others NaN where
    status != 0, and where the peak's duration is too short for the window to hold the widest, farthest shifted model plus
    half an exposure: pass transit_fit=dict(window=1.5) for short peaks).  Everything else of the result stays as it is, bit
    for bit.  transit_fit without peak_fits, or with a bad table or window, raises ValueError before any device work.

    Returns (summary, periods[, chi2, row, depth, power][, per_transit][, models][, peaks]): summary is a numpy structured
    array with the fields of tls_power_summary plus "duration" (and the statistics on request)."""
    given = dict(locals())     # (every argument by its name, for the stages' requests)
    peaks = _peaks_request(peaks, peak_separation, peak_ratios, peak_min_power, models, peak_fits)
    phase_scan = _phase_scan_request(phase_scan, peak_fits, phase_scan_max_bins, phase_scan_min_count)
    stages = {stage.name: stage.request(*(given[k] for k in stage.keywords)) for stage in _PEAK_STAGES}
    return _power_batch(t, flux_batch, dy_batch, power_kwargs, context=context, device=device, devices=devices,
                        with_arrays=with_arrays, statistics=statistics, per_transit=per_transit, models=models,
                        detrend=detrend, detrend_mask=detrend_mask, peaks=peaks, peak_fits=bool(peak_fits),
                        phase_scan=phase_scan, stages=stages)


def _peaks_request(peaks, separation, ratios, min_power, models=False, peak_fits=False):
    """None, or the checked (k, separation, ratios, min_power) of a peaks=K request (ValueError for a bad one, and for
    peak_fits without peaks or with models)."""
    if peak_fits and peaks is None:
        raise ValueError("peak_fits=True needs peaks=K: the fits are those of the peaks")
    if peak_fits and models:
        raise ValueError("peak_fits cannot be combined with models=True: no entry point carries both")
    if peaks is None:
        return None
    from ._lib import peaks_arguments
    request = peaks_arguments(peaks, separation, ratios, min_power)
    if models:
        raise ValueError("peaks cannot be combined with models=True: no entry point carries both")
    return request


def _block(raw, names, sources=None):
    """A group of peak fields of its own: a structured array of raw's shape with the float64 fields `names`, the leading ones
    filled from raw's fields (or from its fields `sources`) in order; what is left is the caller's to fill."""
    out = numpy.zeros(raw.shape, dtype=[(k, "f8") for k in names])
    for k, source in zip(names, raw.dtype.names if sources is None else sources):
        out[k] = raw[source]
    return out


def _joined(records, *blocks):
    """`records` (None: nothing) and the blocks side by side in one structured array: the dtypes concatenated, the result
    allocated once and every field filled once.  One part alone is returned as it is."""
    parts = [part for part in (records,) + blocks if part is not None]
    if len(parts) == 1:
        return parts[0]
    out = numpy.zeros(parts[0].shape, dtype=[field for part in parts for field in part.dtype.descr])
    for part in parts:
        for k in part.dtype.names:
            out[k] = part[k]
    return out


def _duration_block(peaks, duration):
    """`duration` of the device's peak records: table.duration[row], NaN where the row is -1."""
    out = numpy.full(peaks.shape, numpy.nan, dtype=[("duration", "f8")])
    known = peaks["row"] >= 0
    if duration is not None:
        out["duration"][known] = numpy.asarray(duration, dtype=numpy.float64)[peaks["row"][known]]
    return out


def _with_duration(peaks, duration):
    """The device's peak records plus `duration` (_duration_block)."""
    return _joined(peaks, _duration_block(peaks, duration))


def peak_fit_fields():
    """The fields power_batch(peaks=K, peak_fits=True) adds to the `peaks` array, in order: T0, status, the fields of
    tls_transit_stats, rp_rs."""
    from ._lib import TRANSIT_STATS_FIELDS
    return ("T0", "status") + tuple(TRANSIT_STATS_FIELDS) + ("rp_rs",)


def _fits_block(peaks, fits, factor):
    """The device's fit records and rp_rs: rp_rs_from_depth(1 - depth) of the candidate's depth, formed as the summary's
    (numpy's scalar ** 0.5), NaN where nothing was fitted."""
    out = _block(fits, peak_fit_fields())
    fit = fits["status"] == 0
    out["rp_rs"] = numpy.nan
    out["rp_rs"][fit] = [x ** (1 / 2) for x in (1 - peaks["depth"][fit]) * factor]
    return out


def _with_fits(peaks, fits, factor):
    """The peaks (with duration) plus their fits (_fits_block)."""
    return _joined(peaks, _fits_block(peaks, fits, factor))


def _phase_scan_request(phase_scan, peak_fits, max_bins, min_count):
    """None, or the checked (max_bins, min_count) of a phase_scan=True request (ValueError for a bad one, and for phase_scan
    without peak_fits)."""
    if not phase_scan:
        return None
    if not peak_fits:
        raise ValueError("phase_scan=True needs peak_fits=True: the scans read T0 and duration of the fits")
    from ._lib import phase_scan_arguments
    return phase_scan_arguments(max_bins, min_count)


def phase_scan_fields():
    """The fields of a phase scan, in order -- what phase_scan returns and power_batch(..., phase_scan=True) adds to the
    `peaks` array: scan_status (tls_phase_record.status; the peaks array has the fit's `status` already), the other fields of
    tls_phase_record, secondary_significance, primary_significance."""
    from ._lib import PHASE_SCAN_FIELDS
    return ("scan_status",) + tuple(PHASE_SCAN_FIELDS[1:]) + ("secondary_significance", "primary_significance")


def _with_scans(records, scans):
    """`records` (None, or the peaks with their fits) plus the device's scan records and the two significances,
    (depth - scan_mean) / scan_std: NaN without a scatter, +-inf or NaN where the scatter is zero."""
    out = _block(scans, phase_scan_fields())
    with numpy.errstate(all="ignore"):
        out["secondary_significance"] = (scans["secondary_depth"] - scans["scan_mean"]) / scans["scan_std"]
        out["primary_significance"] = (scans["primary_depth"] - scans["scan_mean"]) / scans["scan_std"]
    return _joined(records, out)


def phase_scan(t, flux_batch, period, T0, duration, curve=None, max_bins=4096, min_count=3, context=None, device=None):
    """The secondary-eclipse phase scan of candidates the caller holds, on the device (tls_phase_scan): candidate f is
    (period[f], T0[f], duration[f] in days) on light curve curve[f] of flux_batch [n_curves, n] (or one row [n]) over the
    finite time stamps t; curve=None takes one candidate a curve, in order.  It needs no search.  The curve is folded into B
    bins no narrower than half a duration, a window is two neighbouring bins -- a box of about one duration -- and every
    window's depth is measured against the rest of the baseline (unweighted, as the reference's statistics are):

        status 1 and NaN everywhere else unless P, T0, d are finite, P > 0, d > 0 and q = 2.0 * P / d >= 16
        B = int(min(floor(q), max_bins))
        for i ascending:  x = (t[i] - T0) / P;  phi = x - floor(x);  b = min(int(phi * B), B - 1);  S[b] += y[i];  N[b] += 1
        W[j] = S[j] + S[(j+1)%B],  M[j] = N[j] + N[(j+1)%B];  primary window p = B-1 (phase [-1/B, 1/B))
        baseline Sb, Nb: bins 2 .. B-3;  inside windows: 2 <= j <= B-4
        delta[j] = (Sb - W[j]) / (Nb - M[j]) - W[j] / M[j]   inside j with M[j] >= min_count and Nb - M[j] >= 1
        delta[p] = Sb / Nb - W[p] / M[p]                     if M[p] >= min_count and Nb >= 1
        js, jb = the first inside j of the largest and of the smallest delta; rest = the valid inside j with |j - js| > 2
        scan_mean, scan_std = mean and root mean square deviation of delta over rest, where it has 8 windows or more

    Every step is one IEEE double operation and every sum runs in index order, so the result is bit-equal to the Python
    statement in tests/phase_scan_spec.py.  max_bins in [16, 4096], min_count >= 1; ValueError otherwise, before any device
    work.

    Returns a structured array [n_fits] with the fields phase_scan_fields(): scan_status (0 scanned, 1 nothing to scan),
    n_bins, n_windows, primary_depth and primary_count, secondary_depth, secondary_phase and secondary_count (the deepest
    window away from the primary: the secondary-eclipse candidate, at phase (js + 1) / B), bump_depth and bump_phase (the
    most negative window: a brightening), scan_mean and scan_std (the empirical scatter of such a box, red noise included),
    and secondary_significance and primary_significance, (depth - scan_mean) / scan_std.  Of a planet the secondary
    significance is that of the largest of B noise windows, 2 to 4; of an eclipsing binary it is many times that."""
    from ._lib import phase_scan_arguments
    max_bins, min_count = phase_scan_arguments(max_bins, min_count)
    if numpy.ndim(flux_batch) not in (1, 2) or numpy.ndim(t) != 1 or numpy.shape(flux_batch)[-1] != numpy.size(t):
        raise _checks.over_t(None, "flux_batch")
    ctx = context if context is not None else _search.default_context(device)
    return _with_scans(None, ctx.phase_scan(t, flux_batch, period, T0, duration, curve=curve, max_bins=max_bins,
                                            min_count=min_count))


def find_peaks(power, periods, k, separation=0.02, ratios=HARMONICS, min_power=None, chi2=None, row=None, depth=None,
               context=None, device=None):
    """The k harmonic-aware peaks of a periodogram the caller holds -- power [n_periods] or [n_rows, n_periods] over `periods`
    (any order) -- selected on the device (tls_find_peaks), the selection power_batch(peaks=k) applies to its own spectra:

        cand[j] = (j == 0 or power[j] > power[j-1]) and (j == n-1 or power[j] >= power[j+1]) and power[j] >= min_power
        alive = cand; at most k times, while an index is alive:
            j = lowest index of the largest power among the alive ones (numpy.argmax); take j; P = periods[j]
            for r in (1.0,) + ratios:  c = r * P;  w = separation * c;  alive[i] = False where fabs(periods[i] - c) <= w

    A NaN fails every comparison: an index holding one, or next to one, is no candidate.  Each of c, w and periods[i] - c is
    one IEEE double operation, and no arithmetic reaches the output, so the result is bit-equal to the numpy restatement in
    tests/peaks_spec.py.  k in [1, 32]; separation finite and in [0, 1); at most 16 ratios, each finite and > 0; min_power
    not NaN (None: no threshold); ValueError otherwise, before any device work.

    Returns (peaks, n_peaks): a structured array with period, power, chi2, depth, index, row ([k] for one row, else
    [n_rows, k]) and the number of peaks found per row.  chi2, row and depth (each None or shaped like power) fill the
    fields of their names; a field without a source, and every entry past n_peaks, is NaN or -1."""
    from ._lib import peaks_arguments
    k, separation, ratios, min_power = peaks_arguments(k, separation, ratios, min_power)
    if numpy.ndim(power) not in (1, 2) or numpy.shape(power)[-1] != numpy.size(periods) or numpy.ndim(periods) != 1:
        raise ValueError("power must be [n_periods] or [n_rows, n_periods], periods [n_periods]")
    if numpy.size(periods) < 1:
        raise ValueError("find_peaks needs at least one period")
    for other in (chi2, row, depth):
        if other is not None and numpy.shape(other) != numpy.shape(power):
            raise ValueError("chi2, row and depth must have the shape of power")
    ctx = context if context is not None else _search.default_context(device)
    peaks, n_peaks = ctx.find_peaks(power, periods, k, separation, ratios, min_power, chi2=chi2, row=row, depth=depth)
    if numpy.ndim(power) == 1:
        return peaks[0], n_peaks[0]
    return peaks, n_peaks


# what a peak stage sees of one device's slice of the batch (or, behind the join, of the whole batch): the plan inputs, the rows
# that were searched, whether a dy_batch was given, the slice itself, its peak, fit and scan records (scans None without a
# phase scan) and the most epochs a period of the grid can have
_PeakSlice = collections.namedtuple("_PeakSlice", ("inp", "y_rows", "dy_rows", "weighted", "rows", "peaks", "fits", "scans",
                                                   "max_epochs"))


def _power_batch(t, flux_batch, dy_batch, power_kwargs, context=None, device=None, devices=None, with_arrays=False,
                 statistics=False, per_transit=False, models=False, spectra=False, detrend=None, peaks=None,
                 peak_fits=False, phase_scan=None, detrend_mask=None, stages=None):
    """power_batch; spectra=True (power_results) also returns SR and power_raw [n_curves, n_periods] behind the arrays;
    peaks: None or a checked request (_peaks_request); peak_fits: with peaks, their T0 fits and statistics; phase_scan: None or a checked
    request (_phase_scan_request), with peak_fits, the fits' phase scans; stages: None, or a dict from the name of an entry
    of _PEAK_STAGES to its checked request (absent or None: not asked for), with peak_fits, the follow-ups of the fits."""
    stages = [(stage, stages[stage.name]) for stage in _PEAK_STAGES if stages and stages.get(stage.name) is not None]
    models = bool(models)
    per_transit = bool(per_transit or models)
    statistics = bool(statistics or per_transit)
    if statistics or peak_fits:
        t_check = numpy.asarray(t, dtype=numpy.float64)
        if t_check.ndim != 1 or not numpy.all(t_check[1:] >= t_check[:-1]):
            raise ValueError("%s=True needs ascending time stamps t" % ("statistics" if statistics else "peak_fits"))
    flux_batch = _detrended(t, flux_batch, detrend, context, device, devices, dy_batch, detrend_mask)
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, power_kwargs)
    from . import constants as C
    osf = power_kwargs.get("oversampling_factor", C.OVERSAMPLING_FACTOR)
    kernel = osf * C.SDE_MEDIAN_KERNEL_SIZE
    if kernel != int(kernel):
        raise ValueError("oversampling_factor * %d must be an integer" % C.SDE_MEDIAN_KERNEL_SIZE)
    kw = dict(with_arrays=with_arrays, with_power=with_arrays, with_spectra=spectra, peaks=peaks)
    if statistics or peak_fits:
        from .stats import calculate_fill_factor, count_roots
        fill_factor = calculate_fill_factor(inp["t"])
        root, root_count = count_roots(len(inp["t"]))   # (k ** 0.5 of a count, in the two forms power() takes it)
        max_epochs = _max_epochs(inp["t"], inp["periods"])
    if statistics:
        kw.update(statistics=(fill_factor, root, root_count, max_epochs), per_transit=per_transit,
                  models=_model_template(inp) if models else None, lc_cap=_lc_cap(len(inp["t"]), max_epochs) if models else 0)
    if peak_fits:
        kw.update(peak_fits=(fill_factor, root, root_count, max_epochs), phase_scan=phase_scan)

    def follow_ups(ctx, scope, part, rows):
        # (the same context, the same rows: the candidates are the peaks the search fitted)
        env = _PeakSlice(inp, y_rows[rows], dy_rows[rows], dy_batch is not None, rows, part["peaks"], part["peak_fits"],
                         part.get("phase_scans"), max_epochs)
        for stage, request in stages:
            if stage.scope == scope:
                part.update(stage.run(ctx, env, request))

    def call(ctx, lo, hi):
        part = ctx._power_batch(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], inp["periods"], inp["table"], inp["params"],
                                int(kernel), **kw)
        if stages:
            follow_ups(ctx, "slice", part, slice(lo, hi))
        return part

    out = _run_batch(devices, device, context, len(y_rows), call)
    if any(stage.scope == "batch" for stage, _ in stages):
        # (across the curves, so behind the join: one call on one device, as the SysRem step)
        ctx, lock = _first_context(context, device, devices, len(y_rows))
        with lock:
            follow_ups(ctx, "batch", out, slice(0, len(y_rows)))
    raw = out["summary"]
    names = list(raw.dtype.names) + ["duration"]
    fields = [(k, raw.dtype[k]) for k in raw.dtype.names] + [("duration", "f8")]
    if statistics:
        fields += [(k, "f8") for k in out["stats"].dtype.names] + [("rp_rs", "f8"), ("FAP", "f8"), ("chi2red_min", "f8")]
    summary = numpy.zeros(len(raw), dtype=fields)
    for k in raw.dtype.names:
        summary[k] = raw[k]
    summary["duration"] = numpy.where(raw["no_fit"] != 0, numpy.nan, inp["table"].duration[raw["best_row"]])
    assert names == list(summary.dtype.names)[:len(names)]
    if statistics:
        from .stats import limb_darkening_factor
        for k in out["stats"].dtype.names:
            summary[k] = out["stats"][k]
        # rp_rs_from_depth(1 - depth) curve by curve (numpy's scalar ** 0.5, as power() takes it); NaN without a fit
        factor = limb_darkening_factor(inp["limb_dark"], inp["u"])
        fit = raw["no_fit"] == 0
        summary["rp_rs"] = numpy.nan
        summary["rp_rs"][fit] = [x ** (1 / 2) for x in (1 - raw["depth"][fit]) * factor]
        summary["FAP"] = _fap(raw["SDE"])
        summary["chi2red_min"] = raw["chi2_min"] / (len(inp["t"]) - 4)
    result = (summary, inp["periods"])
    if with_arrays:
        result += (out["chi2"], out["row"], out["depth"], out["power"])
    if per_transit:
        from ._lib import PER_TRANSIT_FIELDS
        pt = {k: out["per_transit"][:, i, :] for i, k in enumerate(PER_TRANSIT_FIELDS)}
        pt["n_epochs"] = out["n_epochs"]
        result += (pt,)
    if models:
        folded, model_folded, lightcurve, lc_len = (out[k] for k in ("folded", "model_folded", "lightcurve", "lc_len"))
        n = len(inp["t"])
        m = dict(folded_phase=folded[:, 0], folded_y=folded[:, 1], model_folded_model=model_folded,
                 model_lightcurve_time=lightcurve[:, 0], model_lightcurve_model=lightcurve[:, 1], lc_len=lc_len,
                 model_folded_phase=numpy.linspace(0 + 1 / n / 2, 1 + 1 / n / 2, n))   # (api.py: half a cadence on)
        # folded_dy: dy gathered by the device's order (NaN without a fit)
        order = folded[:, 2]
        no_fit = numpy.isnan(order[:, 0])
        m["folded_dy"] = numpy.take_along_axis(dy_rows, numpy.where(no_fit[:, None], 0, order).astype(numpy.int64), axis=1)
        m["folded_dy"][no_fit] = numpy.nan
        result += (m,)
    if peaks is not None:
        blocks = [_duration_block(out["peaks"], inp["table"].duration)]
        if peak_fits:
            from .stats import limb_darkening_factor
            blocks.append(_fits_block(out["peaks"], out["peak_fits"], limb_darkening_factor(inp["limb_dark"], inp["u"])))
            if phase_scan is not None:
                blocks.append(_with_scans(None, out["phase_scans"]))
        records = _joined(out["peaks"], *blocks)
        found = dict(peaks=records, n_peaks=out["n_peaks"])
        for stage, request in stages:
            found.update(stage.extras(out, request))
        found["peaks"] = _joined(records, *(stage.block(out, request, records) for stage, request in stages))
        result += (found,)
    if spectra:
        result += (out["SR"], out["power_raw"])
    return result


def power_results(t, flux_batch, dy_batch=None, context=None, device=None, devices=None, detrend=None, detrend_mask=None,
                  **power_kwargs):
    """power()'s results object for every light curve of `flux_batch` (shape [n_curves, len(t)], shared ascending time
    stamps): a list of transitleastsquaresresults, element k equal to
    transitleastsquares(t, flux_batch[k], dy_batch[k]).power(**power_kwargs) key for key and in key order (41 keys).  Search,
    spectra, final T0 fit, statistics, the folded light curve and the model light curves all come from the device
    (power_batch(models=True, with_arrays=True)); tuples are rebuilt from the _std fields, chi2red = chi2 / (n - 4),
    `periods` is one array shared by all objects, and a curve without a fit gets exactly what power() returns then
    (api.transitleastsquares._results_without_fit).  The folded light curve is sorted in the stable order: for equal
    phases (duplicate time stamps) power()'s numpy.argsort may order them otherwise.

    Memory: every object holds O(n_periods + n) doubles -- power, power_raw, SR, chi2, chi2red and the folded and model
    arrays, about 0.7 MB for the k2_90d configuration (90 days at 48 cadences a day), so 1024 curves take about 0.7 GB, and
    the call's own staging as much again while it runs.  Callers with large batches pass them in chunks.
    devices=[...] deals the batch out over several GPUs, as the other survey calls.  detrend=k searches
    flux_batch / medfilt(flux_batch, k) (detrend_batch), detrend=Biweight(...) the rows biweight_batch forms,
    detrend=SysRem(...) the rows sysrem_batch forms and a tuple its steps left to right, as power_batch does; the objects
    then describe the detrended rows.  detrend_mask: power_batch's (the mask of every Biweight and Prewhiten step; SysRem
    runs unmasked; a median-filter step with a mask is a ValueError)."""
    from .api import transitleastsquares
    from .results import transitleastsquaresresults
    if len(numpy.shape(flux_batch)) != 2 or numpy.shape(flux_batch)[1] != len(t):
        raise ValueError("flux_batch must have shape [n_curves, len(t)]")
    if dy_batch is not None and numpy.shape(dy_batch) != numpy.shape(flux_batch):
        raise ValueError("dy_batch must have the shape of flux_batch")
    summary, periods, chi2, row, depth, power, pt, m, SR, power_raw = _power_batch(
        t, flux_batch, dy_batch, power_kwargs, context=context, device=device, devices=devices, with_arrays=True,
        statistics=True, per_transit=True, models=True, spectra=True, detrend=detrend, detrend_mask=detrend_mask)
    n = len(m["model_folded_phase"])
    chi2red = chi2 / (n - 4)   # (main.py:210-212)
    out = []
    for k in range(len(summary)):
        rec = summary[k]
        if rec["no_fit"]:
            out.append(transitleastsquares._results_without_fit(None, periods, chi2[k], chi2red[k], numpy.min(chi2[k]),
                                                                 numpy.min(chi2red[k])))
            continue
        e = int(pt["n_epochs"][k])
        cnt = int(m["lc_len"][k])
        row_of = {key: pt[key][k, :e] for key in ("per_transit_count", "transit_depths", "transit_depths_uncertainties",
                                                   "snr_per_transit", "snr_pink_per_transit")}
        out.append(transitleastsquaresresults(
            float(rec["SDE"]), float(rec["SDE_raw"]), numpy.min(chi2[k]), numpy.min(chi2red[k]), periods[rec["index_power"]],
            rec["period_uncertainty"], float(rec["T0"]), rec["duration_days"], depth[k][rec["index_power"]],
            (rec["depth_mean"], rec["depth_mean_std"]), (rec["depth_mean_even"], rec["depth_mean_even_std"]),
            (rec["depth_mean_odd"], rec["depth_mean_odd_std"]), row_of["transit_depths"],
            row_of["transit_depths_uncertainties"], rec["rp_rs"], rec["snr"], row_of["snr_per_transit"],
            row_of["snr_pink_per_transit"], rec["odd_even_mismatch"], pt["transit_times"][k, :e].tolist(),
            row_of["per_transit_count"], e, int(rec["distinct_transit_count"]), int(rec["empty_transit_count"]),
            rec["FAP"], int(rec["in_transit_count"]), int(rec["after_transit_count"]), int(rec["before_transit_count"]),
            periods, power[k], power_raw[k], SR[k], chi2[k], chi2red[k], m["model_lightcurve_time"][k, :cnt],
            m["model_lightcurve_model"][k, :cnt], m["model_folded_phase"], m["folded_y"][k], m["folded_dy"][k],
            m["folded_phase"][k], m["model_folded_model"][k]))
    return out


def power_batch_protected(t, flux_batch, detrend, sde_min, factor=1.5, n_peaks=1, **power_batch_kwargs):
    """The two-pass flow in one call: search, mask the candidates' transits, detrend the RAW rows again with those points left
    out of the fits, search the result.

        pass 1: power_batch(t, flux_batch, detrend=detrend, peaks=n_peaks, peak_fits=True, ...)
        mask:   transit_mask of the fitted peaks (period, T0, duration_days; status 0) of the curves with SDE >= sde_min,
                `factor` durations wide, built on the device
        pass 2: power_batch(t, flux_batch, detrend=detrend, detrend_mask=mask, ...) with the caller's own options

    sde_min has no default: sde_threshold (from null_sde's table) chooses it.  A curve below sde_min has an all-zero mask row
    and comes out of pass 2 as from plain power_batch(detrend=...).  power_batch_kwargs are power_batch's (dy_batch, context,
    device, devices, statistics, peaks, ..., and the search's own keywords); pass 1 takes of them only what the search itself
    needs (dy_batch, the context or devices and the search's keywords) with peak_ratios, peak_separation and peak_min_power.
    detrend must hold a Biweight or Prewhiten step for the mask to act; a median-filter step raises ValueError, a SysRem step
    runs unmasked.  ValueError, before any device work, for a factor that is not finite and > 0, an sde_min that is not a
    number (NaN included) and n_peaks outside [1, 32].

    Returns (pass 2's result, info): info is a dict with `protected` [n_curves] bool (SDE of pass 1 >= sde_min), `mask`
    (uint8 [n_curves, n]) and `summary` (pass 1's)."""
    _checks.finite_positive("power_batch_protected", "factor", factor)
    _checks.no_nan("power_batch_protected", "sde_min", sde_min, "must be a number")
    if "detrend_mask" in power_batch_kwargs:
        raise ValueError("power_batch_protected forms detrend_mask itself")
    for step in _detrend_steps(detrend):
        if not isinstance(step, (Biweight, SysRem, Prewhiten, Decorrelate, Spline, Clean)):
            raise ValueError("power_batch_protected: the median filter (detrend=%r) has no masked form; use Biweight or "
                             "Prewhiten steps" % (step,))
    _peaks_request(n_peaks, power_batch_kwargs.get("peak_separation", 0.02), power_batch_kwargs.get("peak_ratios", HARMONICS),
                   power_batch_kwargs.get("peak_min_power"), False, True)
    keep = {"dy_batch", "context", "device", "devices", "peak_separation", "peak_ratios", "peak_min_power"}
    named = {k for k, p in inspect.signature(power_batch).parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD}
    first = {k: v for k, v in power_batch_kwargs.items() if k in keep or k not in named}   # (not named: the search's keywords)
    out = power_batch(t, flux_batch, detrend=detrend, peaks=n_peaks, peak_fits=True, **first)
    summary, peaks = out[0], out[-1]["peaks"]
    protected = summary["SDE"] >= sde_min
    n_curves = len(summary)
    use = protected[:, None] & (peaks["status"] == 0)
    curve = numpy.broadcast_to(numpy.arange(n_curves)[:, None], use.shape)[use]
    from ._lib import transit_mask_arguments
    a = transit_mask_arguments(t, peaks["period"][use], peaks["T0"][use], peaks["duration_days"][use], curve, n_curves, factor)
    ctx, lock = _first_context(power_batch_kwargs.get("context"), power_batch_kwargs.get("device"),
                               power_batch_kwargs.get("devices"), n_curves)
    with lock:
        mask = ctx.transit_mask(a["t"], a["period"], a["T0"], a["duration"], a["curve"], a["n_curves"], a["factor"])
    result = power_batch(t, flux_batch, detrend=detrend, detrend_mask=mask, **power_batch_kwargs)
    return result, dict(protected=protected, mask=mask, summary=summary)


# ---- multi-planet search: the fitted transits divided out, the quotient searched again ------------------------------------
def remove_transits(t, flux_batch, planets, curve=None, exposure=None, n_sub=5, profile=None, return_model=False,
                    return_status=False, context=None, device=None, devices=None, **template_kwargs):
    """flux_batch [n_curves, n] (or one row [n]) over the shared, ascending time stamps t with the fitted transits of
    `planets` divided out, on the device (tls_remove_transits): the limb-darkened, exposure-integrated model transit_fit fits
    is evaluated at EVERY point of the planet's curve, y = y / (1 - A * mval) wherever the model dips (flux is multiplicative),
    and every other point comes back bit for bit.  No point is deleted, so the rows keep their shared time stamps and the
    next search is an ordinary power_batch on the result -- the planet under the one found (power_batch_multi is that flow
    in one call).  The statement is in tests/remove_transits_spec.py and include/tls_amd.h, and the device equals it bit for
    bit.

    planets: a structured array with the fields period, T0, fit_row, fit_amplitude, fit_b, fit_duration, fit_shift -- a
    `peaks` array of power_batch(..., transit_fit=True) or what transit_fit returns with period and T0 beside it.  curve
    [n_fits]: the curve of every planet, flattened; None: planets [n_curves, K] are the planets of curve 0, 1, ... row by row,
    planets [n_fits] one a curve, in order.  The planets of a curve are divided out in their order.  A planet takes part
    (status 0) iff its seven values are finite, period, fit_duration and fit_amplitude > 0, fit_b in [0, 1 + k_rows[fit_row])
    and fit_amplitude times the deepest entry of its profile row < 1; any other is skipped (status 1) -- the NaN records of
    an unfitted peak among them.

    exposure, n_sub, profile and the template keywords (u, limb_dark, transit_template) mean what they mean for transit_fit,
    and must be the fit's own for the model to be the fitted one.  ValueError, before any device work, for what
    _lib.remove_transits_arguments and the set-up of transit_fit refuse.

    Returns rows[, model][, status]: rows and model (the product of the factors 1 - A * mval, 1.0 elsewhere) in flux_batch's
    shape, status float64 in planets' shape."""
    from ._lib import REMOVE_TRANSITS_FIELDS, remove_transits_arguments
    what = "remove transits: "
    one_row = numpy.ndim(flux_batch) == 1
    t, flux_batch, _ = _candidate_rows("remove transits", t, flux_batch)
    setup = _transit_fit_setup(t, None, None, None, exposure, n_sub, 1.0, 3, 1.0, profile, template_kwargs, "remove transits")
    planets = numpy.asarray(planets)
    if planets.dtype.names is None or any(k not in planets.dtype.names for k in REMOVE_TRANSITS_FIELDS):
        raise ValueError(what + "planets must be a structured array with the fields %s" % (REMOVE_TRANSITS_FIELDS,))
    n_curves = numpy.shape(flux_batch)[0]
    if curve is None:
        if planets.ndim == 2 and planets.shape[0] == n_curves:
            curve = numpy.repeat(numpy.arange(n_curves, dtype=numpy.int64), planets.shape[1])
        elif planets.ndim != 1 or planets.shape[0] > n_curves:
            raise ValueError(what + "without curve, planets must be [n_curves, K] or hold at most one a curve, got shape %s "
                             "for %d curves" % (planets.shape, n_curves))
    elif numpy.shape(curve) != (planets.size,):
        raise ValueError(what + "curve must hold one index a planet, flattened: %d, got shape %s"
                         % (planets.size, numpy.shape(curve)))
    flat = planets.reshape(-1)
    a = remove_transits_arguments(t, flux_batch, flat["period"], flat["T0"], flat["fit_row"], flat["fit_amplitude"],
                                  flat["fit_b"], flat["fit_duration"], flat["fit_shift"], setup["k_rows"], setup["profile"],
                                  setup["sub"], curve)
    of_curve = numpy.arange(len(flat), dtype=numpy.int64) if a["curve"] is None else a["curve"]
    names = ("period", "T0", "row", "amplitude", "b", "duration", "shift")

    def call(ctx, lo, hi):
        mine = numpy.nonzero((of_curve >= lo) & (of_curve < hi))[0]
        out = ctx.remove_transits(a["t"], a["y"][lo:hi], *(a[k][mine] for k in names), a["k_rows"], a["profile"], a["sub"],
                                  curve=of_curve[mine] - lo, return_model=return_model, return_status=True)
        return dict(rows=out[0], model=out[1] if return_model else None, status=out[-1], index=mine)

    out = _run_batch(devices, device, context, n_curves, call)
    status = numpy.zeros(len(flat))
    status[out["index"]] = out["status"]
    rows, model = out["rows"], out["model"]
    if one_row:
        rows, model = rows[0], None if model is None else model[0]
    result = (rows,) + ((model,) if return_model else ()) + ((status.reshape(planets.shape),) if return_status else ())
    return result[0] if len(result) == 1 else result


def is_repeat(period, earlier, separation=0.02, ratios=HARMONICS):
    """Whether `period` (any shape) repeats the planet found at `earlier` days: the closeness test of the peak selection
    (find_peaks) against the earlier period and its multiples by `ratios` -- fabs(period - r * earlier) <= separation *
    (r * earlier) for r = 1 or an r of ratios, c = r * earlier, w = separation * c and period - c one IEEE double operation
    each.  A NaN repeats nothing."""
    period = numpy.asarray(period, dtype=numpy.float64)
    out = numpy.zeros(period.shape, dtype=bool)
    with numpy.errstate(invalid="ignore", over="ignore"):
        for r in (1.0,) + tuple(float(x) for x in ratios):
            c = numpy.float64(r) * numpy.float64(earlier)
            w = numpy.float64(separation) * c
            out |= numpy.fabs(period - c) <= w
    return out


# power_batch_multi's pass_status
PLANET_ACCEPTED, PLANET_NOT_REACHED, PLANET_BELOW_SDE, PLANET_NO_FIT, PLANET_REPEAT = 0, 1, 2, 3, 4
_SUMMARY_RENAMED = ("period", "T0", "depth", "duration")     # summary fields a peak record has too: summary_period, ...


def multi_planet_fields(summary_dtype, peaks_dtype):
    """The fields [(name, dtype)] of power_batch_multi's planets array: pass_status, the pass's summary fields (period, T0,
    depth and duration as summary_period, ..., the peak record holds fields of those names) and the fields of its peak
    record."""
    fields = [("pass_status", "i8")]
    fields += [("summary_" + k if k in _SUMMARY_RENAMED else k, summary_dtype[k]) for k in summary_dtype.names]
    return fields + [(k, peaks_dtype[k]) for k in peaks_dtype.names]


def power_batch_multi(t, flux_batch, sde_min, n_planets=3, detrend=None, protect_factor=None, transit_fit=True,
                      return_rows=False, **power_batch_kwargs):
    """The multi-planet search in one call: search, divide the fitted transit out of the RAW rows, search the quotient.  A
    second planet under a deep first one never shows in the first periodogram, so no peak list (peaks=K) returns it; with the
    first one divided out it is the pick of the next pass.

        pass 0:     power_batch(t, rows, detrend=detrend, peaks=1, peak_fits=True, transit_fit=transit_fit, ...), every curve
        after every pass, a curve's pick (its peak of rank 0) is ACCEPTED iff its SDE >= sde_min, its peak status and its
                    fit_status are 0, and its period is no repeat (is_repeat with peak_separation and peak_ratios) of an
                    earlier accepted planet of that curve
        pass j + 1: only the curves with an accepted pick that hold fewer than n_planets go on: power_batch as above on
                    remove_transits(RAW rows of those curves, all their accepted planets in the order found) -- from the raw
                    rows every time, with the same detrend, so no pass detrends a quotient of a detrended row

    sde_min has no default: sde_threshold (from null_sde's table) chooses it.  n_planets in [1, 8].  transit_fit is True or
    the dict power_batch takes (the fit is what is divided out, so it cannot be off).  protect_factor (None: off): the
    detrend_mask of pass j + 1 is transit_mask of the accepted planets (period, T0, duration_days), that many durations
    wide, so the detrending fits around the transits already found; power_batch's refusal of a median-filter step with a mask
    stands.  power_batch_kwargs: dy_batch, context, device, devices, peak_separation, peak_ratios, peak_min_power and the
    search's own keywords, passed on unchanged (dy_batch row by row); any other keyword of power_batch raises ValueError --
    the rows of return_rows=True go through power_batch for anything else.  ValueError before any device work for a bad
    argument.

    Returns (planets, info).  planets: a structured array [n_curves, n_planets], entry [c, j] being pass j of curve c --
    pass_status (0 accepted and divided out, 1 not reached, 2 below sde_min, 3 no fit, 4 a repeat) and, where the pass ran,
    its summary fields and its peak record with the fit_ fields (multi_planet_fields; NaN and -1 where it did not run).  The
    accepted entries of a row serve as remove_transits' planets.  info: a dict with `n_found` [n_curves], `searched` (the
    index array of the curves every pass searched, pass by pass) and with return_rows=True `rows`, flux_batch with every
    accepted planet divided out."""
    _checks.no_nan("power_batch_multi", "sde_min", sde_min, "must be a number")
    n_planets = _checks.integer("power_batch_multi", "n_planets", n_planets, 1, 8)
    if protect_factor is not None:
        _checks.finite_positive("power_batch_multi", "protect_factor", protect_factor, "must be None or finite and > 0")
        for step in _detrend_steps(detrend):
            if not isinstance(step, (Biweight, SysRem, Prewhiten, Decorrelate, Spline, Clean)):
                raise ValueError("power_batch_multi: the median filter (detrend=%r) has no masked form; use Biweight or "
                                 "Prewhiten steps with protect_factor" % (step,))
    if transit_fit is None or transit_fit is False:
        raise ValueError("power_batch_multi: transit_fit must be True or a dict: the fitted transit is what is divided out")
    keep = {"dy_batch", "context", "device", "devices", "peak_separation", "peak_ratios", "peak_min_power"}
    named = {k for k, p in inspect.signature(power_batch).parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD}
    for k in power_batch_kwargs:
        if k in named and k not in keep:
            raise ValueError("power_batch_multi: %s is not passed on to the passes; call power_batch on the rows of "
                             "return_rows=True" % k)
    search = {k: v for k, v in power_batch_kwargs.items() if k not in named}
    rest = {k: v for k, v in power_batch_kwargs.items() if k in keep and k != "dy_batch"}
    where = {k: power_batch_kwargs.get(k) for k in ("context", "device", "devices")}
    separation, ratios = power_batch_kwargs.get("peak_separation", 0.02), power_batch_kwargs.get("peak_ratios", HARMONICS)
    _peaks_request(1, separation, ratios, power_batch_kwargs.get("peak_min_power"), False, True)
    raw = numpy.asarray(flux_batch, dtype=numpy.float64)
    if raw.ndim != 2 or raw.shape[1] != len(t) or len(raw) < 1:
        raise ValueError("flux_batch must have shape [n_curves, len(t)]")
    # (a Clean at the head of detrend repairs the raw rows ONCE: the fitted transits are divided out of the repaired rows)
    raw, detrend = _clean_first(t, raw, detrend, where["context"], where["device"], where["devices"])
    dy_batch = power_batch_kwargs.get("dy_batch")
    if dy_batch is not None:
        dy_batch = numpy.asarray(dy_batch, dtype=numpy.float64)
        if dy_batch.shape != raw.shape:
            raise ValueError("dy_batch must have the shape of flux_batch")
    setup = _transit_fit_request(transit_fit, True, t, search)
    # (the passes and remove_transits share ONE profile table: formed once, and the model divided out is the fitted one)
    fit_options = dict({} if transit_fit is True else transit_fit, profile=(setup["k_rows"], setup["profile"]))
    removal = dict(where, profile=(setup["k_rows"], setup["profile"]), exposure=fit_options.get("exposure"),
                   n_sub=fit_options.get("n_sub", 5))
    n_curves = len(raw)
    planets, n_found, searched = None, numpy.zeros(n_curves, dtype=numpy.int64), []
    active = numpy.arange(n_curves)
    for j in range(n_planets):
        if len(active) == 0:
            break
        rows, mask = raw[active], None
        if j:
            found = planets[active, :j]
            rows = remove_transits(t, rows, found, **removal)
            if protect_factor is not None:
                mask = _first_mask(t, found, len(active), j, protect_factor, where)
        out = power_batch(t, rows, dy_batch=None if dy_batch is None else dy_batch[active],
                          detrend=_detrend_of_rows(detrend, active), detrend_mask=mask, peaks=1, peak_fits=True,
                          transit_fit=fit_options, **dict(rest, **search))
        summary, peaks = out[0], out[-1]["peaks"][:, 0]
        if planets is None:
            planets = numpy.zeros((n_curves, n_planets), dtype=multi_planet_fields(summary.dtype, peaks.dtype))
            for k in planets.dtype.names:
                planets[k] = numpy.nan if planets.dtype[k].kind == "f" else -1
            planets["pass_status"] = PLANET_NOT_REACHED
        for k in summary.dtype.names:
            planets["summary_" + k if k in _SUMMARY_RENAMED else k][active, j] = summary[k]
        for k in peaks.dtype.names:
            planets[k][active, j] = peaks[k]
        with numpy.errstate(invalid="ignore"):
            status = numpy.where(summary["SDE"] >= sde_min, PLANET_ACCEPTED, PLANET_BELOW_SDE)
            status[(status == PLANET_ACCEPTED) & ((peaks["status"] != 0) | (peaks["fit_status"] != 0))] = PLANET_NO_FIT
        for e in range(j):                           # (every earlier entry of a curve that goes on is an accepted planet)
            for at, c in enumerate(active):
                if status[at] == PLANET_ACCEPTED and is_repeat(peaks["period"][at], planets["period"][c, e], separation, ratios):
                    status[at] = PLANET_REPEAT
        planets["pass_status"][active, j] = status
        searched.append(active)
        n_found[active] += status == PLANET_ACCEPTED
        active = active[status == PLANET_ACCEPTED]
    info = dict(n_found=n_found, searched=searched)
    if return_rows:
        info["rows"] = remove_transits(t, raw, _accepted_only(planets), **removal)
    return planets, info


def _first_mask(t, found, n_active, j, factor, where):
    """transit_mask of the accepted planets `found` [n_active, j] on the first device of where["devices"]."""
    from ._lib import transit_mask_arguments
    a = transit_mask_arguments(t, found["period"].reshape(-1), found["T0"].reshape(-1), found["duration_days"].reshape(-1),
                               numpy.repeat(numpy.arange(n_active), j), n_active, factor)
    ctx, lock = _first_context(where["context"], where["device"], where["devices"], n_active)
    with lock:
        return ctx.transit_mask(a["t"], a["period"], a["T0"], a["duration"], a["curve"], a["n_curves"], a["factor"])


def _accepted_only(planets):
    """planets with the amplitude of every entry that was not accepted set to NaN: remove_transits skips those."""
    out = planets.copy()
    out["fit_amplitude"][out["pass_status"] != PLANET_ACCEPTED] = numpy.nan
    return out


def search_batch(t, flux_batch, dy_batch=None, context=None, device=None, devices=None, detrend=None, detrend_mask=None,
                 **power_kwargs):
    """Search every light curve of `flux_batch` (shape [n_curves, n_points]) on the grids that
    `transitleastsquares(t, flux).power(**power_kwargs)` would use.

    Returns (periods, chi2[n_curves, n_periods], row[...], depth[...]).  All light curves must
    share `t` and be free of invalid points (clean them first); a `dy_batch` must have the same
    weight structure for every curve (all uniform or all per-point).  detrend=k searches flux_batch / medfilt(flux_batch, k)
    (detrend_batch), detrend=Biweight(...) the rows biweight_batch forms, detrend=SysRem(...) the rows sysrem_batch forms
    (one fit over the whole batch) and a tuple its steps left to right, as power_batch does.  detrend_mask: power_batch's (the
    mask of every Biweight and Prewhiten step; SysRem runs unmasked; a median-filter step with a mask is a ValueError).
    """
    flux_batch = _detrended(t, flux_batch, detrend, context, device, devices, dy_batch, detrend_mask)
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, power_kwargs)

    def call(ctx, lo, hi):
        return dict(zip(("chi2", "row", "depth"), ctx.search_batch(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], inp["periods"],
                                                                   inp["table"], inp["params"])))

    out = _run_batch(devices, device, context, len(y_rows), call)
    return inp["periods"], out["chi2"], out["row"], out["depth"]


# ---- single-transit events: the template slid along the time series itself ------------------------------------------------
def single_transit_widths(t, duration_min=None, duration_max=1.0, log_step=1.1):
    """The default trial widths of single_transits, in samples: with dt = median(diff(t)), the sorted set of int(round(x))
    over the geometric series x = lo, lo * log_step, lo * log_step^2, ... <= hi from lo = max(3, duration_min / dt)
    (duration_min None: 3) to hi = min(duration_max / dt, 4096, n).  Durations are in days, log_step > 1.  At 30 min cadence
    the defaults give 24 widths from 3 to 48 samples.  ValueError for an empty grid (hi < lo) and a bad argument."""
    from ._lib import SINGLE_MAX_WIDTH, SINGLE_MIN_WIDTH
    t = numpy.asarray(t, dtype=numpy.float64)
    if t.ndim != 1 or len(t) < 2:
        raise ValueError("single transits: t must hold at least two time stamps")
    dt = float(numpy.median(numpy.diff(t)))
    if not (dt > 0.0 and dt < numpy.inf):
        raise ValueError("single transits: the median cadence of t must be finite and > 0, got %r" % dt)
    if not (float(log_step) > 1.0 and float(log_step) < numpy.inf):
        raise ValueError("single transits: log_step must be > 1, got %r" % (log_step,))
    if not (float(duration_max) > 0.0) or (duration_min is not None and not (float(duration_min) > 0.0)):
        raise ValueError("single transits: durations must be > 0 days")
    lo = float(SINGLE_MIN_WIDTH) if duration_min is None else max(float(SINGLE_MIN_WIDTH), float(duration_min) / dt)
    hi = min(float(duration_max) / dt, float(SINGLE_MAX_WIDTH), float(len(t)))
    widths, i = set(), 0
    while lo * float(log_step) ** i <= hi:
        widths.add(int(round(lo * float(log_step) ** i)))
        i += 1
    if not widths:
        raise ValueError("single transits: no trial width between %g and %g samples (durations %r to %r days at a cadence of "
                         "%g days, %d points)" % (lo, hi, duration_min, duration_max, dt, len(t)))
    return numpy.array(sorted(widths), dtype=numpy.int64)


def single_event_fields():
    """The fields of a single-transit event, in order: those of tls_single_event -- index, time = t[index], ses, depth, row,
    width (samples), t_first and t_last (the window's first and last time stamp) -- and duration_days = width * dt, formed
    on the host."""
    from ._lib import SINGLE_EVENT_FIELDS
    return tuple(SINGLE_EVENT_FIELDS) + ("duration_days",)


def single_transits(t, flux_batch, dy_batch=None, widths=None, k=8, min_ses=0.0, separation=0.5, gap_tolerance=0.5,
                    transit_depth_min=0.0, with_arrays=False, detrend=None, context=None, device=None, devices=None,
                    **template_kwargs):
    """The single-transit ("mono-transit") search of every light curve of flux_batch [n_curves, n] on the shared ascending
    time stamps t, on the device (tls_single_transits): a planet that transits once in the window has no periodogram peak,
    so the limb-darkened template of every trial width slides along the time series itself instead of along a fold.

    With dt = median(diff(t)), row r is (L_r = widths[r] samples, b_r = 1 - template.reference_transit(L_r, **shape),
    span_max[r] = (L_r - 1) * dt * (1 + gap_tolerance) days); widths=None takes single_transit_widths(t).  The shape comes
    from the keywords and presets of power() -- transit_template, u, limb_dark, per, rp, a, ... -- in template_kwargs, and
    y, dy are what a search of the same rows gets (dy_batch None: the row's standard deviation).

        w = 1 / dy^2;  xw = (1 - y) w
        for every centre c, rows ascending:  h = (L - 1) // 2;  lo = c - h;  hi = lo + L - 1
            skip if the window leaves the series or t[hi] - t[lo] > span_max[r]      (it runs over a gap)
            N = sum_j xw[lo+j] b[j];  D = sum_j w[lo+j] b[j]^2;  d = N / D           (the least-squares depth)
            skip unless d > transit_depth_min;  s = N / sqrt(D)                      (sqrt of the chi^2 the template removes)
            keep the row of the largest s (the first on ties):  ses[c], row[c], depth[c];  NaN, -1, NaN without one
        events: alive = ses >= min_ses (None: every centre with a row); at most k times the alive centre of the largest ses
        (the lowest index on ties) is taken, and with g = int(separation * L) every alive centre whose own window meets
        [lo - g, hi + g] leaves -- a transit longer than the longest row would otherwise return as wing events.

    Each step is one IEEE double operation and every sum runs in index order, so the result is bit-equal to the Python
    statement in tests/single_transit_spec.py.  Widths are strictly ascending integers in [3, 4096], k is in [1, 32],
    separation, gap_tolerance and transit_depth_min are finite and >= 0: ValueError otherwise, before any device work (the
    detrending included).  The rows -- t finite and non-decreasing with n <= 2^20, flux and dy as a search takes them -- are
    checked behind the detrending steps, before the search's own device work.  detrend= takes the steps and tuples of search_batch, devices=[...] deals the curves out over several GPUs.

    Returns (events, n_events): a structured array [n_curves, k] with the fields single_event_fields() -- index, time, ses,
    depth, row, width, t_first, t_last, duration_days; index -1 and NaN past a curve's n_events [n_curves] -- and, with
    with_arrays=True, the planes ses, row and depth [n_curves, n] behind them."""
    from ._lib import single_options, single_widths
    from .template import reference_transit
    depth_min, k, min_ses, separation = single_options(transit_depth_min, k, min_ses, separation)
    if isinstance(gap_tolerance, bool) or not (0.0 <= float(gap_tolerance) < numpy.inf):
        raise ValueError("single transits: gap_tolerance must be finite and >= 0, got %r" % (gap_tolerance,))
    if widths is not None:
        widths = single_widths(widths)
    flux_batch = _detrended(t, flux_batch, detrend, context, device, devices, dy_batch)
    kwargs = dict(template_kwargs)
    kwargs.setdefault("oversampling_factor", 1)      # (the period grid of the plan inputs is not used: the coarsest will do)
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, kwargs)
    if widths is None:
        widths = single_transit_widths(inp["t"])
    dt = float(numpy.median(numpy.diff(inp["t"]))) if len(inp["t"]) > 1 else 0.0
    shapes = [1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in widths]
    span_max = [(int(L) - 1) * dt * (1 + float(gap_tolerance)) for L in widths]

    def call(ctx, lo, hi):
        # (Context.single_transits checks the rows, single_arguments, before its device work)
        out = ctx.single_transits(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], widths, shapes, span_max, depth_min, k, min_ses,
                                  separation, with_arrays=with_arrays)
        return dict(zip(("events", "n_events", "ses", "row", "depth"), tuple(out) + (None,) * (5 - len(out))))

    out = _run_batch(devices, device, context, len(y_rows), call)
    raw = out["events"]
    events = numpy.zeros(raw.shape, dtype=[(f, "f8") for f in single_event_fields()])
    for f in raw.dtype.names:
        events[f] = raw[f]
    events["duration_days"] = raw["width"] * dt
    if with_arrays:
        return events, out["n_events"], out["ses"], out["row"], out["depth"]
    return events, out["n_events"]


# ---- individual transit times and a refitted ephemeris ---------------------------------------------------------------------
# what power_batch(..., transit_times=True) adds to the `peaks` array, and the ephemeris field each comes from
TRANSIT_TIMES_PEAK_FIELDS = (("tt_status", "status"), ("tt_n_timed", "n_timed"), ("tt_period", "period"),
                             ("tt_period_err", "period_err"), ("tt_T0", "T0"), ("tt_T0_err", "T0_err"),
                             ("tt_chi2", "ttv_chi2"), ("tt_rms", "ttv_rms"), ("tt_max_sigma", "ttv_max_sigma"))
TRANSIT_TIMES_GAP_TOLERANCE = 0.5


def ephemeris_fields():
    """The fields of a refitted ephemeris, in order: those of tls_ephemeris."""
    from ._lib import EPHEMERIS_FIELDS
    return tuple(EPHEMERIS_FIELDS)


def transit_time_fields():
    """The fields of one timed transit, in order: those of tls_transit_time -- epoch, status, time_linear, time, time_err,
    ses, depth, index -- and oc = time - (T0_fit + epoch * period_fit), formed on the host."""
    from ._lib import TRANSIT_TIME_FIELDS
    return tuple(TRANSIT_TIME_FIELDS) + ("oc",)


def _transit_times_options(search, min_ses, gap_tolerance=TRANSIT_TIMES_GAP_TOLERANCE, transit_depth_min=0.0,
                           max_epochs=None, what="transit times"):
    """(search, min_ses, gap_tolerance, depth_min, max_epochs) of transit_times, checked: search and gap_tolerance numbers,
    search finite and > 0, gap_tolerance finite and >= 0; the others as _lib.transit_times_options checks them (max_epochs
    None stays None).  ValueError otherwise, headed `what`."""
    from ._lib import transit_times_options
    search = _checks.finite_positive(what, "search", search)
    gap_tolerance = _checks.finite_at_least(what, "gap_tolerance", gap_tolerance)
    depth_min, min_ses, epochs = transit_times_options(transit_depth_min, min_ses, 1 if max_epochs is None else max_epochs, what)
    return search, min_ses, gap_tolerance, depth_min, None if max_epochs is None else epochs


def _transit_times_request(transit_times, peak_fits, search, min_ses):
    """None, or the checked (search, min_ses) of a transit_times=True request (ValueError for a bad one, and for
    transit_times without peak_fits)."""
    if not transit_times:
        return None
    if not peak_fits:
        raise ValueError("transit_times=True needs peak_fits=True: the times start from T0 and duration of the fits")
    return _transit_times_options(search, min_ses)[:2]


def transit_time_rows(t, period, duration, search=1.0, gap_tolerance=TRANSIT_TIMES_GAP_TOLERANCE, what="transit times"):
    """(widths, span_max, row, reach) of transit_times for candidates of `period` and `duration` [n_fits] (days) on the
    time stamps t: with dt = median(diff(t)), L_f = clip(int(round(duration_f / dt)), 3, min(4096, n)); widths are the sorted
    distinct L_f, row[f] the index of L_f among them, span_max[r] = (L_r - 1) * dt * (1 + gap_tolerance), and
    reach_f = max(1, min(int(search * L_f), (int(P_f / dt) - 1) // 2, 4096)) -- two epochs never share a centre (a period that
    is not finite and > 0 gets reach 1: the device reports status 1).  ValueError, headed `what`, for fewer than 3 time
    stamps, a cadence or a duration that is not finite and > 0."""
    from ._lib import SINGLE_MAX_WIDTH, SINGLE_MIN_WIDTH, TIMES_MAX_REACH
    t = numpy.asarray(t, dtype=numpy.float64)
    if t.ndim != 1 or len(t) < SINGLE_MIN_WIDTH:
        raise _checks.refusal(what, "t must hold at least %d time stamps" % SINGLE_MIN_WIDTH)
    dt = float(numpy.median(numpy.diff(t)))
    if not (0.0 < dt < numpy.inf):
        raise _checks.refusal(what, "the median cadence of t must be finite and > 0, got %r" % dt)
    period = numpy.atleast_1d(numpy.asarray(period, dtype=numpy.float64))
    duration = numpy.atleast_1d(numpy.asarray(duration, dtype=numpy.float64))
    if duration.size and not numpy.all((duration > 0.0) & (duration < numpy.inf)):
        raise _checks.refusal(what, "every duration must be finite and > 0 days")
    top = min(SINGLE_MAX_WIDTH, len(t))
    L = numpy.array([min(max(int(round(float(d) / dt)), SINGLE_MIN_WIDTH), top) for d in duration], dtype=numpy.int64)
    widths = numpy.unique(L)
    row = numpy.searchsorted(widths, L).astype(numpy.int64)
    span_max = [(int(w) - 1) * dt * (1 + float(gap_tolerance)) for w in widths]
    reach = numpy.ones(len(L), dtype=numpy.int64)
    for f, P in enumerate(period):
        if 0.0 < P < numpy.inf:
            apart = (int(min(float(P) / dt, 4.0 * TIMES_MAX_REACH)) - 1) // 2
            reach[f] = max(1, min(int(float(search) * int(L[f])), apart, TIMES_MAX_REACH))
    return widths, span_max, row, reach


def _epoch_counts(t, period, T0):
    """n_epochs of every candidate as the statement forms it; NaN without an ephemeris."""
    period, T0 = numpy.asarray(period, dtype=numpy.float64), numpy.asarray(T0, dtype=numpy.float64)
    with numpy.errstate(all="ignore"):
        count = (numpy.floor((t[-1] - T0) / period) - numpy.ceil((t[0] - T0) / period)) + 1.0
    return numpy.where(numpy.isfinite(period) & numpy.isfinite(T0) & (period > 0.0), count, numpy.nan)


def _most_epochs(t, period, T0):
    """The default max_epochs of transit_times and event_vetting: the largest epoch count among the candidates that have
    between 1 and TIMES_MAX_EPOCHS epochs inside the series; 1 without such a candidate."""
    from ._lib import TIMES_MAX_EPOCHS
    counts = _epoch_counts(t, period, T0)
    counts = counts[(counts >= 1.0) & (counts <= TIMES_MAX_EPOCHS)]
    return int(counts.max()) if len(counts) else 1


def _with_oc(ephemeris, times):
    """The device's epoch records plus oc = time - (T0_fit + epoch * period_fit), NaN where either is: the final table is
    allocated once and filled through its float view, one pass for the records and one for oc."""
    names = transit_time_fields()
    times = numpy.ascontiguousarray(times)
    out = numpy.empty(times.shape, dtype=[(k, "f8") for k in names])
    raw = times.view(numpy.float64).reshape(times.shape + (len(names) - 1,))
    flat = out.view(numpy.float64).reshape(times.shape + (len(names),))
    flat[..., :-1] = raw
    epoch, time = raw[..., names.index("epoch")], raw[..., names.index("time")]
    flat[..., -1] = time - (ephemeris["T0"][..., None] + epoch * ephemeris["period"][..., None])
    return out


def _with_ephemeris(records, ephemeris):
    """The peaks (with their fits) plus the tt_ fields of the device's ephemeris records."""
    return _joined(records, _block(ephemeris, *zip(*TRANSIT_TIMES_PEAK_FIELDS)))


def _peak_candidates(peaks, fits, keep=None):
    """(period, T0, duration, curve, fitted) of the peaks of a slice of the batch as candidates, flat over [n_curves * K]:
    the period of the peak and T0 and duration_days of its fit record where the fit status is 0 (and `keep`, where one is
    given, holds), NaN elsewhere -- every peak is a candidate, so the device writes a whole table in place, and one without
    an ephemeris comes back as its statement has it, status 1 and NaN in every other field; curve = the peak's curve."""
    n_curves, k = fits.shape
    fitted = (fits["status"] == 0).reshape(-1)
    if keep is not None:
        fitted = fitted & keep
    period = numpy.where(fitted, peaks["period"].reshape(-1), numpy.nan)
    T0 = numpy.where(fitted, fits["T0"].reshape(-1), numpy.nan)
    duration = numpy.where(fitted, fits["duration_days"].reshape(-1), numpy.nan)
    return period, T0, duration, numpy.repeat(numpy.arange(n_curves), k), fitted


def _peak_rows(inp, period, duration, fitted, rows_of, fill=()):
    """(widths, shapes, span_max, per) of the fitted candidates: the rows rows_of(t, period, duration) gives them
    (transit_time_rows, event_vetting_rows) with every row's template, and `per`, its per-candidate arrays over ALL
    candidates -- row 0, reach 1 and then `fill` where nothing was fitted."""
    from .template import reference_transit
    per = [numpy.zeros(len(fitted), dtype=numpy.int64), numpy.ones(len(fitted), dtype=numpy.int64)]
    per += [numpy.full(len(fitted), value) for value in fill]
    widths, span_max = numpy.array([3], dtype=numpy.int64), [0.0]        # (no fitted peak: one row nobody reads)
    if fitted.any():
        widths, span_max, *found = rows_of(inp["t"], period[fitted], duration[fitted])
        for target, values in zip(per, found):
            target[fitted] = values
    shapes = [1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in widths]
    return widths, shapes, span_max, per


def _peak_transit_times(ctx, env, request):
    """tt_ephemeris [n_curves, K] and tt_times [n_curves, K, max_epochs] of the peaks of a slice of the batch, on ctx."""
    from ._lib import TIMES_MAX_EPOCHS
    search, min_ses = request
    max_epochs = min(env.max_epochs, TIMES_MAX_EPOCHS)
    period, T0, duration, curve, fitted = _peak_candidates(env.peaks, env.fits)
    widths, shapes, span_max, (row, reach) = _peak_rows(
        env.inp, period, duration, fitted, lambda t, P, d: transit_time_rows(t, P, d, search))
    eph, times = ctx.transit_times(env.inp["t"], env.y_rows, env.dy_rows, period, T0, row, reach, widths, shapes, span_max,
                                   curve=curve, min_ses=min_ses, max_epochs=int(max_epochs))
    return dict(tt_ephemeris=eph.reshape(env.fits.shape), tt_times=times.reshape(env.fits.shape + (int(max_epochs),)))


def transit_times(t, flux_batch, period, T0, duration, curve=None, dy_batch=None, search=1.0, min_ses=3.0,
                  gap_tolerance=TRANSIT_TIMES_GAP_TOLERANCE, transit_depth_min=0.0, max_epochs=None, detrend=None,
                  context=None, device=None, **template_kwargs):
    """The individual transit times and the refitted ephemeris of candidates the caller holds, on the device
    (tls_transit_times): candidate f is (period[f], T0[f], duration[f] in days) on light curve curve[f] of flux_batch
    [n_curves, n] (or one row [n]) over the ascending time stamps t; curve=None takes one candidate a curve, in order.  It
    needs no search.  TLS assumes a strictly linear ephemeris; planets near resonance transit hours early and late, and a
    candidate that rests on one or two events looks the same in the summary as a clean planet.  The table of observed-minus-
    computed times tells them apart, and the line through the times is the (period, T0) of every follow-up, with errors that
    come from the transits themselves.

    With dt = median(diff(t)), candidate f gets the template of L_f = clip(int(round(duration_f / dt)), 3, min(4096, n))
    samples, b = 1 - template.reference_transit(L_f, **shape) -- the shape from the keywords and presets of power() in
    template_kwargs --, span_max = (L_f - 1) * dt * (1 + gap_tolerance) and reach_f = max(1, min(int(search * L_f),
    (int(P_f / dt) - 1) // 2, 4096)) (transit_time_rows); y and dy are what a search of the same rows gets.

        w = 1 / dy^2;  xw = (1 - y) w;  g[j] = (b[j+1] - b[j-1]) / 2                     (the shape's slope per sample)
        for every epoch e with t[0] <= tc = T0 + e P <= t[n-1]:  j = the sample nearest tc
            for s = -reach .. reach:  the window of L samples centred on c = j + s, skipped where it leaves the series or runs
                over a gap;  N = sum xw b;  D = sum w b^2;  d = N / D;  skipped unless d > transit_depth_min;  q = N / sqrt(D)
            the shift of the largest q is held (the first on ties): ses = q, depth = d, index = c
            one Gauss-Newton step of the shift over the whole window -- a matched filter, not a parabola through three noisy
            values:  H = sum xw g;  Bg = sum w b g;  G = sum w g^2;  delta = (d Bg - H) / (d G) samples
            time = (the window's centre) + delta * step;  time_err = step / (d sqrt(G)),  step = (t[c+1] - t[c-1]) / 2
        the weighted straight line through (e, time) of the timed epochs: period, T0 and their errors from two or more, and
        from three or more the chi^2 and the root mean square of the residuals, the largest |o - c| / time_err and its epoch

    time_err is the Fisher bound of the shape at the fitted depth on white noise of the given dy: correlated noise and a
    wrong shape make the true scatter larger, so ttv_chi2 of a quiet star is of the order of n_timed - 2 only where both
    hold.  Epoch status: 0 timed; 1 no window with a dip (the epoch lies in a gap or at an end of the series); 2 a dip was
    found but not timed -- the step leaves its sample (|delta| > 1: the reach's edge, a shape that does not fit) or the
    series; 3 the dip is weaker than min_ses.  Candidate status: 0 its epochs were looked at; 1 no such ephemeris (period or
    T0 not finite, period <= 0); 2 it has no epoch inside the series, or more than max_epochs (None: the largest count among
    the candidates, at most 65536).

    Each step is one IEEE double operation and every sum runs in index order, so the result is bit-equal to the Python
    statement in tests/transit_times_spec.py.  search finite and > 0, gap_tolerance and transit_depth_min finite and >= 0,
    min_ses no NaN, max_epochs in [1, 65536], durations finite and > 0, period, T0, duration and curve [n_fits] with curve in
    [0, n_curves): ValueError otherwise, before any device work (the detrending included).  The rows -- flux and dy as a search
    takes them -- and the template keywords are checked behind the detrending steps, before the call's own device work.
    detrend= takes the steps and tuples of search_batch.

    Returns (ephemeris, times): a structured array [n_fits] with the fields ephemeris_fields() -- status, n_epochs, n_timed,
    epoch_first, period, period_err, T0, T0_err, ttv_chi2, ttv_rms, ttv_max_sigma, ttv_max_epoch -- and one [n_fits,
    max_epochs] with the fields transit_time_fields() -- epoch, status, time_linear, time, time_err, ses, depth, index and
    oc = time - (T0_fit + epoch * period_fit); NaN past a candidate's n_epochs."""
    search, min_ses, gap_tolerance, depth_min, max_epochs = _transit_times_options(search, min_ses, gap_tolerance,
                                                                                   transit_depth_min, max_epochs)
    t, flux_batch, dy_batch = _candidate_rows("transit times", t, flux_batch, dy_batch)
    period, T0, duration, curve = _checks.candidates("transit times", period, T0, duration, curve, numpy.shape(flux_batch)[0])
    widths, span_max, row, reach = transit_time_rows(t, period, duration, search, gap_tolerance)
    if max_epochs is None:
        max_epochs = _most_epochs(t, period, T0)
    inp, y_rows, dy_rows, ctx = _candidate_inputs(t, flux_batch, dy_batch, detrend, context, device, template_kwargs)
    from .template import reference_transit
    shapes = [1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in widths]
    eph, times = ctx.transit_times(inp["t"], y_rows, dy_rows, period, T0, row, reach, widths, shapes, span_max, curve=curve,
                                   depth_min=depth_min, min_ses=min_ses, max_epochs=max_epochs)
    return eph, _with_oc(eph, times)


# ---- the period aliases of two- and few-transit events ---------------------------------------------------------------------
def event_pair_fields():
    """The fields of an event pair's record, in order: those of tls_event_pair."""
    from ._lib import EVENT_PAIR_FIELDS
    return tuple(EVENT_PAIR_FIELDS)


def event_alias_fields():
    """The fields of one alias of an event pair, in order: those of tls_event_alias."""
    from ._lib import EVENT_ALIAS_FIELDS
    return tuple(EVENT_ALIAS_FIELDS)


def _ratio(name, value, what="event pairs"):
    return _checks.finite_at_least(what, name, value, 1.0)


def event_pairs(events, n_events, min_ses=7.0, depth_ratio=2.0, width_ratio=2.0, max_pairs=8):
    """The pairs of single-transit events that may be two transits of one planet, on the host: per curve of `events`
    [n_curves, k] (the records of single_transits, n_events [n_curves] of them valid) every two events a, b with
    index_a < index_b that both reach min_ses and whose depths and widths agree within the ratios (larger / smaller <=
    depth_ratio, width_ratio), at most max_pairs a curve by descending ses_a^2 + ses_b^2 (the earlier pair on ties).  The row of
    a pair is that of its stronger event (a on ties).  Returns (curve, index_a, index_b, row), int64 [n_pairs], curve
    ascending.  ValueError for ratios below 1, a NaN min_ses, max_pairs < 1 and records without the fields index, ses, depth,
    width and row."""
    depth_ratio, width_ratio = _ratio("depth_ratio", depth_ratio), _ratio("width_ratio", width_ratio)
    _checks.no_nan("event pairs", "min_ses", min_ses)
    _checks.integer("event pairs", "max_pairs", max_pairs, 1)
    events = numpy.asarray(events)
    if events.dtype.names is None or not {"index", "ses", "depth", "width", "row"} <= set(events.dtype.names):
        raise ValueError("event pairs: events must be the records of single_transits")
    if events.ndim == 1:
        events = events[None, :]
    n_events = numpy.atleast_1d(numpy.asarray(n_events))
    if events.ndim != 2 or n_events.shape != (len(events),) or (n_events.size and (n_events.min() < 0
                                                                                     or n_events.max() > events.shape[1])):
        raise ValueError("event pairs: events must be [n_curves, k] with n_events [n_curves] in [0, k]")
    found = []
    for c in range(len(events)):
        ev = events[c, :int(n_events[c])]
        ev = ev[ev["ses"] >= float(min_ses)]
        ev = ev[numpy.argsort(ev["index"], kind="stable")]
        rows = []
        for i in range(len(ev)):
            for j in range(i + 1, len(ev)):
                a, b = ev[i], ev[j]
                if not a["index"] < b["index"]:
                    continue
                d = sorted((float(a["depth"]), float(b["depth"])))
                w = sorted((float(a["width"]), float(b["width"])))
                if not (d[0] > 0.0 and d[1] <= depth_ratio * d[0] and w[1] <= width_ratio * w[0]):
                    continue
                strength = float(a["ses"]) ** 2 + float(b["ses"]) ** 2
                rows.append((-strength, int(a["index"]), int(b["index"]), int(a["row"] if a["ses"] >= b["ses"] else b["row"])))
        rows.sort()
        found += [(c,) + r[1:] for r in rows[:int(max_pairs)]]
    out = numpy.array(found, dtype=numpy.int64).reshape(-1, 4)
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy()


def event_period_reach(widths, row, dt):
    """(reach, offset) of event_periods' defaults for pairs on the rows `row` of `widths`: reach_f = max(1, min(L_f // 4,
    4096)) samples and offset_f = (reach_f + 0.5) * dt days."""
    from ._lib import TIMES_MAX_REACH
    L = numpy.asarray(widths, dtype=numpy.int64)[numpy.asarray(row, dtype=numpy.int64)]
    reach = numpy.maximum(1, numpy.minimum(L // 4, TIMES_MAX_REACH)).astype(numpy.int64)
    return reach, (reach + 0.5) * float(dt)


def event_periods(t, flux_batch, events=None, n_events=None, pairs=None, dy_batch=None, period_min=None, max_aliases=256,
                  reach=None, min_ses=3.0, veto_sigma=3.0, widths=None, gap_tolerance=0.5, with_aliases=True, detrend=None,
                  context=None, device=None, devices=None, **template_kwargs):
    """The periods two or a few single-transit events of a star allow, on the device (tls_event_periods).  Two events -- two
    TESS sectors a year apart, a K2 campaign with a gap, a 40-day planet in a 90-day window -- have no periodogram peak, but they
    fix the period up to the aliases P_k = (t_b - t_a) / k, and the data decide among them: an alias is ruled out when one of
    its other epochs falls on good data that show no dip, allowed when they all fall in gaps, and confirmed when another epoch
    shows a dip.  This is the table of allowed periods a duo-transit follow-up starts from.

    The pairs are `pairs` = (curve, index_a, index_b, row) -- sample indices index_a < index_b on light curve curve of
    flux_batch [n_curves, n] (or one row), row an index into `widths` --, or event_pairs(events, n_events) of the records of
    single_transits, or, with neither, those of single_transits on the same detrended rows (the rows are detrended once).  The
    rows are single_transits': with dt = median(diff(t)), row r is (L_r = widths[r], b_r = 1 - template.reference_transit(L_r,
    **shape), span_max = (L_r - 1) * dt * (1 + gap_tolerance)); widths=None takes single_transit_widths(t), so the rows of
    single_transits' events fit.  reach (None: max(1, min(L // 4, 4096)) of the pair's row; an integer, or one a pair) is how far
    a dip may lie from an epoch, in samples, offset = (reach + 0.5) * dt, and period_min=None is 4 times the longest row's
    duration.

        look(tc): among the centres within reach of the sample nearest tc and within offset of tc whose window is whole and runs
            over no gap, the one of the largest q = N / sqrt(D) (N = sum xw b, D = sum w b^2; signed, no depth threshold: a
            missing dip must count); no such centre: the epoch is uncovered
        the pair: both events covered and N_a + N_b > 0;  pair_depth = (N_a + N_b) / (D_a + D_b)
        alias k = 1 .. min(floor(dT / period_min), max_aliases):  P = dT / k;  over its epochs inside the series:
            n_covered, n_seen (q >= min_ses), mes = sum N / sqrt(sum D), depth = sum N / sum D
            worst_sigma = the largest (pair_depth - N / D) sqrt(D) over the covered epochs other than the pair's own
        allowed(k) = not (worst_sigma > veto_sigma): an alias without another covered epoch is allowed
        best = the allowed alias of the largest mes; longest / shortest = the allowed aliases of the smallest / largest k

    Pair status: 0 its aliases were looked at; 1 the two events share a time stamp; 2 an event is uncovered (its window runs over
    a gap or an end) or the two show no dip; 3 no alias is as long as period_min.  Each step is one IEEE double operation and
    every sum runs in index order, so the result is bit-equal to the Python statement in tests/event_periods_spec.py.
    ValueError, before any device work (the detrending included), for period_min not finite and > 0, max_aliases outside
    [1, 4096], a NaN min_ses or veto_sigma (inf: no veto), a bad reach, gap_tolerance or widths and `pairs` out of range; the rows
    (and the events of a call without pairs) are checked behind the detrending steps, before the call's own device work.  detrend= takes the steps and tuples of
    search_batch; devices=[...] deals the pairs out by their curves.

    Returns (pairs, aliases): a structured array [n_pairs] with curve, index_a, index_b, row, reach, offset and the fields
    event_pair_fields(), and one [n_pairs, max_aliases] with k, allowed and the fields event_alias_fields() (NaN, not allowed,
    past n_evaluated); aliases is None with with_aliases=False."""
    from ._lib import TIMES_MAX_REACH, event_periods_options, single_widths
    from .template import reference_transit
    _, max_aliases, min_ses, veto_sigma = event_periods_options(1.0 if period_min is None else period_min, max_aliases,
                                                                 min_ses, veto_sigma)
    if isinstance(gap_tolerance, bool) or not (0.0 <= float(gap_tolerance) < numpy.inf):
        raise ValueError("event periods: gap_tolerance must be finite and >= 0, got %r" % (gap_tolerance,))
    if widths is not None:
        widths = single_widths(widths, "event periods")
    if reach is not None:
        reach = numpy.asarray(reach)
        if reach.dtype.kind not in "iu" or reach.ndim > 1 or (reach.size and (reach.min() < 1 or reach.max() > TIMES_MAX_REACH)):
            raise ValueError("event periods: reach must be integers in [1, %d]" % TIMES_MAX_REACH)
    if pairs is not None and (events is not None or n_events is not None):
        raise ValueError("event periods: give pairs or events, not both")
    if (events is None) != (n_events is None):
        raise ValueError("event periods: events and n_events come together")
    t, flux_batch, dy_batch = _candidate_rows("event periods", t, flux_batch, dy_batch)
    if widths is None:
        widths = single_transit_widths(t)
    n_curves = numpy.shape(flux_batch)[0]

    def checked(pairs):
        if isinstance(pairs, dict):
            pairs = tuple(pairs[k] for k in ("curve", "index_a", "index_b", "row"))
        if len(pairs) != 4:
            raise ValueError("event periods: pairs must be (curve, index_a, index_b, row)")
        curve, index_a, index_b, row = (numpy.atleast_1d(numpy.asarray(v)) for v in pairs)
        for name, v, hi in (("curve", curve, n_curves), ("index_a", index_a, len(t)), ("index_b", index_b, len(t)),
                            ("row", row, len(widths))):
            if v.ndim != 1 or v.shape != curve.shape or (v.size and (v.dtype.kind not in "iu" or v.min() < 0 or v.max() >= hi)):
                raise ValueError("event periods: %s must hold one index in [0, %d) a pair" % (name, hi))
        if not numpy.all(index_a < index_b):
            raise ValueError("event periods: index_a must lie in front of index_b")
        if reach is not None and reach.ndim == 1 and reach.shape != curve.shape:
            raise ValueError("event periods: reach must be one integer, or one a pair")
        return tuple(v.astype(numpy.int64) for v in (curve, index_a, index_b, row))

    if pairs is not None:
        pairs = checked(pairs)                       # (what the caller gave is checked in front of the detrending)
    flux_batch = _detrended(t, flux_batch, detrend, context, device, devices, dy_batch)
    if pairs is None:
        if events is None:
            events, n_events = single_transits(t, flux_batch, dy_batch, widths=widths, gap_tolerance=gap_tolerance,
                                               context=context, device=device, devices=devices, **template_kwargs)
        pairs = checked(event_pairs(events, n_events))
    curve, index_a, index_b, row = pairs
    kwargs = dict(template_kwargs)
    kwargs.setdefault("oversampling_factor", 1)      # (the period grid of the plan inputs is not used: the coarsest will do)
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, kwargs)
    dt = float(numpy.median(numpy.diff(inp["t"]))) if len(inp["t"]) > 1 else 0.0
    shapes = [1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in widths]
    span_max = [(int(L) - 1) * dt * (1 + float(gap_tolerance)) for L in widths]
    default_reach, _ = event_period_reach(widths, row, dt)
    if reach is None:
        reach = default_reach
    else:
        reach = numpy.broadcast_to(reach, curve.shape).astype(numpy.int64)
    offset = (reach + 0.5) * dt
    if period_min is None:
        period_min = 4.0 * float(numpy.max(widths)) * dt
    period_min = event_periods_options(period_min)[0]

    def call(ctx, lo, hi):
        where = numpy.flatnonzero((curve >= lo) & (curve < hi))
        rec, table = ctx.event_periods(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], curve[where] - lo, index_a[where],
                                       index_b[where], row[where], reach[where], offset[where], widths, shapes, span_max,
                                       period_min, max_aliases, min_ses, veto_sigma, with_aliases=with_aliases)
        return dict(where=where, pairs=rec, aliases=table)

    out = _run_batch(devices, device, context, n_curves, call)
    from ._lib import EVENT_ALIAS_DTYPE, EVENT_PAIR_DTYPE
    back = numpy.empty(len(curve), dtype=numpy.int64)
    back[out["where"]] = numpy.arange(len(curve))
    raw = out["pairs"][back]
    records = numpy.zeros(len(curve), dtype=[(k, "i8") for k in ("curve", "index_a", "index_b", "row", "reach")]
                          + [("offset", "f8")] + EVENT_PAIR_DTYPE.descr)
    for name, v in (("curve", curve), ("index_a", index_a), ("index_b", index_b), ("row", row), ("reach", reach),
                    ("offset", offset)):
        records[name] = v
    for name in raw.dtype.names:
        records[name] = raw[name]
    if not with_aliases:
        return records, None
    table = out["aliases"][back]
    aliases = numpy.zeros(table.shape, dtype=[("k", "i8"), ("allowed", "?")] + EVENT_ALIAS_DTYPE.descr)
    aliases["k"] = numpy.arange(1, table.shape[1] + 1)[None, :]
    with numpy.errstate(invalid="ignore"):
        aliases["allowed"] = (aliases["k"] <= raw["n_evaluated"][:, None]) & ~(table["worst_sigma"] > veto_sigma)
    for name in table.dtype.names:
        aliases[name] = table[name]
    return records, aliases


# ---- per-transit event vetting ---------------------------------------------------------------------------------------------
EVENT_VETTING_CHASE_WINDOW = 0.1
EVENT_VETTING_GUARD = 1.5


def event_summary_fields():
    """The fields of a candidate's event vetting, in order: those of tls_event_summary.  power_batch(...,
    event_vetting=True) adds each to the `peaks` array behind the prefix ev_."""
    from ._lib import EVENT_SUMMARY_FIELDS
    return tuple(EVENT_SUMMARY_FIELDS)


def event_fields():
    """The fields of one vetted event, in order: those of tls_event_record -- epoch, status, time_linear, ses, depth,
    depth_err, index, point_share, before, after, chases, chase_dt, n_chased, flags."""
    from ._lib import EVENT_RECORD_FIELDS
    return tuple(EVENT_RECORD_FIELDS)


def _event_vetting_options(search, chase_window, guard, min_ses, chase_fraction, chase_min, point_fraction, step_fraction,
                           gap_tolerance=TRANSIT_TIMES_GAP_TOLERANCE, transit_depth_min=0.0, max_epochs=None):
    """The options of event_vetting, checked, as a dict: search, min_ses, gap_tolerance, depth_min and max_epochs as
    _transit_times_options checks them (its messages headed "event vetting"); chase_window a number, finite and > 0; guard a
    number, finite and >= 0; the four parameters as _lib.event_vetting_options checks them.  ValueError otherwise."""
    from ._lib import event_vetting_options
    search, min_ses, gap_tolerance, depth_min, max_epochs = _transit_times_options(
        search, min_ses, gap_tolerance, transit_depth_min, max_epochs, "event vetting")
    chase_window = _checks.finite_positive("event vetting", "chase_window", chase_window)
    guard = _checks.finite_at_least("event vetting", "guard", guard)
    chase_fraction, chase_min, point_fraction, step_fraction = event_vetting_options(chase_fraction, chase_min, point_fraction,
                                                                                     step_fraction)
    return dict(search=search, chase_window=chase_window, guard=guard, min_ses=min_ses,
                chase_fraction=chase_fraction, chase_min=chase_min, point_fraction=point_fraction,
                step_fraction=step_fraction, gap_tolerance=gap_tolerance, depth_min=depth_min, max_epochs=max_epochs)


def _event_vetting_request(event_vetting, peak_fits, search, chase_window, guard, min_ses, chase_fraction, chase_min,
                           point_fraction, step_fraction):
    """None, or the checked options of an event_vetting=True request (ValueError for a bad one, and for event_vetting
    without peak_fits)."""
    if not event_vetting:
        return None
    if not peak_fits:
        raise ValueError("event_vetting=True needs peak_fits=True: the events start from T0 and duration of the fits")
    return _event_vetting_options(search, chase_window, guard, min_ses, chase_fraction, chase_min, point_fraction,
                                  step_fraction)


def event_vetting_rows(t, period, duration, search=1.0, chase_window=EVENT_VETTING_CHASE_WINDOW, guard=EVENT_VETTING_GUARD,
                       gap_tolerance=TRANSIT_TIMES_GAP_TOLERANCE, what="transit times"):
    """(widths, span_max, row, reach, chase_reach, guard, chase_span) of event_vetting for candidates of `period` and
    `duration` [n_fits] (days) on the time stamps t: the four arrays of transit_time_rows, and with dt = median(diff(t)) and
    L_f the candidate's width, chase_reach_f = min(int(chase_window * P_f / dt), 8192) samples, guard_f = int(guard * L_f)
    samples and chase_span_f = chase_window * P_f days.  Where the cap of 8192 samples bites, the span stays
    chase_window * P: `chases` keeps its meaning as a fraction of the period, and the windows beyond the cap are not looked
    at.  A period that is not finite and > 0 gets chase_reach 0 and chase_span 1 (the device reports status 1)."""
    from ._lib import EVENTS_MAX_CHASE
    widths, span_max, row, reach = transit_time_rows(t, period, duration, search, gap_tolerance, what)
    dt = float(numpy.median(numpy.diff(numpy.asarray(t, dtype=numpy.float64))))
    period = numpy.atleast_1d(numpy.asarray(period, dtype=numpy.float64))
    chase_reach = numpy.zeros(len(period), dtype=numpy.int64)
    guards = numpy.zeros(len(period), dtype=numpy.int64)
    chase_span = numpy.ones(len(period), dtype=numpy.float64)
    for f, P in enumerate(period):
        guards[f] = int(float(guard) * int(widths[row[f]]))
        if 0.0 < P < numpy.inf:
            span = float(chase_window) * float(P)
            if 0.0 < span < numpy.inf:
                chase_reach[f] = int(min(span / dt, float(EVENTS_MAX_CHASE)))
                chase_span[f] = span
    return widths, span_max, row, reach, chase_reach, guards, chase_span


def _with_events(records, summaries):
    """The peaks (with whatever they carry) plus the ev_ fields of the device's event summaries."""
    return _joined(records, _block(summaries, ["ev_" + k for k in event_summary_fields()]))


def _peak_event_vetting(ctx, env, request):
    """ev_summaries [n_curves, K] and ev_events [n_curves, K, max_epochs] of the peaks of a slice of the batch, on ctx."""
    from ._lib import TIMES_MAX_EPOCHS
    max_epochs = min(env.max_epochs, TIMES_MAX_EPOCHS)
    period, T0, duration, curve, fitted = _peak_candidates(env.peaks, env.fits)
    widths, shapes, span_max, (row, reach, chase_reach, guard, chase_span) = _peak_rows(
        env.inp, period, duration, fitted,
        lambda t, P, d: event_vetting_rows(t, P, d, request["search"], request["chase_window"], request["guard"]), (0, 0, 1.0))
    out, events = ctx.event_vetting(env.inp["t"], env.y_rows, env.dy_rows, period, T0, row, reach, chase_reach, guard,
                                    chase_span, widths, shapes, span_max, curve=curve, min_ses=request["min_ses"],
                                    chase_fraction=request["chase_fraction"], chase_min=request["chase_min"],
                                    point_fraction=request["point_fraction"], step_fraction=request["step_fraction"],
                                    max_epochs=int(max_epochs))
    return dict(ev_summaries=out.reshape(env.fits.shape), ev_events=events.reshape(env.fits.shape + (int(max_epochs),)))


def event_vetting(t, flux_batch, period, T0, duration, curve=None, dy_batch=None, search=1.0,
                  chase_window=EVENT_VETTING_CHASE_WINDOW, guard=EVENT_VETTING_GUARD, min_ses=3.0, chase_fraction=0.6,
                  chase_min=0.5, point_fraction=0.5, step_fraction=0.5, gap_tolerance=TRANSIT_TIMES_GAP_TOLERANCE,
                  transit_depth_min=0.0, max_epochs=None, detrend=None, context=None, device=None, **template_kwargs):
    """The vetting of the INDIVIDUAL events of candidates the caller holds, on the device (tls_event_vetting): candidate f is
    (period[f], T0[f], duration[f] in days) on light curve curve[f] of flux_batch [n_curves, n] (or one row [n]) over the
    ascending time stamps t; curve=None takes one candidate a curve, in order.  It needs no search.  Every other vetting test
    judges the stacked signal; a candidate of three to six transits can be three unrelated events -- an outlier, a sensitivity
    step with its recovery, a detrending wiggle -- that line up on a linear ephemeris, and passes them all.  These tests are
    the Kepler Robovetter's individual transit metrics (Thompson et al. 2018, A.3.7): Chases, Marshall / Zuma in the plain
    form of a one-sample and a baseline test, and Rubble as the counts.

    Rows, template, reach, y and dy are those of transit_times (transit_time_rows); with dt = median(diff(t)),
    chase_reach_f = min(int(chase_window * P_f / dt), 8192), guard_f = int(guard * L_f), chase_span_f = chase_window * P_f
    (event_vetting_rows).

        every epoch: the held window as transit_times finds it (the largest q = N / sqrt(D) over the shifts): ses, depth, index
            point_share = (the largest term of N) / N                        > point_fraction: the event rests on one sample
            before, after = the mean dip of the L samples on either side of the window, over the depth
                                                                             > step_fraction: the flux is not at the baseline
            chase: every window centred guard_f + 1 .. chase_reach_f samples to either side of the event; one whose
                |q'| >= chase_fraction * q is comparable (a bump counts as a dip does);  chase_dt = the distance in days to the
                nearest comparable one;  chases = min(chase_dt / chase_span, 1), 1 without one  < chase_min: not unique
            flags = 1 (ses < min_ses) | 2 (point) | 4 (step) | 8 (chased); an event without a flag is good
        the candidate: n_held, n_good; mes = SN / sqrt(SD) over the held events, mes_good over the good ones, mes_rest over all
            but the strongest; ses_max, its epoch and dominance = ses_max / mes; depth_mean and the chi^2 of the events' depths
            about it; the least and the mean chases

    mes is formed from every event's BEST shift, so it is biased upward against a strictly linear ephemeris: compare it with
    mes_good and mes_rest, which are formed the same way, not with the search's SNR.  Event status: 0 an event is held; 1 no
    window with a dip.  Candidate status as transit_times has it.

    Each step is one IEEE double operation and every sum runs in index order (the chase's minimum and count do not depend on
    an order), so the result is bit-equal to the Python statement in tests/event_vetting_spec.py.  The arguments are checked
    as transit_times checks its own; chase_window finite and > 0, guard finite and >= 0, chase_fraction in (0, 1], chase_min
    in [0, 1], point_fraction and step_fraction > 0: ValueError otherwise, before any device work.  detrend= takes the steps
    and tuples of search_batch.

    Returns (summary, events): a structured array [n_fits] with the fields event_summary_fields() and one [n_fits,
    max_epochs] with the fields event_fields(); NaN past a candidate's n_epochs."""
    o = _event_vetting_options(search, chase_window, guard, min_ses, chase_fraction, chase_min, point_fraction, step_fraction,
                               gap_tolerance, transit_depth_min, max_epochs)
    t, flux_batch, dy_batch = _candidate_rows("event vetting", t, flux_batch, dy_batch)
    period, T0, duration, curve = _checks.candidates("event vetting", period, T0, duration, curve, numpy.shape(flux_batch)[0])
    widths, span_max, row, reach, chase_reach, guards, chase_span = event_vetting_rows(
        t, period, duration, o["search"], o["chase_window"], o["guard"], o["gap_tolerance"], "event vetting")
    max_epochs = _most_epochs(t, period, T0) if o["max_epochs"] is None else o["max_epochs"]
    inp, y_rows, dy_rows, ctx = _candidate_inputs(t, flux_batch, dy_batch, detrend, context, device, template_kwargs)
    from .template import reference_transit
    shapes = [1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in widths]
    return ctx.event_vetting(inp["t"], y_rows, dy_rows, period, T0, row, reach, chase_reach, guards, chase_span, widths, shapes,
                             span_max, curve=curve, depth_min=o["depth_min"], min_ses=o["min_ses"],
                             chase_fraction=o["chase_fraction"], chase_min=o["chase_min"], point_fraction=o["point_fraction"],
                             step_fraction=o["step_fraction"], max_epochs=max_epochs)


# ---- trapezoid shape fit and transit geometry --------------------------------------------------------------------------------
SHAPE_FIT_RATIOS = numpy.geomspace(0.5, 2.0, 17)
SHAPE_FIT_INGRESS = numpy.linspace(0.0, 0.5, 16)
SHAPE_FIT_SHIFTS = numpy.linspace(-0.25, 0.25, 9)


def shape_fit_fields():
    """The fields of a shape fit, in order -- what shape_fit returns and power_batch(..., shape_fit=True) adds to the `peaks`
    array: the fields of tls_shape_record, each behind the prefix shape_ (shape_status first; the peaks array has depth,
    duration and status of its own), then shape_delta_chi2 = ses^2 - ses_vee^2 and the geometry of the best trapezoid
    (transit_geometry): shape_impact, shape_a_rs, shape_rho_star."""
    from ._lib import SHAPE_FIELDS
    return tuple("shape_" + k for k in SHAPE_FIELDS) + ("shape_delta_chi2", "shape_impact", "shape_a_rs", "shape_rho_star")


def transit_geometry(period, depth, duration, ingress):
    """(impact, a_rs, rho_star) of a trapezoid of `depth`, total duration `duration` = T14 (days) and ingress fraction
    `ingress` = T12/T14 at `period` (days): the analytic solution of Seager & Mallen-Ornelas (2003, ApJ 585, 1038, their
    equations 7, 8 and 9) for a circular orbit and a star without limb darkening.  Plain numpy on the host, broadcasting.

        tT = duration;  tF = duration * (1 - 2 ingress);  k = sqrt(depth);  sT = sin^2(pi tT / P);  r = sin^2(pi tF / P) / sT
        b^2 = ((1 - k)^2 - r (1 + k)^2) / (1 - r)
        a_rs = sqrt(((1 + k)^2 - b^2 (1 - sT)) / sT)
        rho_star = 3 pi a_rs^3 / (G P^2), in units of the solar mean density

    impact is b, a_rs the semi-major axis in stellar radii and rho_star the stellar density the transit implies, to be compared
    with the catalogue's: a transit on another, blended star gives a different one.  NaN where b^2 < 0 -- no such geometry:
    the ingress is shorter than that of a central transit of this depth, sin(pi tF / P) / sin(pi tT / P) > (1 - k) / (1 + k),
    as for a box; a V, tF = 0, is the grazing b = 1 - k -- and where an input is not finite."""
    from . import constants as C
    period, depth, duration, ingress = numpy.broadcast_arrays(*(numpy.asarray(v, dtype=numpy.float64)
                                                                for v in (period, depth, duration, ingress)))
    with numpy.errstate(all="ignore"):
        k = numpy.sqrt(depth)
        sT = numpy.sin(numpy.pi * duration / period) ** 2
        sF = numpy.sin(numpy.pi * (duration * (1.0 - 2.0 * ingress)) / period) ** 2
        r = sF / sT
        b2 = ((1.0 - k) ** 2 - r * (1.0 + k) ** 2) / (1.0 - r)
        a_rs = numpy.sqrt(((1.0 + k) ** 2 - b2 * (1.0 - sT)) / sT)
        rho_sun = C.M_sun / (4.0 / 3.0 * numpy.pi * float(C.R_sun) ** 3)
        rho = 3.0 * numpy.pi * a_rs ** 3 / (C.G * (period * C.SECONDS_PER_DAY) ** 2) / rho_sun
        good = numpy.isfinite(period) & numpy.isfinite(depth) & numpy.isfinite(duration) & numpy.isfinite(ingress) \
            & (b2 >= 0.0) & numpy.isfinite(a_rs)
        impact = numpy.where(good, numpy.sqrt(numpy.where(good, b2, 0.0)), numpy.nan)
    return impact, numpy.where(good, a_rs, numpy.nan), numpy.where(good, rho, numpy.nan)


def _shape_fit_request(shape_fit, peak_fits, window, min_count):
    """None, or the checked (window, min_count) of a shape_fit=True request over the default tables (ValueError for a bad
    one, and for shape_fit without peak_fits)."""
    if not shape_fit:
        return None
    if not peak_fits:
        raise ValueError("shape_fit=True needs peak_fits=True: the fits start from T0 and duration of the fits")
    from ._lib import shape_fit_tables
    return shape_fit_tables(SHAPE_FIT_RATIOS, SHAPE_FIT_INGRESS, SHAPE_FIT_SHIFTS, window, min_count)[3:5]


def _with_shapes(records, shapes, period):
    """`records` (None, or the peaks with their fits) plus the device's shape records, shape_delta_chi2 and the geometry of
    the best trapezoid at `period`."""
    out = _block(shapes, shape_fit_fields())
    out["shape_delta_chi2"] = shapes["ses"] * shapes["ses"] - shapes["ses_vee"] * shapes["ses_vee"]
    out["shape_impact"], out["shape_a_rs"], out["shape_rho_star"] = transit_geometry(
        period, shapes["depth"], shapes["duration"], shapes["ingress"])
    return _joined(records, out)


def _peak_shape_fits(ctx, env, request):
    """shape_fits [n_curves, K]: the shape records of the peaks of a slice of the batch, on ctx."""
    window, min_count = request
    period, T0, duration, curve, _ = _peak_candidates(env.peaks, env.fits)
    out = ctx.shape_fit(env.inp["t"], env.y_rows, env.dy_rows, period, T0, duration, SHAPE_FIT_RATIOS, SHAPE_FIT_INGRESS,
                        SHAPE_FIT_SHIFTS, curve=curve, window=window, min_count=min_count)
    return dict(shape_fits=out.reshape(env.fits.shape))


def shape_fit(t, flux_batch, period, T0, duration, curve=None, dy_batch=None, ratios=None, ingress=None, shifts=None,
              window=2.0, min_count=3, transit_depth_min=0.0, detrend=None, context=None, device=None, **power_kwargs):
    """The shape of the dip of candidates the caller holds, on the device (tls_shape_fit): candidate f is (period[f], T0[f],
    duration[f] in days) on light curve curve[f] of flux_batch [n_curves, n] (or one row [n]) over the ascending time stamps
    t; curve=None takes one candidate a curve, in order.  It needs no search.  A grazing eclipsing binary, or a blend of one,
    is V-shaped; a planet has a flat bottom and a short ingress.  The search cannot tell: it matches one limb-darkened
    template whose duration moves in steps of 10 %.  Here a trapezoid of unit depth -- total duration T = T14, ingress
    fraction g = T12/T14, centre T0 + c0 -- is matched to the points within window * duration of every transit, with the
    baseline fixed at 1 as everywhere in TLS, over the grid of T = duration * ratios, g = ingress and c0 = duration * shifts
    (defaults: numpy.geomspace(0.5, 2.0, 17), numpy.linspace(0.0, 0.5, 16), numpy.linspace(-0.25, 0.25, 9): 2448 units);
    y and dy are what a search of the same rows gets (power_kwargs: the keywords of power()).

        w = 1 / dy^2;  xw = (1 - y) w
        status 1 and NaN in every other field unless P, T0, d finite, P > 0, d > 0 and wd = window * d < 0.5 * P
        members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff |tau| <= wd
        unit (a, b, c), a outermost, c innermost:
            T = d * ratios[a];  ho = 0.5 * T;  hb = ho * (1.0 - 2.0 * ingress[b]);  r = 1.0 / (ho - hb) where hb < ho
            c0 = d * shifts[c];  over the members in index order:  u = |tau - c0|
                s = 1.0 if u <= hb,  (ho - u) * r if u < ho,  else the member does not count
                cnt += 1;  N += xw * s;  D += w * (s * s)
            valid iff cnt >= min_count and D > 0 and depth = N / D > transit_depth_min;  ses = N / sqrt(D)
        best = the valid unit of the largest ses, the first in unit order on ties; box and vee = the same pick among the units
        of ingress[0] == 0.0 and of ingress[-1] == 0.5;  status 2 (n_points reported, the rest NaN) if no unit is valid

    Each step is one IEEE double operation and every sum runs in index order, so the result is bit-equal to the Python
    statement in tests/shape_fit_spec.py.  The trapezoid knows nothing of limb darkening or of the exposure time: both round
    the contacts, so `shape_ingress` of a planet is LARGER than its geometric T12/T14, and the geometry below inherits that.
    What separates the classes is the comparison: shape_ses_box^2 - shape_ses_vee^2 has the sign of the shape, and
    shape_delta_chi2 = ses^2 - ses_vee^2 is the chi^2 by which the best trapezoid beats the best V.

    The tables must be finite and ascending, ratios > 0, ingress from 0.0 to 0.5, at most 65536 units; window finite and at
    least 0.5 * max(ratios) + max|shifts| (the model must lie inside the window); min_count >= 1; transit_depth_min finite
    and >= 0; period, T0, duration and curve [n_fits] with curve in [0, n_curves): ValueError otherwise, before any device
    work (the detrending included).  detrend= takes the steps and tuples of search_batch.

    Returns a structured array [n_fits] with the fields shape_fit_fields(): shape_status (0 fitted; 1 no such candidate; 2 no
    valid unit), shape_n_points, shape_n_in, shape_ses, shape_depth, shape_depth_err, shape_duration (T14, days),
    shape_ingress (T12/T14), shape_shift (days), shape_i_duration, shape_i_ingress, shape_i_shift, shape_ses_box,
    shape_duration_box, shape_ses_vee, shape_duration_vee, shape_delta_chi2, and shape_impact, shape_a_rs, shape_rho_star:
    transit_geometry of the best trapezoid (NaN where it has none)."""
    from ._lib import shape_fit_candidates, shape_fit_tables
    ratio, ingress, shift, window, min_count, depth_min = shape_fit_tables(
        SHAPE_FIT_RATIOS if ratios is None else ratios, SHAPE_FIT_INGRESS if ingress is None else ingress,
        SHAPE_FIT_SHIFTS if shifts is None else shifts, window, min_count, transit_depth_min)
    t, flux_batch, dy_batch = _candidate_rows("shape fit", t, flux_batch, dy_batch)
    period, T0, duration, curve = shape_fit_candidates(period, T0, duration, curve, numpy.shape(flux_batch)[0])
    inp, y_rows, dy_rows, ctx = _candidate_inputs(t, flux_batch, dy_batch, detrend, context, device, power_kwargs)
    out = ctx.shape_fit(inp["t"], y_rows, dy_rows, period, T0, duration, ratio, ingress, shift, curve=curve, window=window,
                        min_count=min_count, depth_min=depth_min)
    return _with_shapes(None, out, period)


# ---- limb-darkened transit fit -------------------------------------------------------------------------------------------------
TRANSIT_FIT_K_ROWS = numpy.geomspace(0.01, 0.5, 81)
TRANSIT_FIT_IMPACTS = numpy.linspace(0.0, 0.96, 13)
TRANSIT_FIT_RATIOS = numpy.geomspace(0.7, 1.4, 29)
TRANSIT_FIT_SHIFTS = numpy.linspace(-0.1, 0.1, 9)


def transit_profile(k_rows=None, M=1024, **template_kwargs):
    """(k_rows, profile): the table tls_transit_fit reads its dips from.  Row j is the dip of a planet of k_rows[j] stellar
    radii over a star of the template's limb darkening -- u and limb_dark as power() takes them (transit_template="box"
    included), the other template keywords are not used -- at M + 1 separations from the centre to the contact:
    profile[j][m] = 1 - F((1 + k_rows[j]) m / M; k_rows[j]) and profile[j][M] = 0, F being transit_model.quadratic_ld_flux for
    the quadratic, linear and uniform laws and transit_model.numerical_ld_flux for the others.  Default rows:
    numpy.geomspace(0.01, 0.5, 81).  Formed on the host, so the device stage is the same for every law."""
    return _transit_profile("transit fit", k_rows, M, **template_kwargs)


def _transit_profile(what, k_rows=None, M=1024, **template_kwargs):
    """transit_profile, its messages headed `what`."""
    import warnings
    from . import transit_model, validate
    from ._lib import TRANSIT_FIT_MAX_M
    k_rows = numpy.array(TRANSIT_FIT_K_ROWS if k_rows is None else k_rows, dtype=numpy.float64)
    if k_rows.ndim != 1 or len(k_rows) < 1 or not numpy.all(numpy.isfinite(k_rows)) or not k_rows[0] > 0.0 \
            or not numpy.all(k_rows[1:] >= k_rows[:-1]):
        raise _checks.refusal(what, "k_rows must be a finite, ascending table of values > 0")
    M = _checks.integer(what, "M", M, 1, TRANSIT_FIT_MAX_M)

    class _Template(object):
        pass

    chosen = _Template()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        validate.validate_args(chosen, dict(template_kwargs, verbose=False))
    law = chosen.limb_dark
    u = [float(v) for v in numpy.atleast_1d(chosen.u)] if chosen.u is not None else []
    profile = numpy.zeros((len(k_rows), M + 1))
    grid = numpy.arange(M + 1) / float(M)
    for j, k in enumerate(k_rows.tolist()):
        z = (1.0 + k) * grid
        if law == "quadratic":
            flux = transit_model.quadratic_ld_flux(z, k, u[0], u[1])
        elif law == "linear":
            flux = transit_model.quadratic_ld_flux(z, k, u[0], 0.0)
        elif law == "uniform":
            flux = transit_model.quadratic_ld_flux(z, k, 0.0, 0.0)
        else:
            flux = transit_model.numerical_ld_flux(z, k, law, u)
        profile[j] = 1.0 - flux
        profile[j, M] = 0.0
    if not numpy.all(numpy.isfinite(profile)):
        raise _checks.refusal(what, "the profile of %r with u = %r is not finite" % (law, u))
    return k_rows, profile


def transit_fit_fields():
    """The fields of a transit fit, in order -- what transit_fit returns and power_batch(..., transit_fit=True) adds to the
    `peaks` array: the fields of tls_transit_fit_record, each behind the prefix fit_ (fit_status first), then the host-formed
    fit_T0 = T0 + fit_shift and the geometry of the fit (transit_fit_geometry): fit_a_rs, fit_inc, fit_rho_star."""
    from ._lib import TRANSIT_FIT_FIELDS
    return tuple("fit_" + k for k in TRANSIT_FIT_FIELDS) + ("fit_T0", "fit_a_rs", "fit_inc", "fit_rho_star")


def transit_fit_geometry(period, k, b, T14):
    """(a_rs, inc, rho_star) of a planet of k stellar radii crossing at impact parameter b in T14 days (first to last
    contact) on a circular orbit of `period` days, by the exact contact formula sin(pi T14 / P) = sqrt((1 + k)^2 - b^2) /
    (a_rs sin i) with b = a_rs cos i (Seager & Mallen-Ornelas 2003, equation 3):

        sT = sin^2(pi T14 / P);  a_rs = sqrt(b^2 + ((1 + k)^2 - b^2) / sT);  inc = arccos(b / a_rs) in degrees
        rho_star = 3 pi a_rs^3 / (G P^2), in units of the solar mean density

    Plain numpy on the host, broadcasting.  NaN where an input is not finite, (1 + k)^2 <= b^2, or T14 is not in (0, P / 2]."""
    from . import constants as C
    period, k, b, T14 = numpy.broadcast_arrays(*(numpy.asarray(v, dtype=numpy.float64) for v in (period, k, b, T14)))
    with numpy.errstate(all="ignore"):
        sT = numpy.sin(numpy.pi * T14 / period) ** 2
        chord2 = (1.0 + k) ** 2 - b * b
        a_rs = numpy.sqrt(b * b + chord2 / sT)
        inc = numpy.degrees(numpy.arccos(b / a_rs))
        rho_sun = C.M_sun / (4.0 / 3.0 * numpy.pi * float(C.R_sun) ** 3)
        rho = 3.0 * numpy.pi * a_rs ** 3 / (C.G * (period * C.SECONDS_PER_DAY) ** 2) / rho_sun
        good = numpy.isfinite(period) & numpy.isfinite(k) & numpy.isfinite(b) & numpy.isfinite(T14) & (chord2 > 0.0) \
            & (T14 > 0.0) & (T14 <= 0.5 * period) & (b >= 0.0) & numpy.isfinite(a_rs)
    return numpy.where(good, a_rs, numpy.nan), numpy.where(good, inc, numpy.nan), numpy.where(good, rho, numpy.nan)


def _transit_fit_setup(t, impacts, ratios, shifts, exposure, n_sub, window, min_count, delta, profile, template_kwargs,
                       what="transit fit"):
    """The checked tables of a transit fit: a dict with k_rows, profile, impact, ratio, shift, sub, window, min_count, delta.
    exposure None: the median cadence of t; 0: no smearing.  `what` heads the messages: remove_transits sets up the same."""
    from ._lib import TRANSIT_FIT_MAX_SUB, transit_fit_tables
    _checks.integer(what, "n_sub", n_sub, 1, TRANSIT_FIT_MAX_SUB)
    if exposure is None:
        t = numpy.asarray(t, dtype=numpy.float64)
        exposure = float(numpy.median(numpy.diff(t))) if t.ndim == 1 and len(t) > 1 else 0.0
    _checks.finite_at_least(what, "exposure", exposure, text="must be finite and >= 0 (days)")
    S = int(n_sub) if float(exposure) > 0.0 else 1
    sub = float(exposure) * ((2.0 * numpy.arange(S) + 1.0) / (2.0 * S) - 0.5) if S > 1 else numpy.zeros(1)
    if profile is None:
        profile = _transit_profile(what, **template_kwargs)
    try:
        k_rows, table = profile
    except (TypeError, ValueError):
        raise _checks.refusal(what, "profile must be the pair (k_rows, profile) of transit_profile")
    names = ("k_rows", "profile", "impact", "ratio", "shift", "sub", "window", "min_count", "delta")
    return dict(zip(names, transit_fit_tables(
        k_rows, table, TRANSIT_FIT_IMPACTS if impacts is None else impacts, TRANSIT_FIT_RATIOS if ratios is None else ratios,
        TRANSIT_FIT_SHIFTS if shifts is None else shifts, sub, window, min_count, delta, what)))


def _seed_rows(k_rows, depth):
    """The row of k_rows nearest sqrt(depth), the lowest on ties; row 0 where the depth is not a finite number >= 0."""
    depth = numpy.asarray(depth, dtype=numpy.float64)
    with numpy.errstate(all="ignore"):
        k0 = numpy.sqrt(numpy.where(numpy.isfinite(depth) & (depth >= 0.0), depth, 0.0))
    return numpy.argmin(numpy.fabs(k_rows[None, :] - k0.reshape(-1, 1)), axis=1).astype(numpy.int64).reshape(depth.shape)


def _with_transit_fits(records, fits, period, T0):
    """`records` (None, or the peaks with their fits) plus the device's transit-fit records, fit_T0 and the geometry."""
    out = _block(fits, transit_fit_fields())
    out["fit_T0"] = numpy.asarray(T0, dtype=numpy.float64) + fits["shift"]
    out["fit_a_rs"], out["fit_inc"], out["fit_rho_star"] = transit_fit_geometry(period, fits["k"], fits["b"], fits["duration"])
    return _joined(records, out)


def _transit_fit_request(transit_fit, peak_fits, t, power_kwargs):
    """None, or the checked tables (_transit_fit_setup) of a transit_fit=True / transit_fit=dict request -- the dict holds
    keywords of survey.transit_fit: impacts, ratios, shifts, exposure, n_sub, window, min_count, delta, profile (ValueError
    for a bad one, for an unknown key, and for transit_fit without peak_fits)."""
    if transit_fit is None or transit_fit is False:
        return None
    if not peak_fits:
        raise ValueError("transit_fit needs peak_fits=True: the fits start from T0 and duration of the fits")
    options = {} if transit_fit is True else transit_fit
    known = ("impacts", "ratios", "shifts", "exposure", "n_sub", "window", "min_count", "delta", "profile")
    if not isinstance(options, dict) or any(k not in known for k in options):
        raise ValueError("transit_fit must be True or a dict with keys among %s" % (known,))
    o = dict(dict(impacts=None, ratios=None, shifts=None, exposure=None, n_sub=5, window=1.0, min_count=3, delta=1.0,
                  profile=None), **options)
    template = {k: power_kwargs[k] for k in ("u", "limb_dark", "transit_template") if k in power_kwargs}
    return _transit_fit_setup(t, o["impacts"], o["ratios"], o["shifts"], o["exposure"], o["n_sub"], o["window"],
                              o["min_count"], o["delta"], o["profile"], template)


def _peak_transit_fits(ctx, inp, y_rows, dy_rows, peaks, fits, request):
    """The transit-fit records [n_curves, K] of the peaks of a slice of the batch, on ctx.  A peak whose duration is too
    short for the window to hold the widest, farthest shifted model plus half an exposure is no candidate either (the entry
    refuses such a candidate, and the durations are known only behind the search)."""
    reach = 0.5 * float(request["ratio"][-1]) + max(abs(float(request["shift"][0])), abs(float(request["shift"][-1])))
    with numpy.errstate(all="ignore"):
        d = fits["duration_days"].reshape(-1)
        holds = request["window"] * d >= reach * d + float(numpy.max(numpy.fabs(request["sub"])))
    period, T0, duration, curve, fitted = _peak_candidates(peaks, fits, holds)
    rows = _seed_rows(request["k_rows"], numpy.where(fitted, 1.0 - peaks["depth"].reshape(-1), numpy.nan))
    out = ctx.transit_fit(inp["t"], y_rows, dy_rows, period, T0, duration, rows, request["k_rows"], request["profile"],
                          request["impact"], request["ratio"], request["shift"], request["sub"], curve=curve,
                          window=request["window"], min_count=request["min_count"], delta=request["delta"])
    return out.reshape(fits.shape)


def transit_fit(t, flux_batch, period, T0, duration, depth, curve=None, dy_batch=None, impacts=None, ratios=None, shifts=None,
                exposure=None, n_sub=5, window=1.0, min_count=3, delta=1.0, profile=None, detrend=None, context=None,
                device=None, **template_kwargs):
    """The limb-darkened transit fit of candidates the caller holds, on the device (tls_transit_fit): candidate f is
    (period[f], T0[f], duration[f] in days, depth[f]) on light curve curve[f] of flux_batch [n_curves, n] (or one row [n])
    over the ascending time stamps t; curve=None takes one candidate a curve, in order.  It needs no search.  The search gives
    rp_rs from the depth alone, and the trapezoid of shape_fit knows nothing of limb darkening or of the exposure time.  Here
    the model is a planet of radius k crossing a limb-darkened star on a straight chord at constant speed, the separation
    z^2 = b^2 + ((1 + k)^2 - b^2) v^2 with v = (time from mid-transit) / (T14 / 2), averaged over n_sub sub-exposures of
    `exposure` days (None: the median cadence of t; 0: no smearing).  Its dip comes from a table the host forms once
    (transit_profile: any law power() takes, from u / limb_dark / transit_template in template_kwargs, or profile=(k_rows,
    profile)); the depth amplitude A is free and the baseline fixed at 1, as everywhere in TLS.  The grid is b / (1 + k) =
    impacts, T14 = duration * ratios and the centre T0 + duration * shifts (defaults: numpy.linspace(0, 0.96, 13),
    numpy.geomspace(0.7, 1.4, 29), numpy.linspace(-0.1, 0.1, 9): 3393 units), searched twice: with the profile row nearest
    sqrt(depth), then with the row nearest k of the first pass.  The row only shapes ingress and egress; the size is carried
    by A: k = k_rows[row] * sqrt(A).  The statement is in tests/transit_fit_spec.py and include/tls_amd.h, and the device
    equals it bit for bit.

    fit_k_lo .. fit_shift_hi are the least and the largest value over the units whose chi^2 lies within `delta` of the best:
    a profile-likelihood range, the honest answer where b, k and T14 are degenerate (at 30-minute cadence they are).  The
    straight chord differs from the circular orbit by about (pi T14 / P)^2 / 6 of the duration.

    The tables must be finite and ascending, impacts in [0, 1), ratios > 0, at most 65536 units; n_sub in [1, 16]; window
    finite, at least 0.5 * max(ratios) + max|shifts|, and for every candidate with a duration wide enough to hold the widest,
    farthest shifted model plus half an exposure; min_count >= 1; delta finite and >= 0; period, T0, duration, depth and
    curve [n_fits] with curve in [0, n_curves): ValueError otherwise, before any device work (the detrending included).
    detrend= takes the steps and tuples of search_batch.

    Returns a structured array [n_fits] with the fields transit_fit_fields(): fit_status (0 fitted; 1 no such candidate; 2 no
    valid unit), fit_n_points, fit_n_in, fit_row_first, fit_row, fit_ses, fit_amplitude, fit_k (rp / R*), fit_b,
    fit_duration (T14, days), fit_shift (days), fit_i_impact, fit_i_duration, fit_i_shift, fit_x2, the eight interval ends,
    fit_reserved, and fit_T0 = T0 + fit_shift, fit_a_rs, fit_inc (degrees), fit_rho_star (solar): transit_fit_geometry of the
    fit (NaN where it has none)."""
    from ._lib import shape_fit_candidates, transit_fit_window_holds
    setup = _transit_fit_setup(t, impacts, ratios, shifts, exposure, n_sub, window, min_count, delta, profile, template_kwargs)
    t, flux_batch, dy_batch = _candidate_rows("transit fit", t, flux_batch, dy_batch)
    period, T0, duration, curve = shape_fit_candidates(period, T0, duration, curve, numpy.shape(flux_batch)[0], "transit fit")
    try:
        depth = numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(depth, dtype=numpy.float64)))
    except (TypeError, ValueError) as e:
        raise ValueError(str(e))
    if depth.shape != period.shape:
        raise ValueError("transit fit: depth must hold one value a candidate")
    if not transit_fit_window_holds(duration, setup["ratio"], setup["shift"], setup["sub"], setup["window"]):
        raise ValueError("transit fit: window %r does not hold the widest, farthest shifted model plus half an exposure for "
                         "the shortest duration" % (setup["window"],))
    rows = _seed_rows(setup["k_rows"], depth)
    inp, y_rows, dy_rows, ctx = _candidate_inputs(t, flux_batch, dy_batch, detrend, context, device, template_kwargs)
    out = ctx.transit_fit(inp["t"], y_rows, dy_rows, period, T0, duration, rows, setup["k_rows"], setup["profile"],
                          setup["impact"], setup["ratio"], setup["shift"], setup["sub"], curve=curve, window=setup["window"],
                          min_count=setup["min_count"], delta=setup["delta"])
    return _with_transit_fits(None, out, period, T0)


# ---- centroid-shift test ------------------------------------------------------------------------------------------------------
def centroid_fields():
    """The fields of a centroid test, in order -- what centroid_test returns and power_batch(..., centroids=(cx, cy)) adds to
    the `peaks` array: the fields of tls_centroid_record, each behind the prefix cen_ (cen_status first), then what
    centroid_offsets forms of them on the host: cen_shift, cen_significance, cen_offset_x, cen_offset_y, cen_offset,
    cen_offset_err."""
    from ._lib import CENTROID_FIELDS
    return tuple("cen_" + k for k in CENTROID_FIELDS) + ("cen_shift", "cen_significance", "cen_offset_x", "cen_offset_y",
                                                         "cen_offset", "cen_offset_err")


def centroid_offsets(depth, depth_err, shift_x, shift_x_err, shift_y, shift_y_err):
    """(shift, significance, offset_x, offset_y, offset, offset_err) of a measured in-transit shift (sx +- ex, sy +- ey) of
    the photocentre and the depth D +- eD measured on the same points.  Plain numpy on the host, broadcasting.

        shift = sqrt(sx^2 + sy^2);  significance = sqrt((sx / ex)^2 + (sy / ey)^2)
        offset_x = -sx (1 - D) / D;  offset_y = -sy (1 - D) / D;  offset = shift (1 - D) / D
        offset_err^2 = ((1 - D) / D)^2 (sx^2 ex^2 + sy^2 ey^2) / shift^2 + (shift / D^2)^2 eD^2

    The photocentre of an aperture is the flux-weighted mean of its stars.  When a star at position r (relative to the
    out-of-transit photocentre) loses the share D of the aperture's flux, the photocentre moves by -r D / (1 - D): the offset
    is r, the position of the DIMMING source, in the unit of the centroids (pixels), and offset_err its error to first order
    in the errors of the shift and of the depth.  significance is, without a shift, a chi variable of 2 degrees of freedom:
    5 is exceeded by chance 4e-6 of the time.  All six are NaN where depth <= 0 or an input is NaN; offset_err also where the
    shift is exactly 0."""
    D, eD, sx, ex, sy, ey = numpy.broadcast_arrays(*(numpy.asarray(v, dtype=numpy.float64)
                                                     for v in (depth, depth_err, shift_x, shift_x_err, shift_y, shift_y_err)))
    with numpy.errstate(all="ignore"):
        good = D > 0.0
        shift = numpy.sqrt(sx * sx + sy * sy)
        significance = numpy.sqrt((sx / ex) ** 2 + (sy / ey) ** 2)
        lever = (1.0 - D) / D
        offset_x, offset_y, offset = -sx * lever, -sy * lever, shift * lever
        var_shift = (sx * sx * ex * ex + sy * sy * ey * ey) / (shift * shift)
        offset_err = numpy.sqrt(lever * lever * var_shift + (shift / (D * D)) ** 2 * eD * eD)
    return tuple(numpy.where(good, v, numpy.nan) for v in (shift, significance, offset_x, offset_y, offset, offset_err))


def _centroid_shape(inp):
    """The shape tls_centroid_test takes: 1 - the search's reference transit on CENTROID_SHAPE_SAMPLES samples (0 out of
    transit, 1 at the bottom)."""
    from ._lib import CENTROID_SHAPE_SAMPLES
    from .template import reference_transit
    return 1.0 - reference_transit(CENTROID_SHAPE_SAMPLES, **inp["shape"])


def _centroid_request(centroids, peak_fits, flux_shape, window, min_in, min_out):
    """None, or the checked request of centroids=(cx_batch, cy_batch): a dict with cx, cy (float64, of the flux's shape),
    window, min_in, min_out (ValueError for a bad one, and for centroids without peak_fits)."""
    if centroids is None:
        return None
    if not peak_fits:
        raise ValueError("centroids=(cx, cy) needs peak_fits=True: the test starts from T0 and duration of the fits")
    from ._lib import centroid_options, centroid_rows
    window, min_in, min_out, _ = centroid_options(window, min_in, min_out)
    try:
        cx, cy = centroids
    except (TypeError, ValueError):
        raise ValueError("centroids must be the pair (cx_batch, cy_batch)")
    if len(flux_shape) != 2:
        raise ValueError("flux_batch must have shape [n_curves, len(t)]")
    cx, cy = centroid_rows(cx, cy, flux_shape)
    return dict(cx=cx, cy=cy, window=window, min_in=min_in, min_out=min_out)


def _with_centroids(records, tests):
    """`records` (None, or the peaks with their fits) plus the device's centroid records and what centroid_offsets forms of
    them."""
    out = _block(tests, centroid_fields())
    (out["cen_shift"], out["cen_significance"], out["cen_offset_x"], out["cen_offset_y"], out["cen_offset"],
     out["cen_offset_err"]) = centroid_offsets(tests["depth"], tests["depth_err"], tests["shift_x"], tests["shift_x_err"],
                                               tests["shift_y"], tests["shift_y_err"])
    return _joined(records, out)


def _peak_centroid_tests(ctx, env, request):
    """centroid_tests [n_curves, K]: the centroid records of the peaks of a slice of the batch, on ctx, from the flux rows
    it searched and the centroid rows of the same curves."""
    from ._lib import CENTROID_MAX_EPOCHS
    period, T0, duration, curve, _ = _peak_candidates(env.peaks, env.fits)
    out = ctx.centroid_test(env.inp["t"], env.y_rows, request["cx"][env.rows], request["cy"][env.rows], period, T0, duration,
                            _centroid_shape(env.inp), curve=curve, window=request["window"], min_in=request["min_in"],
                            min_out=request["min_out"], max_epochs=min(env.max_epochs, CENTROID_MAX_EPOCHS))
    return dict(centroid_tests=out.reshape(env.fits.shape))


def centroid_epochs(t, period):
    """The max_epochs centroid_test takes by default: the most epochs a candidate of these periods can have on t, at most
    CENTROID_MAX_EPOCHS (periods that are not finite and > 0 have no epochs)."""
    from ._lib import CENTROID_MAX_EPOCHS
    t, period = numpy.asarray(t, dtype=numpy.float64), numpy.asarray(period, dtype=numpy.float64)
    real = period[numpy.isfinite(period) & (period > 0.0)]
    if len(t) == 0 or len(real) == 0:
        return 1
    with numpy.errstate(all="ignore"):
        most = numpy.ceil((t[-1] - t[0]) / numpy.min(real)) + 2.0
    return int(min(max(most, 1.0), CENTROID_MAX_EPOCHS))


def centroid_test(t, flux_batch, cx_batch, cy_batch, period, T0, duration, curve=None, window=3.0, min_in=1, min_out=3,
                  max_epochs=None, detrend=None, context=None, device=None, **power_kwargs):
    """WHICH star dims: the in-transit shift of the flux-weighted photocentre of candidates the caller holds, on the device
    (tls_centroid_test).  Candidate f is (period[f], T0[f], duration[f] in days) on light curve curve[f] of flux_batch
    [n_curves, n] (or one row [n]) over the ascending time stamps t; curve=None takes one candidate a curve, in order.
    cx_batch and cy_batch, of flux_batch's shape, are the column and row centroids of the aperture on the same cadences
    (MOM_CENTR1, MOM_CENTR2 of a Kepler, K2 or TESS light-curve file), in any unit; a cadence whose centroid is NaN or
    infinite is skipped.  It needs no search.  A background eclipsing binary a few pixels from the target, diluted to a
    planet-like depth, passes every test of the flux alone; the photocentre gives it away.

    The search's limb-darkened template (power_kwargs: the keywords of power()) at the candidate's ephemeris, s = 1 at the
    bottom and 0 out of transit, is regressed on three series -- the flux deficit 1 - y, cx and cy -- over the points within
    window * duration of every transit, with a free constant in every epoch, because centroids drift with the pointing:

        status 1 and NaN in every other field unless P, T0, d finite, P > 0, d > 0 and wd = window * d < 0.5 * P
        points, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P
            member iff |tau| <= wd and cx[i], cy[i] both finite;  its epoch is k;  inside iff |tau| <= d / 2
        an epoch is used iff it has min_in members inside and min_out outside;  status 2 without a used epoch, or with more
            epochs than max_epochs (default: the most the shortest period can have on t, at most 65536)
        in every used epoch the means of s and of the three series are taken off;  D = sum ds^2,  N = sum ds dc,  Q = sum dc^2
        amplitude A = N / D;  var = (Q - A N) / (n_points - n_epochs - 1);  err = sqrt(var / D);  rms = sqrt(var)
        chi2 = sum over the used epochs of (A_epoch - A)^2 D_epoch / var:  n_epochs - 1 degrees of freedom

    tests/centroid_spec.py states every step, and the result is bit-equal to it.  A linear drift across a window is orthogonal
    to the symmetric template, so the constant is enough for a slow pointing drift; what it leaves inflates rms, not the
    shift.  The flux is detrended where detrend= asks for it (the steps and tuples of search_batch); the centroids never are.

    How to read it.  cen_shift_x, cen_shift_y are the motion of the photocentre in transit and cen_significance its
    distance from zero in sigmas.  An isolated target gives no shift and an offset of 0: the dimming star is at the
    photocentre.  In a crowded aperture the photocentre is not on the target, so even a true planet gives a shift: what
    counts is cen_offset_x, cen_offset_y -- the position of the dimming source relative to the out-of-transit photocentre
    (centroid_offsets) -- held against the target's catalogue position relative to that photocentre, not the shift against
    zero.  A cen_chi2_x or cen_chi2_y far above cen_n_epochs - 1 says single events carry the shift: a systematic, not a
    source.  cen_depth is the depth measured in the same way on the same points.

    window must be finite and >= 1, min_in and min_out integers >= 1, max_epochs in [1, 65536]; cx_batch and cy_batch of
    flux_batch's shape; period, T0, duration and curve [n_fits] with curve in [0, n_curves): ValueError otherwise, before
    any device work (the detrending included).

    Returns a structured array [n_fits] with the fields centroid_fields(): cen_status (0 measured; 1 no such candidate; 2
    no usable epoch, or too many), cen_n_epochs, cen_n_skipped, cen_n_points, cen_n_in, cen_depth, cen_depth_err,
    cen_shift_x, cen_shift_x_err, cen_shift_y, cen_shift_y_err, cen_rms_x, cen_rms_y, cen_chi2_depth, cen_chi2_x,
    cen_chi2_y, and cen_shift, cen_significance, cen_offset_x, cen_offset_y, cen_offset, cen_offset_err (NaN where
    cen_depth is not > 0)."""
    from ._lib import centroid_options, centroid_rows, shape_fit_candidates
    t, flux_batch, _ = _candidate_rows("centroid test", t, flux_batch)
    cx_rows, cy_rows = centroid_rows(cx_batch, cy_batch, numpy.shape(flux_batch))
    period, T0, duration, curve = shape_fit_candidates(period, T0, duration, curve, numpy.shape(flux_batch)[0], "centroid test")
    window, min_in, min_out, max_epochs = centroid_options(window, min_in, min_out,
                                                           centroid_epochs(t, period) if max_epochs is None else max_epochs)
    inp, y_rows, _, ctx = _candidate_inputs(t, flux_batch, None, detrend, context, device, power_kwargs)
    out = ctx.centroid_test(inp["t"], y_rows, cx_rows, cy_rows, period, T0, duration, _centroid_shape(inp), curve=curve,
                            window=window, min_in=min_in, min_out=min_out, max_epochs=max_epochs)
    return _with_centroids(None, out)


# ---- folded, median-binned views ------------------------------------------------------------------------------------------------
def folded_view_fields():
    """The fields of a folded-views record, in order (tls_views_record): status (0 binned; 1 no such candidate),
    secondary_status (0 binned; 1 no secondary view), and n_global, n_local, n_local_even, n_local_odd, n_secondary -- the
    points that are a member of at least one bin of the view.  power_batch(..., views=True) adds views_status and the five
    counts as views_n_global ... views_n_secondary to the `peaks` array."""
    from ._lib import VIEWS_FIELDS
    return tuple(VIEWS_FIELDS)


def _views_dict(g_med, g_cnt, l_med, l_cnt, lead):
    """The dict of view arrays from the device's four arrays, their candidate axis reshaped to `lead`."""
    from ._lib import VIEWS_LOCAL
    views = {"global": g_med.reshape(lead + g_med.shape[1:]), "global_count": g_cnt.reshape(lead + g_cnt.shape[1:])}
    for i, name in enumerate(VIEWS_LOCAL):
        views[name] = l_med[:, i].reshape(lead + l_med.shape[2:])
        views[name + "_count"] = l_cnt[:, i].reshape(lead + l_cnt.shape[2:])
    return views


def folded_views(t, flux_batch, period, T0, duration, curve=None, secondary_phase=None, n_global=2001, n_local=201,
                 local_durations=4.0, local_width=0.16, context=None, device=None):
    """The phase-folded, median-binned views of candidates the caller holds, on the device (tls_folded_views): candidate f
    is (period[f], T0[f], duration[f] in days) on light curve curve[f] of flux_batch [n_curves, n] (or one row [n]) over the
    ascending time stamps t; curve=None takes one candidate a curve, in order.  It needs no search.  These are the "global
    view" and "local view" of Shallue & Vanderburg (2018) and the even, odd and secondary-eclipse local views of
    Valizadegan et al. (2022) -- the panels of a data-validation report, the input of a neural-net vetter.  A view is
    (phi_c, x_min, x_max, w, B, parity):

        x = (t[i] - T0) / P;  u = x - phi_c;  e = floor(u + 0.5);  tau = (u - e) * P         (days from the view's centre)
        bin b:  s = ((x_max - x_min) - w) / (B - 1);  lo = b * s + x_min;  member iff lo <= tau and tau < lo + w
                (with a parity also e - 2 * floor(e / 2) == parity)
        count[b] = the members;  median[b] = the middle member by value, (a + b) / 2 of the two middle ones, NaN of none

        global      phi_c 0      -0.5 P .. 0.5 P                          w = P / n_global         n_global bins
        local       phi_c 0      -local_durations d .. local_durations d  w = local_width d        n_local bins
        local_even, local_odd    the local view of the epochs e of parity 0 and 1: with the fit's own T0 -- its first
                                 transit -- even is the first, third, ... transit, power()'s transit_depths[::2]
        secondary   the local view about phi_c = secondary_phase[f] (phase_scan's secondary_phase); NaN / 0 where that is
                    not finite, and everywhere with secondary_phase=None

    Each step is one IEEE double operation and a median is a selection, so records and arrays are bit-equal to the Python
    statement in tests/folded_views_spec.py.  The medians are unweighted.  The defaults are Astronet's.  n_global and n_local
    in [2, 65536], local_durations and local_width finite and > 0, local_width <= 2 * local_durations, curve in
    [0, n_curves), t finite and ascending, flux finite: ValueError otherwise, before any device work.

    Returns (records, views): a structured array [n_fits] with the fields folded_view_fields(), and a dict of arrays
    [n_fits, bins]: global, local, local_even, local_odd, secondary (float64 medians) and the same names + "_count" (int32).
    A candidate without an ephemeris (status 1) has NaN and 0 everywhere.  normalize_views scales them for a vetter."""
    from ._lib import folded_views_arguments
    a = folded_views_arguments(t, flux_batch, period, T0, duration, curve, secondary_phase, n_global, n_local,
                               local_durations, local_width)
    ctx = context if context is not None else _search.default_context(device)
    out = ctx.folded_views(a["t"], a["y"], a["period"], a["T0"], a["duration"], curve=a["curve"],
                           secondary_phase=a["secondary_phase"], n_global=a["n_global"], n_local=a["n_local"],
                           local_durations=a["local_durations"], local_width=a["local_width"])
    return out[0], _views_dict(*out[1:], lead=(len(out[0]),))


def normalize_views(views):
    """The views as a vetter takes them (host numpy; the Astronet convention, stated in tests/folded_views_spec.py): in every
    row of every array of medians the empty bins (NaN) are filled by linear interpolation between the neighbouring non-empty
    ones, the edges held; the row's median is subtracted; the row is divided by the absolute value of its minimum, so the
    deepest bin is -1.  A row whose minimum is 0 is left undivided, a row without a non-empty bin stays NaN.  The "_count"
    arrays are copied as they are.  Returns a new dict."""
    out = {}
    for name, v in views.items():
        if name.endswith("_count"):
            out[name] = numpy.array(v)
            continue
        v = numpy.array(v, dtype=numpy.float64)
        rows = v.reshape(-1, v.shape[-1]) if v.ndim else v.reshape(1, 1)
        where = numpy.arange(rows.shape[1], dtype=numpy.float64)
        for row in rows:
            full = ~numpy.isnan(row)
            if not full.any():
                continue
            filled = numpy.interp(where, where[full], row[full])
            filled = filled - numpy.median(filled)
            low = filled.min()
            row[:] = filled if low == 0.0 else filled / abs(low)
        out[name] = v
    return out


def _views_request(views, peak_fits, n_global, n_local, local_durations, local_width):
    """None, or the checked (n_global, n_local, local_durations, local_width) of a views=True request (ValueError for a bad
    one, and for views without peak_fits)."""
    if not views:
        return None
    if not peak_fits:
        raise ValueError("views=True needs peak_fits=True: the views fold at T0 and bin by duration_days of the fits")
    from ._lib import folded_views_tables
    return folded_views_tables(n_global, n_local, local_durations, local_width)


def _peak_views(ctx, env, request):
    """The views of the peaks of a slice of the batch, on ctx: views_records [n_curves, K] and the four arrays of the
    device, [n_curves, K, ...].  Without phase scans there is no secondary view."""
    n_global, n_local, k, width = request
    period, T0, duration, curve, fitted = _peak_candidates(env.peaks, env.fits)
    phi = None if env.scans is None else numpy.where(fitted, env.scans["secondary_phase"].reshape(-1), numpy.nan)
    out = ctx.folded_views(env.inp["t"], env.y_rows, period, T0, duration, curve=curve, secondary_phase=phi,
                           n_global=n_global, n_local=n_local, local_durations=k, local_width=width)
    names = ("views_records", "views_global", "views_global_count", "views_local", "views_local_count")
    return {name: v.reshape(env.fits.shape + v.shape[1:]) for name, v in zip(names, out)}


def _peak_views_dict(out, request):
    """The `views` entry of the peaks dict from the joined arrays of _peak_views."""
    flat = (out[k].reshape((-1,) + out[k].shape[2:]) for k in ("views_global", "views_global_count", "views_local",
                                                               "views_local_count"))
    return dict(views=_views_dict(*flat, lead=out["views_records"].shape))


def _with_views(records, views):
    """The peaks plus views_status and the five views_n_* member counts of the device's view records."""
    fields = folded_view_fields()
    return _joined(records, _block(views, ["views_status"] + ["views_" + k for k in fields[2:]], ("status",) + fields[2:]))


# ---- variability periodogram and sine test -----------------------------------------------------------------------------------
def variability_frequencies(t, oversampling=5, f_max=None):
    """The default frequency grid of lomb_scargle: k / (oversampling * T) for k = 1, 2, ... up to f_max (cycles a day), with
    T = t[-1] - t[0]; f_max None: 0.5 / median(diff(t)), the Nyquist frequency of the median cadence.  ValueError for a t
    that is not 1-D, finite and ascending with T > 0, an oversampling that is not finite and > 0, and an f_max that is not
    finite and at least 1 / (oversampling * T)."""
    try:
        t = numpy.asarray(t, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise ValueError("periodogram: t must hold numbers")
    if t.ndim != 1 or len(t) < 2 or not numpy.all(numpy.isfinite(t)) or not numpy.all(t[1:] >= t[:-1]) or not t[-1] > t[0]:
        raise ValueError("periodogram: t must be [n], finite and ascending over a span > 0")
    if isinstance(oversampling, bool) or not isinstance(oversampling, numbers.Real) or not (0.0 < float(oversampling) < numpy.inf):
        raise ValueError("periodogram: oversampling must be finite and > 0, got %r" % (oversampling,))
    step = 1.0 / (float(oversampling) * float(t[-1] - t[0]))
    if f_max is None:
        f_max = 0.5 / float(numpy.median(numpy.diff(t)))
    if isinstance(f_max, bool) or not isinstance(f_max, numbers.Real) or not (step <= float(f_max) < numpy.inf):
        raise ValueError("periodogram: f_max must be finite and at least 1 / (oversampling * T) = %r, got %r" % (step, f_max))
    count = int(numpy.floor(float(f_max) / step))
    return numpy.arange(1, count + 1) * step


def lomb_scargle(t, flux_batch, frequencies=None, dy_batch=None, peaks=None, with_arrays=True, detrend=None, context=None,
                 device=None, devices=None, peak_separation=0.02, detrend_mask=None):
    """The generalised (floating-mean, weighted) Lomb-Scargle periodogram of Zechmeister & Kuerster (2009) of every light
    curve of flux_batch [n_curves, n] (or one row [n]) on the shared ascending time stamps t, on the device
    (tls_lomb_scargle): is the STAR periodic -- spots, pulsations, a contact binary -- and at which period?  frequencies
    (cycles a day, any order, None: variability_frequencies(t)); dy_batch: per-point errors (None: uniform weights).

        prologue, every sum in index order:
            w_i = 1 / dy_i^2, normalised to sum w = 1 (1 / n without dy_batch);  ybar = sum w_i y_i
            a_i = w_i (y_i - ybar);  YY = sum a_i (y_i - ybar)
        phi_ki = 2 pi frac(f_k (t_i - t_0)), the phase reduced in cycles before it is scaled
        YC, YS = sum a_i cos phi, sum a_i sin phi;  C, S the same of w;  C2, S2 the same of w at 2 f
        CC = 0.5 (1 + C2) - C C;  SS = 0.5 (1 - C2) - S S;  CS = 0.5 S2 - C S;  D = CC SS - CS CS
        power = (SS YC YC + CC YS YS - 2 CS YC YS) / (YY D)         (the fraction of the variance a sinusoid removes)
        ca = (YC SS - YS CS) / D;  sa = (YS CC - YC CS) / D;  amplitude = sqrt(ca^2 + sa^2);  phase = atan2(sa, ca) / (2 pi)
        NaN where D <= 0 or YY <= 0 (a constant curve; a frequency at which every point has one phase)

    The sums are one dense product -- the rows times a [n x 2 F] matrix of cos / sin that is generated on the fly and never
    stored -- in fp64 FMAs; they lie within (n + 2 pi max|f (t - t_0)| + 8) 2^-52 sum|a| of the exact sums.  The prologue
    equals the Python statement in tests/gls_spec.py bit for bit, and power and amplitude equal its epilogue applied to the
    device's own sums bit for bit.  phase is the DEVICE's atan2: it agrees with numpy's within a few ulp, not bit for bit.

    peaks=K also selects the K highest peaks of every curve on the device, from the power where it lies, by the selection of
    find_peaks with periods = 1 / frequencies, separation peak_separation and the ratios (0.5, 2.0); with_arrays=False then
    brings back the peaks alone.  detrend= takes the steps and tuples of search_batch and detrend_mask= its mask (for the
    Biweight and Prewhiten steps; SysRem runs unmasked; a median-filter step with a mask is a ValueError; the periodogram
    itself uses every point), devices=[...] deals the curves out over several GPUs.  ValueError, before any device work (the detrending included), for non-finite input, a t that is not
    ascending, frequencies that are not finite and > 0, n < 3 and shapes that disagree.

    Returns a dict: frequencies [F], mean (ybar) and variance (YY) [n_curves]; power, amplitude, phase [n_curves, F] with
    with_arrays; peaks (period, power, index; [n_curves, K]) and n_peaks with peaks=K.  One row gives [F] and [K]."""
    from ._lib import lomb_scargle_arguments
    if frequencies is None:
        frequencies = variability_frequencies(t)
    one = numpy.ndim(flux_batch) == 1
    if numpy.ndim(flux_batch) == 2:                  # (a Clean at the head of detrend repairs the rows before they are checked)
        flux_batch, detrend = _clean_first(t, flux_batch, detrend, context, device, devices)
    a = lomb_scargle_arguments(t, flux_batch, dy_batch, frequencies, peaks, peak_separation)
    rows = _detrended(a["t"], a["y"], detrend, context, device, devices, a["dy"], detrend_mask)

    def call(ctx, lo, hi):
        return ctx.lomb_scargle(a["t"], rows[lo:hi], a["frequencies"], None if a["dy"] is None else a["dy"][lo:hi], peaks=peaks,
                                separation=a["separation"], with_arrays=with_arrays)

    out = dict(_run_batch(devices, device, context, len(a["y"]), call))
    if one:
        out = {k: v[0] for k, v in out.items()}
    out["frequencies"] = a["frequencies"]
    return out


def sine_test_fields(harmonics=(0.5, 1.0, 2.0)):
    """The fields of a sine test, in order -- what sine_test returns and power_batch(..., sine_test=True) adds to the `peaks`
    array: sine_status (0 done; 1 no such candidate; 2 fewer than 4 points left), sine_n_used, sine_mean, sine_variance, then
    sine_power, sine_amplitude, sine_phase, sine_amplitude_err and sine_significance, each [n_harmonics]."""
    from ._lib import SINE_FIELDS, SINE_HARMONIC_FIELDS
    return tuple("sine_" + k for k in SINE_FIELDS + SINE_HARMONIC_FIELDS)


def _sine_test_request(sine_test, peak_fits, mask, harmonics):
    """None, or the checked (mask, harmonics) of a sine_test=True request (ValueError for a bad one, and for sine_test
    without peak_fits)."""
    if not sine_test:
        return None
    if not peak_fits:
        raise ValueError("sine_test=True needs peak_fits=True: the transits of the fits are masked out")
    from ._lib import sine_test_arguments
    a = sine_test_arguments([0.0], [1.0], None, [1.0], None, None, None, mask, harmonics)
    return a["mask"], a["harmonics"]


def _with_sines(records, sines, harmonics):
    """`records` (None, or the peaks with their fits) plus the device's sine records and harmonic records."""
    from ._lib import SINE_FIELDS, SINE_HARMONIC_FIELDS
    nH = harmonics.shape[-1]
    out = numpy.zeros(sines.shape, dtype=[("sine_" + k, "f8") for k in SINE_FIELDS]
                      + [("sine_" + k, "f8", (nH,)) for k in SINE_HARMONIC_FIELDS])
    for k in SINE_FIELDS:
        out["sine_" + k] = sines[k]
    for k in SINE_HARMONIC_FIELDS:
        out["sine_" + k] = harmonics[k]
    return _joined(records, out)


def _peak_sine_tests(ctx, env, request):
    """sine_tests [n_curves, K] and sine_harmonics [n_curves, K, n_harmonics] of the peaks of a slice of the batch, on ctx.
    The weights are normalised, so the search's dy / mean(dy) serve; without a dy_batch they are uniform."""
    mask, harmonics = request
    period, T0, duration, curve, _ = _peak_candidates(env.peaks, env.fits)
    out, out_h = ctx.sine_test(env.inp["t"], env.y_rows, period, curve=curve, dy=env.dy_rows if env.weighted else None, T0=T0,
                               duration=duration, mask=mask, harmonics=harmonics)
    return dict(sine_tests=out.reshape(env.fits.shape), sine_harmonics=out_h.reshape(env.fits.shape + (len(harmonics),)))


def sine_test(t, flux_batch, period, curve=None, dy_batch=None, T0=None, duration=None, mask=1.5, harmonics=(0.5, 1.0, 2.0),
              detrend=None, context=None, device=None):
    """Is a candidate the star's own variability?  The per-candidate counterpart of lomb_scargle, after the SWEET test of the
    Kepler Robovetter, on the device (tls_sine_test): candidate f is period[f] (days) on light curve curve[f] of flux_batch
    [n_curves, n] (or one row [n]) over the ascending time stamps t; curve=None takes one candidate a curve, in order.  A
    contact binary or an ellipsoidal variable is a sinusoid at P or P / 2, a spotted star at P or 2 P; the odd-even test, the
    phase scan and the shape fit all see such a curve as a wide, shallow dip.  With T0 and duration [n_fits] the points within
    0.5 * mask * duration of a transit leave the fit (folded as shape_fit folds them), so the sinusoid is measured on the
    out-of-transit baseline.

        status 1 (NaN elsewhere) unless P finite and > 0 and, with T0 / duration, T0 finite and duration finite and > 0
        x = (t_i - T0) / P;  k = floor(x + 0.5);  tau = (x - k) P;  point i is out iff |tau| <= 0.5 mask duration
        n_used = the points left;  status 2 if n_used < 4
        the prologue of lomb_scargle over the points left (1 / n_used without dy_batch), every sum an ordered sum: lane
        j = i mod 256 adds its terms over i ascending (0.0 for a point that is out), the lanes are added in lane order
        for every harmonic h: the six sums at f = 1 / (h P) and 2 f, ordered sums of rounded products, and the epilogue
        amplitude_err = sqrt(2 YY (1 - power) / (n_used - 3));  significance = amplitude / amplitude_err

    n_used, mean and variance equal the Python statement in tests/gls_spec.py bit for bit, the sums lie within the bound
    lomb_scargle states, and the harmonic records equal the statement's epilogue applied to the device's own sums bit for
    bit but for phase (the device's atan2).  There is no threshold here: on the statement's 1800-point curve (noise 3e-4,
    seeds 0 to 4) a planet of rp 0.07 has a largest significance of 1.2 to 2.5, a contact-binary sinusoid of the same depth
    233 to 246 (tests/test_gls_host.py reports both).  mask finite and >= 0; 1 to 8 harmonics, finite and > 0; T0 and duration come
    together; curve in [0, n_curves): ValueError otherwise, before any device work (the detrending included).  detrend=
    takes the steps and tuples of search_batch.

    Returns a structured array [n_fits] with the fields sine_test_fields(): sine_status, sine_n_used, sine_mean,
    sine_variance, and sine_power, sine_amplitude, sine_phase, sine_amplitude_err, sine_significance [n_harmonics]."""
    from ._lib import sine_test_arguments
    a = sine_test_arguments(t, flux_batch, dy_batch, period, T0, duration, curve, mask, harmonics)
    rows = _detrended(a["t"], a["y"], detrend, context, device, None, a["dy"])
    ctx = context if context is not None else _search.default_context(device)
    out, out_h = ctx.sine_test(a["t"], rows, a["period"], curve=a["curve"], dy=a["dy"], T0=a["T0"], duration=a["duration"],
                               mask=a["mask"], harmonics=a["harmonics"])
    return _with_sines(None, out, out_h)


# ---- the ephemeris match: the test across the stars of a batch -----------------------------------------------------------------
def ephemeris_match_fields():
    """The fields of an ephemeris match, in order -- what ephemeris_match returns (tls_match_record): status, n_same,
    n_period, n_match, best, best_ratio, best_dt, best_drift, best_strength, child."""
    from ._lib import MATCH_FIELDS
    return tuple(MATCH_FIELDS)


def ephemeris_match_peak_fields():
    """The fields power_batch(..., ephemeris_match=True) adds to the `peaks` array, in order: those of
    ephemeris_match_fields() under the prefix match_, with `best` as the pair (match_curve, match_rank), both int64."""
    return ("match_status", "match_n_same", "match_n_period", "match_n_match", "match_curve", "match_rank", "match_ratio",
            "match_dt", "match_drift", "match_strength", "match_child")


def _ephemeris_match_request(ephemeris_match, peak_fits, drift, epoch, max_ratio):
    """None, or the checked (drift_tolerance, epoch_tolerance, max_ratio) of an ephemeris_match=True request (ValueError for
    a bad one, and for ephemeris_match without peak_fits)."""
    if not ephemeris_match:
        return None
    if not peak_fits:
        raise ValueError("ephemeris_match=True needs peak_fits=True: the match reads T0 and duration of the fits")
    from ._lib import ephemeris_match_arguments
    a = ephemeris_match_arguments([], [], [], [], [], 1.0, drift, epoch, max_ratio)
    return a["drift_tolerance"], a["epoch_tolerance"], a["max_ratio"]


def _peak_matches(ctx, env, request):
    """matches: the match records of the fitted peaks of the whole batch, on ctx, as (records MATCH_DTYPE [M], the
    candidates' flat indices c K + r into [n_curves, K], the shape).  A candidate is a peak of fit status 0: star = its
    curve, its period, T0 and duration_days of its fit, strength = 1 - depth; span = max t - min t."""
    drift, epoch, max_ratio = request
    peaks, fits, t = env.peaks, env.fits, env.inp["t"]
    k = fits.shape[1]
    at = numpy.flatnonzero((fits["status"] == 0).reshape(-1))
    records = ctx.ephemeris_match(at // k, peaks["period"].reshape(-1)[at], fits["T0"].reshape(-1)[at],
                                  fits["duration_days"].reshape(-1)[at], 1 - peaks["depth"].reshape(-1)[at],
                                  numpy.max(t) - numpy.min(t), drift, epoch, max_ratio)
    return dict(matches=(records, at, fits.shape))


def _with_matches(records, matches):
    """`records` (the peaks with their fits) plus the match records of the fitted ones (_peak_matches): match_status 1, -1 in
    match_curve and match_rank and NaN in the others where nothing was fitted."""
    from ._lib import MATCH_FIELDS
    found, at, shape = matches
    k = shape[1]
    names = ephemeris_match_peak_fields()
    out = numpy.zeros(shape, dtype=[(n, "i8" if n in ("match_curve", "match_rank") else "f8") for n in names])
    flat = out.reshape(-1)
    for n in names:
        flat[n] = -1 if n in ("match_curve", "match_rank") else numpy.nan
    flat["match_status"] = 1
    for n, source in zip(names[:4] + names[6:], MATCH_FIELDS[:4] + MATCH_FIELDS[5:]):
        flat[n][at] = found[source]
    best = found["best"].astype(numpy.int64)
    there = best >= 0
    target = at[numpy.where(there, best, 0)]
    flat["match_curve"][at] = numpy.where(there, target // k, -1)
    flat["match_rank"][at] = numpy.where(there, target % k, -1)
    return _joined(records, out)


def ephemeris_match(star, period, T0, duration, strength, span, drift_tolerance=0.5, epoch_tolerance=0.5, max_ratio=3,
                    context=None, device=None):
    """The ephemeris match of the Kepler and TESS false-positive catalogues (Coughlin et al. 2014), on the device
    (tls_ephemeris_match): which candidates on DIFFERENT stars share a period (or an integer multiple of it) and an epoch?
    The stars of one field contaminate one another: a faint star next to an eclipsing binary shows the binary's ephemeris at
    a diluted depth and passes every single-curve test, because the signal in its light curve is real.  The strongest member
    of such a group is taken as the source.  A period that many stars show with no common epoch is a systematic: n_same
    counts it.  Candidate f is (star[f], any integer: candidates of one star are never matched, so `star` may name groups of
    the caller's own; period[f], T0[f], duration[f] in days; strength[f], larger = more likely the source, e.g. the depth);
    span is the length of the observations in days.  All pairs are tested, up to 2^20 candidates.

        good[f] = period, T0, duration, strength finite, period > 0, duration > 0;  a bad f: status 1, NaN elsewhere, and
        invisible to the others.  For a good f and every good g != f with star[g] != star[f], (l, s) = the member of the
        longer / the shorter period:
        m = rint(P_l / P_s);  e = m * P_s;  dP = fabs(P_l - e);  c = span / P_l;  drift = dP * c
        dmax = fmax(d_f, d_g);  plim = drift_tolerance * dmax;  elim = epoch_tolerance * dmax
        period_match = (m <= max_ratio) and (drift <= plim)
        x = (T0_l - T0_s) / P_s;  r = rint(x);  u = x - r;  dt = fabs(u) * P_s;  match = period_match and (dt <= elim)

    drift is how far the two ephemerides slide apart over the span, dt the distance of the epochs modulo the shorter period;
    both are held against the longer of the two durations.  Every step is one IEEE double operation, the counts and the
    argmax do not depend on the order of evaluation and no doubles are summed, so the result is bit-equal to the numpy
    statement in tests/ephemeris_match_spec.py.  span finite and > 0, both tolerances finite and >= 0, max_ratio an integer in
    [1, 64]; ValueError otherwise, before any device work.

    Returns a structured array [M] with the fields ephemeris_match_fields(), all doubles: status (0; 1 a bad candidate),
    n_same (the g with period_match and m == 1: the pile-up count), n_period (the g with period_match), n_match (the g with
    match), best (the index of the match of the largest strength, the lowest index among equals; -1 without one), best_ratio
    (+m if P_best >= P_f, else -m), best_dt, best_drift, best_strength, and child (1 if strength[best] > strength[f], else 0);
    the last five NaN without a match.  ephemeris_groups names every candidate's source."""
    from ._lib import ephemeris_match_arguments
    a = ephemeris_match_arguments(star, period, T0, duration, strength, span, drift_tolerance, epoch_tolerance, max_ratio)
    ctx = context if context is not None else _search.default_context(device)
    return ctx.ephemeris_match(**a)


def ephemeris_groups(records):
    """The root of every candidate of ephemeris_match's records [M]: follow `best` while child == 1 -- strength rises
    strictly along the chain, so it ends -- and report where it ends; a candidate without a stronger match is its own root.
    int64 [M].  Host only."""
    records = numpy.asarray(records)
    best = records["best"]
    child = records["child"] == 1
    root = numpy.arange(len(records), dtype=numpy.int64)
    for f in range(len(records)):
        at = f
        while child[at]:
            at = int(best[at])
        root[f] = at
    return root


# ---- the per-star noise profile ------------------------------------------------------------------------------------------------
# the 14 pulse durations (hours) of Kepler's rms CDPP table
KEPLER_PULSE_HOURS = (1.5, 2.0, 2.5, 3.0, 3.5, 4.5, 5.0, 6.0, 7.5, 9.0, 10.5, 12.0, 12.5, 15.0)
NOISE_CLIP = 5.0
NOISE_GAP_TOLERANCE = 0.5
NOISE_MIN_COUNT = 3


def noise_curve_fields():
    """The fields of the per-curve record of a noise profile, in order: status (0 measured; 1 sigma == 0: a constant row, or
    more than half of it on one value), n_clipped, n_pairs, median, sigma (1.4826 * MAD) and sigma_p2p (the point-to-point
    sigma of the kept neighbours)."""
    from ._lib import NOISE_CURVE_FIELDS
    return NOISE_CURVE_FIELDS


def _noise_cadence(t, what="noise profile"):
    """(t as float64, numpy.median(numpy.diff(t))): ValueError unless t is [n >= 3], finite and ascending with a cadence > 0."""
    try:
        t = numpy.asarray(t, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: t must hold numbers" % what)
    if t.ndim != 1 or len(t) < 3 or not numpy.all(numpy.isfinite(t)) or not numpy.all(t[1:] >= t[:-1]):
        raise ValueError("%s: t must be [n] with n >= 3, finite and ascending" % what)
    cadence = numpy.median(numpy.diff(t))
    if not 0.0 < cadence < numpy.inf:
        raise ValueError("%s: the median cadence of t must be finite and > 0, got %r" % (what, cadence))
    return t, cadence


def noise_widths(t, hours=KEPLER_PULSE_HOURS):
    """The default window widths (samples) of noise_profile on the time stamps t: max(1, round(h / 24 / cadence)) for every h
    of `hours` (by default the 14 Kepler pulse durations) and 1, unique and ascending, cut at min(n, NOISE_MAX_WIDTH);
    cadence = numpy.median(numpy.diff(t)).  At 30 min that is 1, 3, 4, 5, 6, 7, 9, 10, 12, 15, 18, 21, 24, 25, 30.  ValueError
    for a t that is not [n >= 3], finite and ascending with a cadence > 0, and for hours that are not finite and > 0."""
    from ._lib import NOISE_MAX_WIDTH
    t, cadence = _noise_cadence(t)
    try:
        hours = numpy.atleast_1d(numpy.asarray(hours, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise ValueError("noise profile: hours must hold numbers")
    if hours.ndim != 1 or not numpy.all(numpy.isfinite(hours) & (hours > 0.0)):
        raise ValueError("noise profile: every pulse duration must be finite and > 0 hours")
    widths = {1} | {max(1, int(round(float(h) / 24.0 / float(cadence)))) for h in hours}
    top = min(len(t), NOISE_MAX_WIDTH)
    return numpy.array(sorted(w for w in widths if w <= top), dtype=numpy.int64)


def _noise_spans(t, widths, gap_tolerance):
    """(span_max [W], pair_span) of noise_profile: (w - 1 + gap_tolerance) * cadence for every width and
    (1 + gap_tolerance) * cadence, the adjacency limit of the point-to-point sigma; all inf without t."""
    _checks.finite_at_least("noise profile", "gap_tolerance", gap_tolerance)
    try:
        count = len(numpy.atleast_1d(numpy.asarray(widths)))
        steps = [numpy.float64(int(w) - 1) for w in numpy.atleast_1d(numpy.asarray(widths))]
    except (TypeError, ValueError, OverflowError):
        raise ValueError("noise profile: the widths must be integers, got %r" % (widths,))
    if t is None:
        return numpy.full(count, numpy.inf), numpy.inf
    t, cadence = _noise_cadence(t)
    g = numpy.float64(gap_tolerance)
    return numpy.array([(s + g) * cadence for s in steps], dtype=numpy.float64).reshape(count), float((numpy.float64(1.0) + g) * cadence)


def _noise_beta(robust, widths, sigma):
    """robust * sqrt(w) / sigma: 1 for white noise, larger with red noise."""
    with numpy.errstate(all="ignore"):
        return robust * numpy.sqrt(numpy.asarray(widths, dtype=numpy.float64)) / numpy.asarray(sigma)[..., None]


def noise_profile(flux_batch, t=None, widths=None, clip_upper=NOISE_CLIP, clip_lower=NOISE_CLIP, gap_tolerance=NOISE_GAP_TOLERANCE,
                  min_count=NOISE_MIN_COUNT, detrend=None, context=None, device=None, devices=None):
    """How noisy is every star on the time scale of a transit: a robust CDPP at the window widths `widths` (samples; None:
    noise_widths(t), the Kepler pulse durations), of every light curve of flux_batch [n_curves, n] (or one row [n]) on the
    shared ascending time stamps t (None: no gaps), on the device (tls_noise_profile).  K = 1.4826022185056018:

        m = median(y);  d = y - m;  sigma = K median(|d|);  sigma == 0: status 1, everything else NaN / 0
        keep = (d <= clip_upper sigma) and (d >= -clip_lower sigma): ONE pass, internal to the measurement (a deep eclipse
            does not inflate the profile; no row that is searched changes); inf switches a side off
        sigma_p2p = K median(|y_{j+1} - y_j|) / sqrt(2) over the kept neighbours at most (1 + gap_tolerance) cadences apart
        width w: v_i = the mean of d over the samples [i, i + w), valid when all are kept and t[i + w - 1] - t[i] <=
            (w - 1 + gap_tolerance) cadence;  count = the valid windows;  count < min_count: NaN
            robust = K median(|v - median(v)|);  rms = the standard deviation of v;  beta = robust sqrt(w) / sigma

    robust is the noise a transit of w samples competes with (depth sqrt(n_transits) / robust is its expected detection
    statistic), rms the same without the robustness (a transit inflates it), beta 1 for white noise and larger with red
    noise.  cadence = numpy.median(numpy.diff(t)).  The device equals the numpy statement in tests/noise_profile_spec.py bit
    for bit.  detrend= takes the steps and tuples of search_batch (a Biweight or a Prewhiten needs t), devices=[...] deals the
    curves out over several GPUs.  ValueError, before any device work (the detrending included), for non-finite input, a t
    that is not ascending, n < 3, widths that are not integers, not strictly ascending, below 1, above n or above
    NOISE_MAX_WIDTH, a negative or NaN clip, min_count < 1, widths=None without t and shapes that disagree.

    Returns a dict: widths [W]; curves, a structured array [n_curves] with noise_curve_fields(); count (int64), robust, rms
    and beta [n_curves, W].  One row gives one record and [W]."""
    from ._lib import noise_arguments
    if widths is None:
        if t is None:
            raise ValueError("noise profile: widths=None takes the Kepler pulse durations at the cadence of t, so it needs t")
        widths = noise_widths(t)
    one = numpy.ndim(flux_batch) == 1
    span_max, pair_span = _noise_spans(t, widths, gap_tolerance)
    a = noise_arguments(t, flux_batch, widths, span_max, pair_span, clip_upper, clip_lower, min_count)
    rows = a["y"]
    if _detrend_steps(detrend):
        if a["t"] is None and any(isinstance(step, (Biweight, Prewhiten)) for step in _detrend_steps(detrend)):
            raise ValueError("noise profile: a Biweight or a Prewhiten step of detrend needs t")
        axis = a["t"] if a["t"] is not None else numpy.arange(rows.shape[1], dtype=numpy.float64)
        rows = _detrended(axis, rows, detrend, context, device, devices)

    def call(ctx, lo, hi):
        curves, count, robust, rms = ctx.noise_profile(a["t"], rows[lo:hi], a["widths"], a["span_max"], a["pair_span"],
                                                       a["clip_upper"], a["clip_lower"], a["min_count"])
        return dict(curves=curves, count=count, robust=robust, rms=rms)

    out = dict(_run_batch(devices, device, context, len(rows), call))
    out["beta"] = _noise_beta(out["robust"], a["widths"], out["curves"]["sigma"])
    if one:
        out = {k: v[0] for k, v in out.items()}
    out["widths"] = a["widths"]
    return out


def _noise_request(noise, peak_fits, t):
    """None, or the checked request of noise=True (noise_widths(t)) or noise=widths of power_batch: a dict with widths,
    span_max, pair_span and cadence (ValueError for a bad one, and for noise without peak_fits)."""
    if noise is None or noise is False:
        return None
    if not peak_fits:
        raise ValueError("noise needs peak_fits=True: noise_mes is formed from depth_mean and transit_count of the fits")
    from ._lib import noise_arguments
    t, cadence = _noise_cadence(t)
    widths = noise_widths(t) if noise is True else noise
    span_max, pair_span = _noise_spans(t, widths, NOISE_GAP_TOLERANCE)
    a = noise_arguments(t, numpy.ones((1, len(t))), widths, span_max, pair_span, NOISE_CLIP, NOISE_CLIP, NOISE_MIN_COUNT)
    return dict(widths=a["widths"], span_max=a["span_max"], pair_span=a["pair_span"], cadence=float(cadence))


def noise_width_index(duration_days, cadence, widths):
    """The index of the profile width nearest duration_days / cadence, the smaller one on a tie; -1 where the duration is not
    finite."""
    x = numpy.asarray(duration_days, dtype=numpy.float64) / numpy.float64(cadence)
    w = numpy.asarray(widths, dtype=numpy.float64)
    with numpy.errstate(invalid="ignore"):
        index = numpy.argmin(numpy.fabs(w - x[..., None]), axis=-1)   # (the first of equals: the smaller width)
    return numpy.where(numpy.isfinite(x), index, -1)


def _noise_block(records, profile, cadence):
    """noise_width (the profile width nearest duration_days / cadence, the smaller one on a tie), noise_sigma (robust at that
    width) and noise_mes = depth_mean * sqrt(transit_count) / noise_sigma of the peaks `records`; NaN, and noise_width -1,
    where status != 0 or noise_sigma is NaN."""
    out = numpy.zeros(records.shape, dtype=[("noise_width", "f8"), ("noise_sigma", "f8"), ("noise_mes", "f8")])
    index = noise_width_index(records["duration_days"], cadence, profile["widths"])
    curve = numpy.arange(records.shape[0])[:, None]
    sigma = numpy.where(index >= 0, profile["robust"][curve, numpy.maximum(index, 0)], numpy.nan)
    good = (records["status"] == 0) & (index >= 0) & ~numpy.isnan(sigma)
    with numpy.errstate(all="ignore"):
        mes = records["depth_mean"] * numpy.sqrt(records["transit_count"]) / sigma
    out["noise_width"] = numpy.where(good, profile["widths"][numpy.maximum(index, 0)], -1)
    out["noise_sigma"] = numpy.where(good, sigma, numpy.nan)
    out["noise_mes"] = numpy.where(good, mes, numpy.nan)
    return out


def _with_noise(records, profile, cadence):
    """The peaks plus noise_width, noise_sigma and noise_mes (_noise_block)."""
    return _joined(records, _noise_block(records, profile, cadence))


def _peak_noise(ctx, env, request):
    """noise_curves, noise_count, noise_robust and noise_rms of a slice of the batch, on ctx: the profile of the rows that
    were searched."""
    names = ("noise_curves", "noise_count", "noise_robust", "noise_rms")
    return dict(zip(names, ctx.noise_profile(env.inp["t"], env.y_rows, request["widths"], request["span_max"],
                                             request["pair_span"], NOISE_CLIP, NOISE_CLIP, NOISE_MIN_COUNT)))


def _peak_noise_dict(out, request):
    """The `noise` entry of the peaks dict: what noise_profile returns, from the joined arrays of _peak_noise."""
    return dict(noise=dict(widths=request["widths"], curves=out["noise_curves"], count=out["noise_count"],
                           robust=out["noise_robust"], rms=out["noise_rms"],
                           beta=_noise_beta(out["noise_robust"], request["widths"], out["noise_curves"]["sigma"])))


# ---- the peak stages: every follow-up of power_batch(peaks=K, peak_fits=True), in the order of their field groups in `peaks` ----
# name: the power_batch keyword and the key of _power_batch's `stages`; keywords: the power_batch arguments `request` takes,
# in order; request: None, or the checked request; scope: "slice" -- run(ctx, env,
# request) for every device's slice inside its call, env a _PeakSlice -- or "batch" -- once behind the join, on the first
# context under its lock; run returns the stage's arrays by name, which are joined across the slices; block(out, request,
# records): the stage's own fields [n_curves, K] from the joined arrays `out`, records being the peaks with their fits (and
# scans); extras(out, request): what the stage adds to the peaks dict.
_PeakStage = collections.namedtuple("_PeakStage", ("name", "keywords", "request", "scope", "run", "block", "extras"))


def _no_extras(out, request):
    return {}


_PEAK_STAGES = (
    _PeakStage("transit_times", ("transit_times", "peak_fits", "transit_times_search", "transit_times_min_ses"),
               _transit_times_request, "slice", _peak_transit_times,
               lambda out, request, records: _with_ephemeris(None, out["tt_ephemeris"]),
               lambda out, request: dict(transit_times=_with_oc(out["tt_ephemeris"], out["tt_times"]))),
    _PeakStage("shape_fit", ("shape_fit", "peak_fits", "shape_fit_window", "shape_fit_min_count"),
               _shape_fit_request, "slice", _peak_shape_fits,
               lambda out, request, records: _with_shapes(None, out["shape_fits"], records["period"]), _no_extras),
    _PeakStage("sine_test", ("sine_test", "peak_fits", "sine_test_mask", "sine_test_harmonics"),
               _sine_test_request, "slice", _peak_sine_tests,
               lambda out, request, records: _with_sines(None, out["sine_tests"], out["sine_harmonics"]), _no_extras),
    _PeakStage("ephemeris_match", ("ephemeris_match", "peak_fits", "ephemeris_match_drift", "ephemeris_match_epoch",
                                   "ephemeris_match_max_ratio"),
               _ephemeris_match_request, "batch", _peak_matches,
               lambda out, request, records: _with_matches(None, out["matches"]), _no_extras),
    _PeakStage("views", ("views", "peak_fits", "views_global_bins", "views_local_bins", "views_local_durations",
                         "views_local_width"),
               _views_request, "slice", _peak_views,
               lambda out, request, records: _with_views(None, out["views_records"]), _peak_views_dict),
    _PeakStage("event_vetting", ("event_vetting", "peak_fits", "event_vetting_search", "event_vetting_chase_window",
                                 "event_vetting_guard", "event_vetting_min_ses", "event_vetting_chase_fraction",
                                 "event_vetting_chase_min", "event_vetting_point_fraction", "event_vetting_step_fraction"),
               _event_vetting_request, "slice", _peak_event_vetting,
               lambda out, request, records: _with_events(None, out["ev_summaries"]),
               lambda out, request: dict(events=out["ev_events"])),
    _PeakStage("centroids", ("centroids", "peak_fits", "flux_batch", "centroid_window", "centroid_min_in", "centroid_min_out"),
               lambda centroids, peak_fits, flux_batch, *options: _centroid_request(centroids, peak_fits,
                                                                                   numpy.shape(flux_batch), *options),
               "slice", _peak_centroid_tests,
               lambda out, request, records: _with_centroids(None, out["centroid_tests"]), _no_extras),
    _PeakStage("noise", ("noise", "peak_fits", "t"), _noise_request, "slice", _peak_noise,
               lambda out, request, records: _noise_block(records, dict(widths=request["widths"], robust=out["noise_robust"]),
                                                          request["cadence"]), _peak_noise_dict),
    _PeakStage("transit_fit", ("transit_fit", "peak_fits", "t", "power_kwargs"), _transit_fit_request, "slice",
               lambda ctx, env, request: dict(transit_fits=_peak_transit_fits(ctx, env.inp, env.y_rows, env.dy_rows, env.peaks,
                                                                              env.fits, request)),
               lambda out, request, records: _with_transit_fits(None, out["transit_fits"], records["period"], records["T0"]),
               _no_extras),
)


# ---- injection-recovery ---------------------------------------------------------------------------------------------------
INJECTION_FIELDS = ("T0", "period", "rp_rs", "a", "inc")
INJECTION_LAWS = ("quadratic", "linear", "uniform")


def _injection_table(injections):
    """The injections as a structured float64 array with the fields T0, period (days), rp_rs, a (a/R*) and inc (degrees),
    from a structured array or a dict of arrays; ValueError for anything the device model does not cover."""
    if isinstance(injections, dict):
        names = tuple(injections.keys())
    else:
        injections = numpy.asarray(injections)
        names = injections.dtype.names or ()
        if not names:
            raise ValueError("injections must be a structured array or a dict with fields %s" % (INJECTION_FIELDS,))
    for k in ("ecc", "w"):
        if k in names:
            raise ValueError("injections carry an %r field: injection-recovery injects circular orbits only (ecc = 0, w = 90)"
                             % k)
    missing = [k for k in INJECTION_FIELDS if k not in names]
    if missing:
        raise ValueError("injections lack the fields %s (wanted: %s)" % (missing, INJECTION_FIELDS))
    cols = [numpy.atleast_1d(numpy.asarray(injections[k], dtype=numpy.float64)) for k in INJECTION_FIELDS]
    if any(c.ndim != 1 for c in cols) or len({len(c) for c in cols}) != 1:
        raise ValueError("the injection fields must be 1-d arrays of one length")
    table = numpy.zeros(len(cols[0]), dtype=[(k, "f8") for k in INJECTION_FIELDS])
    for k, c in zip(INJECTION_FIELDS, cols):
        if not numpy.all(numpy.isfinite(c)):
            raise ValueError("injection field %r has a non-finite value" % k)
        table[k] = c
    if numpy.any(table["period"] <= 0):
        raise ValueError("injection periods must be > 0")
    if numpy.any(table["a"] <= 0):
        raise ValueError("injection a/R* must be > 0")
    if numpy.any(table["rp_rs"] < 0):
        raise ValueError("injection rp_rs must be >= 0")
    return table


def injection_constants(injections):
    """The tls_injection constants of every injection (_lib.INJECTION_DTYPE), formed by numpy as transit_model's
    _true_anomaly (ecc < 1e-5) and projected_separation form them for light_curve(t, T0, period, rp_rs, a, inc, 0, 90, ...)."""
    from ._lib import INJECTION_DTYPE
    table = _injection_table(injections)
    c = numpy.zeros(len(table), dtype=INJECTION_DTYPE)
    omega = numpy.radians(90)
    f_conj = numpy.pi / 2.0 - omega
    for k in range(len(table)):
        t0, per, inc = float(table["T0"][k]), float(table["period"][k]), float(table["inc"][k])
        c["tp"][k] = t0 - per * f_conj / (2.0 * numpy.pi)
        c["sin_inc"][k] = numpy.sin(numpy.radians(inc))   # (a scalar, as projected_separation takes it)
    c["period"], c["rp"], c["a"], c["omega"] = table["period"], table["rp_rs"], table["a"], omega
    return c


def _injection_law(inject_u, inject_limb_dark, power_kwargs):
    """(law, u1, u2) of the injected planet: inject_u / inject_limb_dark, else the search template's u / limb_dark, else the
    TLS defaults; u2 = 0 for the linear law, u1 = u2 = 0 for the uniform one (as transit_model.light_curve takes them)."""
    from . import constants as C
    law = inject_limb_dark if inject_limb_dark is not None else power_kwargs.get("limb_dark", C.DEFAULT_LIMB_DARK)
    if law not in INJECTION_LAWS:
        raise ValueError("injection limb darkening law %r has no closed form on the device: use one of %s"
                         % (law, INJECTION_LAWS))
    u = inject_u if inject_u is not None else power_kwargs.get("u", C.DEFAULT_U)
    u = [float(v) for v in numpy.atleast_1d(u)] if u is not None else []
    need = {"quadratic": 2, "linear": 1, "uniform": 0}[law]
    if len(u) < need:
        raise ValueError("limb darkening law %r needs %d coefficients, got %d" % (law, need, len(u)))
    if law == "quadratic":
        return law, u[0], u[1]
    if law == "linear":
        return law, u[0], 0.0
    return law, 0.0, 0.0


def injected_duration(injections):
    """T14 (days) of every injection on its circular orbit: b = a cos i,
    T14 = P / pi * arcsin(min(1, sqrt(max((1 + rp)^2 - b^2, 0)) / (a sin i)))."""
    table = _injection_table(injections)
    inc = numpy.radians(table["inc"])
    b = table["a"] * numpy.cos(inc)
    chord = numpy.sqrt(numpy.maximum((1.0 + table["rp_rs"]) ** 2 - b ** 2, 0.0)) / (table["a"] * numpy.sin(inc))
    return table["period"] / numpy.pi * numpy.arcsin(numpy.minimum(1.0, chord))


def classify_recovery(injections, summary, n_in_transit=None, sde_threshold=7.0, period_tolerance=0.01, aliases=(1.0,),
                      epoch_tolerance=None):
    """The recovery record of every injection from the search summary of its injected light curve (power_batch's summary:
    SDE, period, T0, no_fit).  period_match: the first factor m of `aliases` with |P_found - m P| <= period_tolerance m P,
    else 0; epoch_offset: the found T0 minus the nearest injected mid-time, these spaced min(m, 1) P (NaN without a match);
    recovered: no_fit == 0, SDE >= sde_threshold, a period match and |epoch_offset| <= epoch_tolerance (default 0.5 T14)."""
    table = _injection_table(injections)
    summary = numpy.asarray(summary)
    if len(summary) != len(table):
        raise ValueError("summary has %d records for %d injections" % (len(summary), len(table)))
    aliases = tuple(float(m) for m in aliases)
    if not aliases or any(not (m > 0) for m in aliases):
        raise ValueError("aliases must be positive period factors")
    fields = [(k, "f8") for k in INJECTION_FIELDS] + [("T14", "f8"), ("n_in_transit", "i8"), ("period_match", "f8"),
                                                       ("epoch_offset", "f8"), ("recovered", "?")]
    rec = numpy.zeros(len(table), dtype=fields)
    for k in INJECTION_FIELDS:
        rec[k] = table[k]
    rec["T14"] = injected_duration(table)
    rec["n_in_transit"] = -1 if n_in_transit is None else numpy.asarray(n_in_transit, dtype=numpy.int64)
    P, found_P, found_T0 = table["period"], summary["period"], summary["T0"]
    match = numpy.zeros(len(table))
    with numpy.errstate(invalid="ignore"):
        for m in aliases[::-1]:   # (the first factor that matches wins)
            ok = numpy.abs(found_P - m * P) <= period_tolerance * (m * P)
            match = numpy.where(ok, m, match)
        spacing = numpy.minimum(match, 1.0) * P
        offset = numpy.full(len(table), numpy.nan)
        has = match > 0
        d = found_T0[has] - table["T0"][has]
        offset[has] = d - numpy.rint(d / spacing[has]) * spacing[has]
        tol = 0.5 * rec["T14"] if epoch_tolerance is None else numpy.broadcast_to(float(epoch_tolerance), len(table))
        rec["period_match"] = match
        rec["epoch_offset"] = offset
        rec["recovered"] = ((summary["no_fit"] == 0) & (summary["SDE"] >= sde_threshold) & has
                            & (numpy.abs(offset) <= tol))
    return rec


def _search_chunks(t, n_rows, chunk, form, dy, return_rows, statistics, context, device, devices, power_kwargs):
    """power_batch on rows formed on the device chunk by chunk: form(ctx, lo, hi) -> (rows lo .. hi, extra) on the call's
    device (the given context or device, or the group's first one, under the group's lock), then _power_batch on those rows
    with dy (None, [n] or [n_rows, n]).  The lists (summaries, extras, rows -- empty without return_rows), one entry a chunk."""
    kind, what = _resolve(devices, device, context, n_rows)
    if kind == "group":
        form_ctx, lock = what.contexts[0], what._lock
    else:
        form_ctx, lock = (context if context is not None else _search.default_context(what)), contextlib.nullcontext()
    summaries, extras, all_rows = [], [], []
    for lo in range(0, n_rows, chunk):
        hi = min(n_rows, lo + chunk)
        with lock:
            rows, extra = form(form_ctx, lo, hi)
        dy_rows = None if dy is None else (numpy.broadcast_to(dy, rows.shape) if dy.ndim == 1 else dy[lo:hi])
        summaries.append(_power_batch(t, rows, dy_rows, power_kwargs, context=context, device=device, devices=devices,
                                      statistics=statistics)[0])
        extras.append(extra)
        if return_rows:
            all_rows.append(rows)
    return summaries, extras, all_rows


def _default_chunk(n):
    """Injections per chunk: the chunk's rows stay at or below about 256 MB, whole launch groups of 32 where that allows."""
    rows = max(1, (256 << 20) // (8 * max(int(n), 1)))
    return rows - rows % 32 if rows >= 32 else rows


def injection_recovery(t, flux, injections, dy=None, inject_u=None, inject_limb_dark=None, sde_threshold=7.0,
                       period_tolerance=0.01, aliases=(1.0,), epoch_tolerance=None, chunk=None, return_rows=False,
                       statistics=False, context=None, device=None, devices=None, detrend=None, **power_kwargs):
    """Injection-recovery in survey mode: inject every planet of `injections` into `flux` on the device
    (tls_inject_transits: flux * transit_model.light_curve(t, T0, period, rp_rs, a, inc, 0, 90, u, law)), search every
    injected light curve with power_batch, and classify each injection (classify_recovery).

    flux: [n] (every injection into the same base curve) or [n_injections, n]; dy: None (std of each injected row, as
    power() takes it), [n] or [n_injections, n].  injections: a structured array or dict with T0, period, rp_rs, a (a/R*)
    and inc (degrees); circular orbits only.  inject_u / inject_limb_dark set the injected planet's limb darkening
    (quadratic, linear or uniform), by default the search template's u / limb_dark of power_kwargs, else the TLS defaults;
    power_kwargs (u, limb_dark, ecc, w included) go to the search unchanged.

    Per chunk of `chunk` injections (default: about 256 MB of rows, a multiple of 32): the rows are formed on the call's
    device (the given context or device, or the group's first one), copied to the host, searched by power_batch (with
    `statistics` and `devices` passed through) and classified.  The round trip makes the search's inputs exactly
    power_batch's, so `summary` equals power_batch(t, rows, dy) on the same rows.

    detrend=k (an odd kernel size): `flux` is the RAW light curve, and every injected row is detrended on the same device
    right after the injection (row / medfilt(row, k), tls_medfilt_detrend) before it is searched, so the transits pass through
    the filter the data pass through, and completeness counts what the filter absorbs.  rows are then the detrended rows;
    n_in_transit and the classification are unchanged, and dy is passed through as it is.  detrend=Biweight(window_length,
    break_tolerance) does the same with the time-windowed biweight (tls_biweight_detrend, biweight_batch), and a tuple of
    such steps applies them left to right.  A SysRem raises ValueError: the rows all come from ONE star; so does a Decorrelate, whose
    columns belong to rows the caller holds (decorrelate the star's flux with decorrelate_batch first).

    Returns (recovery, summary[, rows]): recovery a structured array -- the injected fields, T14, n_in_transit (points
    with z < 1 + rp_rs: 0 where every transit falls into a gap), period_match, epoch_offset, recovered -- and summary
    power_batch's summary; rows [n_injections, n] with return_rows=True."""
    table = _injection_table(injections)
    n_inj = len(table)
    t = numpy.asarray(t, dtype=numpy.float64)
    if t.ndim != 1:
        raise ValueError("t must be 1-d")
    n = len(t)
    flux = numpy.asarray(flux, dtype=numpy.float64)
    if flux.shape not in ((n,), (n_inj, n)):
        raise ValueError("flux must have shape [len(t)] or [n_injections, len(t)], got %s" % (flux.shape,))
    if dy is not None:
        dy = numpy.asarray(dy, dtype=numpy.float64)
        if dy.shape not in ((n,), (n_inj, n)):
            raise ValueError("dy must be None or have shape [len(t)] or [n_injections, len(t)], got %s" % (dy.shape,))
    _, u1, u2 = _injection_law(inject_u, inject_limb_dark, power_kwargs)
    chunk = _default_chunk(n) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    # (checked before any device work)
    classify_recovery(table[:0], numpy.zeros(0, dtype=[("period", "f8"), ("T0", "f8"), ("SDE", "f8"), ("no_fit", "i8")]),
                      None, sde_threshold, period_tolerance, aliases, epoch_tolerance)
    _no_ensemble_step(detrend, "injection_recovery")
    _no_regression_step(detrend, "injection_recovery")
    # (behind a Clean at the head the later steps see repaired rows: their checks take rows of ones of flux's shape)
    probe = numpy.ones(flux.shape) if isinstance((_detrend_steps(detrend) or (None,))[0], Clean) else flux
    for step in _detrend_steps(detrend):
        if isinstance(step, Biweight):
            from ._lib import biweight_arguments
            biweight_arguments(t, probe, step.window_length, step.break_tolerance)
        elif isinstance(step, Prewhiten):
            from ._lib import prewhiten_arguments
            grid, k, h, low = _prewhiten_step(t, step, n)
            prewhiten_arguments(t, probe, None, grid, k, h, low)
        elif isinstance(step, Spline):
            from ._lib import spline_arguments
            spline_arguments(t, probe, *step)
        elif isinstance(step, Clean):
            from ._lib import clean_arguments
            clean_arguments(t, flux, **_clean_step(step))
        else:
            from ._lib import medfilt_arguments
            medfilt_arguments(probe, step)
    consts = injection_constants(table)

    def form(ctx, lo, hi):
        rows, count = ctx.inject_transits(t, flux if flux.ndim == 1 else flux[lo:hi], consts[lo:hi], u1, u2)
        return _detrend_rows(ctx, t, rows, detrend), count

    summaries, counts, all_rows = _search_chunks(t, n_inj, chunk, form, dy, return_rows, statistics, context, device, devices,
                                                 power_kwargs)
    if not summaries:
        raise ValueError("no injections")
    summary, count = numpy.concatenate(summaries), numpy.concatenate(counts)
    recovery = classify_recovery(table, summary, count, sde_threshold, period_tolerance, aliases, epoch_tolerance)
    if return_rows:
        return recovery, summary, numpy.concatenate(all_rows)
    return recovery, summary


def injection_grid(t, periods, rp_rs, per_cell=1, b_max=0.0, seed=0, R_star=1.0, M_star=1.0):
    """Deterministic injections on a (period, rp_rs) grid, `per_cell` of each pair (periods outermost): T0 = min(t) + U(0, 1) P,
    a/R* from Kepler's third law (tls_amd.constants G, R_sun, M_sun; R_star, M_star in solar units), b ~ U(0, b_max) and
    inc = degrees(arccos(b / a)).  The draws come from numpy.random.RandomState(seed) (T0 of all injections, then b), never
    from the global generator.  Returns the structured array injection_recovery takes."""
    from . import constants as C
    periods = numpy.atleast_1d(numpy.asarray(periods, dtype=numpy.float64))
    rp_rs = numpy.atleast_1d(numpy.asarray(rp_rs, dtype=numpy.float64))
    per_cell = int(per_cell)
    if periods.ndim != 1 or rp_rs.ndim != 1 or per_cell < 1:
        raise ValueError("periods and rp_rs must be 1-d, per_cell >= 1")
    if not (0.0 <= float(b_max)):
        raise ValueError("b_max must be >= 0")
    P = numpy.repeat(periods, len(rp_rs) * per_cell)
    rp = numpy.tile(numpy.repeat(rp_rs, per_cell), len(periods))
    rng = numpy.random.RandomState(seed)
    T0 = numpy.min(t) + rng.uniform(0.0, 1.0, len(P)) * P
    b = rng.uniform(0.0, float(b_max), len(P))
    P_s = P * C.SECONDS_PER_DAY
    a = (C.G * (M_star * C.M_sun) * P_s ** 2 / (4.0 * numpy.pi ** 2)) ** (1.0 / 3.0) / (R_star * C.R_sun)
    out = numpy.zeros(len(P), dtype=[(k, "f8") for k in INJECTION_FIELDS])
    out["T0"], out["period"], out["rp_rs"], out["a"] = T0, P, rp, a
    out["inc"] = numpy.degrees(numpy.arccos(b / a))
    _injection_table(out)
    return out


def completeness(recovery, period_edges, rp_edges, exclude_untransiting=True):
    """Recovered fraction per (period, rp_rs) cell: (fraction, recovered, total), each [len(period_edges) - 1,
    len(rp_edges) - 1] (numpy.histogram2d bins; fraction NaN in an empty cell).  exclude_untransiting leaves out the
    injections without a point in transit (n_in_transit == 0)."""
    rec = numpy.asarray(recovery)
    keep = numpy.ones(len(rec), dtype=bool)
    if exclude_untransiting:
        keep &= rec["n_in_transit"] != 0
    bins = (numpy.asarray(period_edges, dtype=numpy.float64), numpy.asarray(rp_edges, dtype=numpy.float64))
    total = numpy.histogram2d(rec["period"][keep], rec["rp_rs"][keep], bins=bins)[0].astype(numpy.int64)
    hit = keep & rec["recovered"]
    recovered = numpy.histogram2d(rec["period"][hit], rec["rp_rs"][hit], bins=bins)[0].astype(numpy.int64)
    with numpy.errstate(invalid="ignore", divide="ignore"):
        fraction = numpy.where(total > 0, recovered / numpy.maximum(total, 1), numpy.nan)
    return fraction, recovered, total


# ---- false-alarm calibration: SDE of searches on noise alone --------------------------------------------------------------
NULL_SIGMA_MAX = 0.1   # (tls_null_rows' bound on the white-noise sigma)


def _integer(name, value, lo, hi=None):
    """int(value) for an integral `value` in [lo, hi); ValueError otherwise."""
    try:
        v = operator.index(value)
    except TypeError:
        raise ValueError("%s must be an integer, got %r" % (name, value))
    if v < lo or (hi is not None and v >= hi):
        raise ValueError("%s must lie in [%d, %s), got %d" % (name, lo, "inf" if hi is None else hi, v))
    return v


def _null_arguments(t, n_trials, sigma, source, block, seed, first_trial):
    """(t, mode, sigma, source, block, seed, first_trial) checked as tls_null_rows checks them, plus the Philox counter bound
    of the last trial; sigma a float64 array ([1] or [n_trials]) in mode 0, source [n_src, n] in mode 1."""
    t = numpy.asarray(t, dtype=numpy.float64)
    if t.ndim != 1 or len(t) < 1:
        raise ValueError("t must be a non-empty 1-d array")
    n = len(t)
    n_trials = _integer("n_trials", n_trials, 1)
    seed = _integer("seed", seed, 0, 2 ** 64)
    first_trial = _integer("first_trial", first_trial, 0)
    if source is None:
        if block is not None:
            raise ValueError("block is the bootstrap's: it needs a source")
        if sigma is None:
            raise ValueError("white noise (no source) needs sigma")
        sigma = numpy.asarray(sigma, dtype=numpy.float64)
        if sigma.shape not in ((), (n_trials,)):
            raise ValueError("sigma must be a scalar or have shape [n_trials], got %s" % (sigma.shape,))
        if not numpy.all((sigma > 0) & (sigma <= NULL_SIGMA_MAX)):
            raise ValueError("sigma must lie in (0, %g]" % NULL_SIGMA_MAX)
        sigma = numpy.atleast_1d(sigma)
        words = 2 * n
    else:
        if sigma is not None:
            raise ValueError("sigma is the white noise's: a bootstrap (source given) takes none")
        if block is None:
            raise ValueError("a bootstrap (source given) needs block")
        block = _integer("block", block, 1, n + 1)
        source = numpy.asarray(source, dtype=numpy.float64)
        if source.ndim == 1:
            source = source[None, :]
        if source.ndim != 2 or source.shape[1] != n or len(source) < 1:
            raise ValueError("source must have shape [len(t)] or [n_sources, len(t)], got %s" % (numpy.shape(source),))
        if not numpy.all(numpy.isfinite(source) & (source > 0)):
            raise ValueError("source has a non-finite or non-positive value")
        words = -(-n // block)
    if first_trial + n_trials > (2 ** 64 - 2) // (-(-words // 4)):
        raise ValueError("trials first_trial .. first_trial + n_trials - 1 run past the 64-bit Philox counter")
    return t, (0 if source is None else 1), sigma, source, block, seed, first_trial


def null_sde(t, n_trials, sigma=None, source=None, block=None, seed=0, first_trial=0, dy=None, chunk=None, return_rows=False,
             statistics=False, context=None, device=None, devices=None, detrend=None, **power_kwargs):
    """Search `n_trials` null (noise-only) light curves formed on the device and return their power_batch summary: the
    SDE of every search of noise alone, the input of fap_table.

    White noise (source None): row R is 1 + sigma_R z, z standard normals (Box-Muller on numpy's Philox4x64-10 stream);
    sigma a scalar or [n_trials], each in (0, 0.1].  Block bootstrap (source [n] or [n_sources, n], block L in [1, n]):
    row R copies source row R mod n_sources in blocks of L points taken from uniformly drawn starts, which keeps the
    sources' correlated noise on time scales below L and breaks any periodicity.  Row R depends on (seed, R) alone
    (tls_null_rows: trial R takes its own stretch of the stream), trials being R = first_trial .. first_trial + n_trials
    - 1, so splitting a calibration into calls over consecutive first_trial gives the same rows.

    Per chunk of `chunk` trials (default: about 256 MB of rows, a multiple of 32) the rows are formed on the call's device
    (the given context or device, or the group's first one), copied to the host and searched by power_batch (`dy`,
    `statistics`, `devices` and power_kwargs passed through), so `summary` equals power_batch(t, rows, dy) on the same
    rows.  dy: None (std of each row, as power() takes it), [n] or [n_trials, n].

    detrend=k (an odd kernel size) detrends every null row on the same device right after it is formed (row / medfilt(row, k),
    tls_medfilt_detrend) and searches the detrended rows: the null of a pipeline that detrends.  A bootstrap then takes RAW
    source rows, filtered after resampling as the data are.  A row still depends on (seed, R) alone; rows are then the
    detrended rows, and dy is passed through as it is.  detrend=Biweight(window_length, break_tolerance) does the same with
    the time-windowed biweight (tls_biweight_detrend, biweight_batch), and a tuple of such steps applies them left to
    right.  A SysRem raises ValueError: the rows all come from ONE star; so does a Decorrelate, whose
    columns belong to rows the caller holds (decorrelate the star's flux with decorrelate_batch first).

    Returns summary, or (summary, rows [n_trials, n]) with return_rows=True."""
    t, mode, sigma, source, block, seed, first_trial = _null_arguments(t, n_trials, sigma, source, block, seed, first_trial)
    n_trials, n = int(n_trials), len(t)
    if dy is not None:
        dy = numpy.asarray(dy, dtype=numpy.float64)
        if dy.shape not in ((n,), (n_trials, n)):
            raise ValueError("dy must be None or have shape [len(t)] or [n_trials, len(t)], got %s" % (dy.shape,))
        if not numpy.all(numpy.isfinite(dy) & (dy > 0)):
            raise ValueError("dy must be finite and positive")
    chunk = _default_chunk(n) if chunk is None else _integer("chunk", chunk, 1)
    if statistics and not numpy.all(t[1:] >= t[:-1]):
        raise ValueError("statistics=True needs ascending time stamps t")
    _no_ensemble_step(detrend, "null_sde")
    _no_regression_step(detrend, "null_sde")
    for step in _detrend_steps(detrend):
        if isinstance(step, Biweight):
            from ._lib import biweight_windows
            biweight_windows(t, step.window_length, step.break_tolerance)
        elif isinstance(step, Prewhiten):
            from ._lib import prewhiten_arguments
            grid, k, h, low = _prewhiten_step(t, step, n)
            prewhiten_arguments(t, numpy.ones(n), None, grid, k, h, low)
        elif isinstance(step, Spline):
            from ._lib import spline_arguments
            spline_arguments(t, numpy.ones(n), *step)
        elif isinstance(step, Clean):
            from ._lib import clean_arguments
            clean_arguments(t, numpy.ones(n), **_clean_step(step))
        else:
            from ._lib import medfilt_kernel
            medfilt_kernel(step, n)

    def form(ctx, lo, hi):
        sig = None if mode == 1 else sigma if len(sigma) == 1 else sigma[lo:hi]
        rows = ctx.null_rows(n, hi - lo, seed, first_trial + lo, sigma=sig, source=source, block=block)
        return _detrend_rows(ctx, t, rows, detrend), None

    summaries, _, all_rows = _search_chunks(t, n_trials, chunk, form, dy, return_rows, statistics, context, device, devices,
                                            power_kwargs)
    summary = numpy.concatenate(summaries)
    if return_rows:
        return summary, numpy.concatenate(all_rows)
    return summary


def fap_table(null_sde, max_fap=0.1):
    """A false-alarm table from the SDE of n null searches, in the format of the reference's fap.csv (stats._fap_table):
    (fap [m + 1], thresholds [m + 1], n) with m = min(n, ceil(max_fap n) + 1), thresholds the m largest SDE ascending and
    then inf, fap[k] = max(m - k, 1) / n and fap[0] = NaN.  For n = 12495 and max_fap = 0.1 that is the reference's shape
    (m = 1251).  Every value must be finite (a search without a fit reports SDE 0 and counts as 0)."""
    x = numpy.asarray(null_sde, dtype=numpy.float64)
    if x.ndim != 1 or len(x) < 1:
        raise ValueError("null_sde must be a non-empty 1-d array")
    if not numpy.all(numpy.isfinite(x)):
        raise ValueError("null_sde has a non-finite value")
    max_fap = float(max_fap)
    if not (0.0 < max_fap <= 1.0):
        raise ValueError("max_fap must lie in (0, 1]")
    n = len(x)
    m = min(n, int(numpy.ceil(max_fap * n)) + 1)
    thresholds = numpy.append(numpy.sort(x)[n - m:], numpy.inf)
    fap = numpy.maximum(m - numpy.arange(m + 1), 1) / n
    fap[0] = numpy.nan
    return fap, thresholds, n


def _fap_of(table):
    """(fap, thresholds, n) of a fap_table result, checked."""
    fap, thr, n = table
    fap, thr, n = numpy.asarray(fap, dtype=numpy.float64), numpy.asarray(thr, dtype=numpy.float64), int(n)
    if fap.ndim != 1 or fap.shape != thr.shape or len(fap) < 2 or n < 1:
        raise ValueError("not a fap_table: (fap [m + 1], thresholds [m + 1], n)")
    if numpy.any(numpy.isnan(thr)) or not numpy.all(thr[1:] >= thr[:-1]) or thr[-1] != numpy.inf:
        raise ValueError("not a fap_table: the thresholds must ascend and end with inf")
    return fap, thr, n


def empirical_fap(sde, table):
    """The false-alarm probability of every entry of `sde` under a fap_table, by the reference's rule
    fap[argmax(thresholds > SDE)] (stats.FAP): NaN below the smallest kept SDE (and for NaN or inf), 1 / n at the top."""
    fap, thr, _ = _fap_of(table)
    sde = numpy.asarray(sde, dtype=numpy.float64)
    flat = sde.ravel()
    # (ascending thresholds: the first one above SDE is a binary search; none above -- inf or NaN SDE -- gives 0, like argmax)
    idx = numpy.searchsorted(thr, flat, side="right")
    idx[(idx >= len(thr)) | numpy.isnan(flat)] = 0
    out = fap[idx].reshape(sde.shape)
    return out if out.ndim else out[()]


def sde_threshold(table, target_fap):
    """The smallest SDE x with empirical_fap(x, table) <= target_fap: thresholds[k - 1] for the smallest k >= 1 with
    fap[k] <= target_fap.  ValueError for a target outside [1 / n, fap[1]] (fap[1] = (m - 1) / n, at least the table's
    max_fap)."""
    fap, thr, n = _fap_of(table)
    target = float(target_fap)
    if not (1.0 / n <= target <= fap[1]):
        raise ValueError("target_fap must lie in [1/n, max_fap] = [%.6g, %.6g] of this table, got %r" % (1.0 / n, fap[1], target_fap))
    k = 1 + int(numpy.argmax(fap[1:] <= target))
    return float(thr[k - 1])
