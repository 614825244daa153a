"""Survey mode (BASELINE config 5): many light curves on the SAME time stamps, grids and
template searched back to back on one GPU by ONE C-ABI call (`tls_search_batch`).  The plan (period
list, duration windows, template rows, work queue order) is prepared once; per light curve only
the flux (and weights) are re-uploaded before the search kernel runs again.

Across GPUs the light curves are simply dealt out: one process per GPU (bench.py), or `devices=[0, 1, ...]` / `devices="auto"`
(every visible GPU) on the calls below -- contiguous slices of the batch to the contexts of a `tls_amd.search.DeviceGroup`, one host thread each, no
collective (every light curve's results come back over its own GPU's copy engine).
"""
import numpy

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


def power_batch(t, flux_batch, dy_batch=None, context=None, device=None, with_arrays=False, devices=None, statistics=False,
                per_transit=False, models=False, **power_kwargs):
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

    Returns (summary, periods[, chi2, row, depth, power][, per_transit][, models]): summary is a numpy structured array with
    the fields of tls_power_summary plus "duration" (and the statistics on request)."""
    return _power_batch(t, flux_batch, dy_batch, context, device, with_arrays, devices, statistics, per_transit, models,
                        False, power_kwargs)


def _power_batch(t, flux_batch, dy_batch, context, device, with_arrays, devices, statistics, per_transit, models, spectra,
                 power_kwargs):
    """power_batch; spectra=True (power_results) also returns SR and power_raw [n_curves, n_periods] behind the arrays."""
    models = bool(models)
    per_transit = bool(per_transit or models)
    statistics = bool(statistics or per_transit)
    if statistics:
        t_check = numpy.asarray(t, dtype=numpy.float64)
        if t_check.ndim != 1 or not numpy.all(t_check[1:] >= t_check[:-1]):
            raise ValueError("statistics=True needs ascending time stamps t")
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, power_kwargs)
    from . import constants as C
    osf = power_kwargs.get("oversampling_factor", C.OVERSAMPLING_FACTOR)
    kernel = osf * C.SDE_MEDIAN_KERNEL_SIZE
    if kernel != int(kernel):
        raise ValueError("oversampling_factor * %d must be an integer" % C.SDE_MEDIAN_KERNEL_SIZE)

    if statistics:
        from .stats import calculate_fill_factor
        fill_factor = calculate_fill_factor(inp["t"])
        root = numpy.array([float(k) ** 0.5 for k in range(len(inp["t"]) + 1)])   # (Python's pow, as power() forms k ** 0.5)
        max_epochs = _max_epochs(inp["t"], inp["periods"])
        template = _model_template(inp) if models else None
        lc_cap = _lc_cap(len(inp["t"]), max_epochs) if models else 0

        def call(ctx, lo, hi):
            return ctx.power_batch_stats(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], inp["periods"], inp["table"], inp["params"],
                                         int(kernel), fill_factor, root, max_epochs, per_transit=per_transit,
                                         with_arrays=with_arrays, with_spectra=spectra, models=template, lc_cap=lc_cap)
    else:
        def call(ctx, lo, hi):
            return ctx.power_batch(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], inp["periods"], inp["table"], inp["params"],
                                   int(kernel), with_arrays=with_arrays, with_power=with_arrays)

    kind, what = _resolve(devices, device, context, len(y_rows))
    if kind == "group":
        parts = _on_devices(what, call, len(y_rows))
    else:
        ctx = context if context is not None else _search.default_context(what)
        parts = [call(ctx, 0, len(y_rows))]
    # (one part: its arrays as they are -- the padded model rows of a large batch run to hundreds of MB)
    out = [None if parts[0][k] is None else parts[0][k] if len(parts) == 1 else numpy.concatenate([p[k] for p in parts])
           for k in range(len(parts[0]))]
    if statistics:
        raw, tstats, rows, n_epochs, chi2, row, depth, power = out[:8]
        extra = out[8:]
        if spectra:
            SR, power_raw = extra[:2]
            extra = extra[2:]
    else:
        raw, chi2, row, depth, power = out
    names = list(raw.dtype.names) + ["duration"]
    fields = [(k, raw.dtype[k]) for k in raw.dtype.names] + [("duration", "f8")]
    if statistics:
        fields += [(k, "f8") for k in tstats.dtype.names] + [("rp_rs", "f8"), ("FAP", "f8"), ("chi2red_min", "f8")]
    summary = numpy.zeros(len(raw), dtype=fields)
    for k in raw.dtype.names:
        summary[k] = raw[k]
    summary["duration"] = numpy.where(raw["no_fit"] != 0, numpy.nan, inp["table"].duration[raw["best_row"]])
    assert names == list(summary.dtype.names)[:len(names)]
    if statistics:
        from .stats import limb_darkening_factor
        for k in tstats.dtype.names:
            summary[k] = tstats[k]
        # rp_rs_from_depth(1 - depth) curve by curve (numpy's scalar ** 0.5, as power() takes it); NaN without a fit
        factor = limb_darkening_factor(inp["limb_dark"], inp["u"])
        fit = raw["no_fit"] == 0
        summary["rp_rs"] = numpy.nan
        summary["rp_rs"][fit] = [x ** (1 / 2) for x in (1 - raw["depth"][fit]) * factor]
        summary["FAP"] = _fap(raw["SDE"])
        summary["chi2red_min"] = raw["chi2_min"] / (len(inp["t"]) - 4)
    result = (summary, inp["periods"])
    if with_arrays:
        result += (chi2, row, depth, power)
    if per_transit:
        from ._lib import PER_TRANSIT_FIELDS
        pt = {k: rows[:, i, :] for i, k in enumerate(PER_TRANSIT_FIELDS)}
        pt["n_epochs"] = n_epochs
        result += (pt,)
    if models:
        folded, model_folded, lightcurve, lc_len = extra
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
    if spectra:
        result += (SR, power_raw)
    return result


def power_results(t, flux_batch, dy_batch=None, context=None, device=None, devices=None, **power_kwargs):
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
    devices=[...] deals the batch out over several GPUs, as the other survey calls."""
    from .api import transitleastsquares
    from .results import transitleastsquaresresults
    if len(numpy.shape(flux_batch)) != 2 or numpy.shape(flux_batch)[1] != len(t):
        raise ValueError("flux_batch must have shape [n_curves, len(t)]")
    if dy_batch is not None and numpy.shape(dy_batch) != numpy.shape(flux_batch):
        raise ValueError("dy_batch must have the shape of flux_batch")
    summary, periods, chi2, row, depth, power, pt, m, SR, power_raw = _power_batch(
        t, flux_batch, dy_batch, context, device, True, devices, True, True, True, True, power_kwargs)
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


def search_batch(t, flux_batch, dy_batch=None, context=None, device=None, devices=None, **power_kwargs):
    """Search every light curve of `flux_batch` (shape [n_curves, n_points]) on the grids that
    `transitleastsquares(t, flux).power(**power_kwargs)` would use.

    Returns (periods, chi2[n_curves, n_periods], row[...], depth[...]).  All light curves must
    share `t` and be free of invalid points (clean them first); a `dy_batch` must have the same
    weight structure for every curve (all uniform or all per-point).
    """
    inp, y_rows, dy_rows = _batch_inputs(t, flux_batch, dy_batch, power_kwargs)

    def call(ctx, lo, hi):
        return ctx.search_batch(inp["t"], y_rows[lo:hi], dy_rows[lo:hi], inp["periods"], inp["table"], inp["params"])

    kind, what = _resolve(devices, device, context, len(y_rows))
    if kind == "group":
        parts = _on_devices(what, call, len(y_rows))
        chi2, row, depth = (numpy.concatenate([p[k] for p in parts]) for k in range(3))
    else:
        ctx = context if context is not None else _search.default_context(what)
        chi2, row, depth = call(ctx, 0, len(y_rows))
    return inp["periods"], chi2, row, depth
