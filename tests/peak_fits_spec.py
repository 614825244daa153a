"""The peak-fit stage of power_batch(peaks=K, peak_fits=True) / tls_debug_peak_fits, restated with numpy and the project's
host functions: what the device is tested against bit for bit (include/tls_amd.h tls_peak_fit, DESIGN.md "Peak fits").

A candidate is (period, depth, row, index) of one peak on the light curve y -- period, depth AND template row all from the
peak's own index:

    status  1 where rank >= n_peaks, 2 where row < 0, else 0; T0 and every statistics field NaN unless 0
    T0      stats.final_T0_fit of template row `row` scaled to `depth` (the residuals of the trial epochs from the device
            kernel of the single fit, search.t0_fit_residuals, on the same context: the product has no host evaluation)
    stats   api.py:175-241 through stats.py, as tests/test_power_batch_statistics.py host_stats forms them (the odd and even
            depth errors from stats.intransit_stats, like power()), with the period-uncertainty walk started at `index`
            instead of argmax(power)
"""
import warnings

import numpy

from tls_amd import search
from tls_amd.helpers import transit_mask
from tls_amd.stats import (_intransit_fluxes, all_transit_times, calculate_fill_factor, calculate_transit_duration_in_days,
                           count_stats, final_T0_fit, intransit_stats)

FITTED, NONE, UNFITTED = 0, 1, 2


def period_uncertainty_at(periods, power, index):
    """stats.period_uncertainty with the peak given: half the full width at half maximum around `index`, inf where a walk
    leaves the grid (the lower walk wraps through negative indices first, as the reference's does)."""
    try:
        peak = int(index)
        half = 0.5 * power[peak]
        upper = peak + 1
        while power[upper] > half:
            upper += 1
        lower = peak - 1
        while power[lower] > half:
            lower -= 1
        return 0.5 * (periods[upper] - periods[lower])
    except Exception:
        return float("inf")


def candidate_T0(ctx, inp, y, period, depth, row):
    return final_T0_fit(signal=inp["rows"][int(row)], depth=depth, t=inp["t"], y=y, dy=None, period=period,
                        T0_fit_margin=inp["params"]["T0_fit_margin"], show_progress_bar=False, verbose=False,
                        residuals_fn=lambda *a: search.t0_fit_residuals(*a, context=ctx))


def candidate_stats(t, y, period, T0, duration, periods, power, index):
    """The tls_transit_stats record of one candidate (dict by field)."""
    with warnings.catch_warnings(), numpy.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        transit_times = all_transit_times(T0, t, period)
        fill = calculate_fill_factor(t)
        d = calculate_transit_duration_in_days(t, period, transit_times, duration, fill_factor=fill)
        chunks = _intransit_fluxes(t, y, transit_times, d)
        flux_ootr = y[~transit_mask(t, period, 2 * duration, T0)]
        (mo, me, mos, mes, fo, fe, ptc, td, tdu) = intransit_stats(t, y, transit_times, d, chunks=chunks)
        all_flux = numpy.concatenate([fo, fe])
        std_ootr = numpy.std(flux_ootr)
        dm = numpy.mean(all_flux)
        dms = numpy.std(all_flux) / numpy.sum(ptc) ** (0.5)
        snr = ((1 - dm) / std_ootr) * len(all_flux) ** (0.5)
        n_in, n_after, n_before = count_stats(t, y, transit_times, d)
        mismatch = abs(mo - me) / (mos + mes)
        E = len(transit_times)
        empty = numpy.count_nonzero(ptc == 0)
    return dict(period_uncertainty=period_uncertainty_at(periods, power, index), duration_days=d, depth_mean=dm,
                depth_mean_std=dms, depth_mean_even=me, depth_mean_even_std=mes, depth_mean_odd=mo, depth_mean_odd_std=mos,
                snr=snr, odd_even_mismatch=mismatch, transit_count=E, distinct_transit_count=E - empty,
                empty_transit_count=empty, in_transit_count=n_in, after_transit_count=n_after, before_transit_count=n_before)


def expected(ctx, inp, y, peak, rank, n_peaks, power):
    """The tls_peak_fit of one peak record (anything with period, depth, row, index) at `rank` of a curve with n_peaks peaks:
    dict with T0, status and the statistics fields."""
    from tls_amd._lib import TRANSIT_STATS_FIELDS
    nothing = dict(T0=numpy.nan, **{k: numpy.nan for k in TRANSIT_STATS_FIELDS})
    if rank >= n_peaks:
        return dict(nothing, status=NONE)
    if int(peak["row"]) < 0:
        return dict(nothing, status=UNFITTED)
    period, depth, row, index = float(peak["period"]), float(peak["depth"]), int(peak["row"]), int(peak["index"])
    T0 = candidate_T0(ctx, inp, y, period, depth, row)
    rec = candidate_stats(inp["t"], y, period, T0, inp["table"].duration[row], inp["periods"], power, index)
    return dict(rec, T0=T0, status=FITTED)
