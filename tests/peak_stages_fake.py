"""A stand-in for tls_amd._lib.Context that runs power_batch's whole host chain without a device, and the cases
tests/test_peak_stages_host.py and tools/gen_peak_stages_golden.py both run on it.

Every record is a fixed function of the candidate's own arguments, of the call's scalar options and of its curve's rows
(their exactly rounded sums, math.fsum), formed with single IEEE additions and multiplications in a fixed order: a
misrouted argument changes the bytes, the candidate's position in the call does not.  The one exception is the ephemeris
match, whose `best` is an index into the call's candidates by its nature.
"""
import json
import math
import threading

import numpy

from tls_amd import _lib


def _row_sums(rows):
    """math.fsum of every row of [n_rows, n] (None: None): the same double on every machine."""
    if rows is None:
        return None
    return numpy.array([math.fsum(r) for r in numpy.atleast_2d(numpy.asarray(rows, dtype=numpy.float64))])


def _scalar(v):
    """A plain number for the call list."""
    return int(v) if isinstance(v, (bool, int, numpy.integer)) else float(v)


def _mix(*parts):
    """sum_i (2 i + 1) * part_i over arrays and numbers, NaN taken as -1, left to right."""
    total = 0.0
    for i, part in enumerate(parts):
        part = numpy.asarray(part, dtype=numpy.float64)
        total = total + (2.0 * i + 1.0) * numpy.where(numpy.isnan(part), -1.0, part)
    return total


def _records(dtype, base, shape=None, live=None, first=0.0):
    """Records of `dtype` [len(base)] (or [len(base)] + shape): field j holds base * (1 + j / 16) + j (plus the index along
    the trailing axis), the first field `first` -- a status -- and, where live is False, status 1 and NaN elsewhere."""
    base = numpy.asarray(base, dtype=numpy.float64)
    out = numpy.zeros(base.shape + (shape or ()), dtype=dtype)
    tail = numpy.arange(int(numpy.prod(shape or (1,))), dtype=numpy.float64).reshape(shape or ())
    for j, name in enumerate(dtype.names):
        value = base * (1.0 + j / 16.0) + j
        value = value.reshape(base.shape + (1,) * len(shape or ())) + tail
        if j == 0:
            value = numpy.full(value.shape, first)
        if live is not None:
            dead = ~numpy.asarray(live).reshape(base.shape + (1,) * len(shape or ()))
            value = numpy.where(dead, 1.0 if j == 0 else numpy.nan, value)
        out[name] = value
    return out


class FakeContext(object):
    """The bindings power_batch's chain calls, with their signatures, return dtypes and shapes; `log` (shared by the
    contexts of a group) gets (context name, call name, curves, candidates, scalar options) for every call."""

    def __init__(self, name="ctx0", log=None):
        self.name = name
        self.log = [] if log is None else log

    def _note(self, call, curves, candidates, **options):
        self.log.append([self.name, call, int(curves), int(candidates), {k: _scalar(v) for k, v in sorted(options.items())}])

    def _power_batch(self, t, y_batch, dy_batch, periods, table, params, median_kernel, with_arrays=False, with_power=False,
                     with_spectra=False, statistics=None, per_transit=False, models=None, lc_cap=0, peaks=None,
                     peak_fits=None, phase_scan=None):
        y, dy = numpy.asarray(y_batch, dtype=numpy.float64), numpy.asarray(dy_batch, dtype=numpy.float64)
        t, periods = numpy.asarray(t, dtype=numpy.float64), numpy.asarray(periods, dtype=numpy.float64)
        n_c, n_p = len(y), len(periods)
        self._note("_power_batch", n_c, 0, median_kernel=median_kernel, peaks=-1 if peaks is None else peaks[0],
                   peak_fits=peak_fits is not None, phase_scan=phase_scan is not None,
                   max_bins=-1 if phase_scan is None else phase_scan[0], min_count=-1 if phase_scan is None else phase_scan[1])
        sy, sdy = _row_sums(y), _row_sums(dy)
        duration = numpy.asarray(table.duration, dtype=numpy.float64)
        out = dict(summary=numpy.zeros(n_c, dtype=_lib.POWER_SUMMARY_DTYPE), chi2=None, row=None, depth=None, power=None,
                   SR=None, power_raw=None)
        pick = (numpy.floor(sy * 4096.0).astype(numpy.int64) % n_p)
        s = out["summary"]
        s["SDE"], s["SDE_raw"], s["chi2_min"] = 9.0 + (sy - numpy.floor(sy)), 8.0 + (sdy - numpy.floor(sdy)), 0.5 * sy
        s["period"], s["T0"], s["depth"] = periods[pick], t[0] + 0.25 * periods[pick], 0.99 - 1e-3 * (sy - numpy.floor(sy))
        s["index_best"], s["index_power"], s["best_row"], s["no_fit"] = pick, pick, pick % len(duration), 0
        if peaks is None:
            return out
        k = int(peaks[0])
        rank = numpy.arange(k)
        index = (pick[:, None] + 7 * rank[None, :]) % n_p
        found = numpy.broadcast_to(rank[None, :] < max(k - 1, 1), (n_c, k))       # (the last rank of every curve: no such peak)
        p = numpy.zeros((n_c, k), dtype=_lib.PEAK_DTYPE)
        frac = (sy - numpy.floor(sy))[:, None]
        p["period"] = numpy.where(found, periods[index], numpy.nan)
        p["power"] = numpy.where(found, 20.0 - rank[None, :] + frac, numpy.nan)
        p["chi2"] = numpy.where(found, sy[:, None] - rank[None, :], numpy.nan)
        p["depth"] = numpy.where(found, 0.995 - 1e-3 * rank[None, :] - 1e-3 * frac, numpy.nan)
        p["index"] = numpy.where(found, index, -1)
        p["row"] = numpy.where(found, index % len(duration), -1)
        out["peaks"], out["n_peaks"] = p, found.sum(axis=1).astype(numpy.int64)
        if peak_fits is None:
            return out
        # (status 2 -- the search fitted nothing at the index -- where the curve's sum says so: it depends on the curve alone)
        status = numpy.where(found, numpy.where((pick[:, None] + rank[None, :]) % 5 == 0, 2.0, 0.0), 1.0)
        live = status == 0
        base = _mix(p["period"], p["depth"], sy[:, None], sdy[:, None], rank[None, :] * 1.0)
        fits = _records(_lib.PEAK_FIT_DTYPE, base.reshape(-1), live=live.reshape(-1)).reshape(n_c, k)
        fits["status"] = status
        fits["T0"] = numpy.where(live, t[0] + (0.125 + 0.5 * frac) * p["period"], numpy.nan)
        # (durations from 0.05 to 0.35 days: some too short for the transit fit's window, every one a few samples wide)
        fits["duration_days"] = numpy.where(live, 0.05 + 0.3 * ((index % 7) / 6.0), numpy.nan)
        fits["depth_mean"] = numpy.where(live, 1.0 - p["depth"], numpy.nan)
        fits["transit_count"] = numpy.where(live, 3.0 + rank[None, :], numpy.nan)
        out["peak_fits"] = fits
        if phase_scan is not None:
            scan_base = _mix(p["period"], fits["T0"], fits["duration_days"], sy[:, None], float(phase_scan[0]), float(phase_scan[1]))
            scans = _records(_lib.PHASE_SCAN_DTYPE, scan_base.reshape(-1), live=live.reshape(-1)).reshape(n_c, k)
            scans["secondary_phase"] = numpy.where(live, 0.25 + 0.5 * frac, numpy.nan)
            scans["scan_std"] = numpy.where(live, numpy.where(rank[None, :] == 0, 0.0, 1.5 + frac), numpy.nan)
            out["phase_scans"] = scans
        return out

    def _candidates(self, y, curve, period, *more):
        """(base, live) of the candidates: their own arguments mixed with the sum of their curve's row."""
        sy = _row_sums(y)
        period = numpy.asarray(period, dtype=numpy.float64)
        curve = numpy.arange(len(period)) if curve is None else numpy.asarray(curve)
        return _mix(period, sy[curve], *more), numpy.isfinite(period)

    def transit_times(self, t, y, dy, period, T0, row, reach, widths, shapes, span_max, curve=None, depth_min=0.0,
                      min_ses=3.0, max_epochs=1):
        self._note("transit_times", len(y), len(period), depth_min=depth_min, min_ses=min_ses, max_epochs=max_epochs)
        row = numpy.asarray(row)
        template = numpy.array([math.fsum(s) for s in shapes])[row]
        base, live = self._candidates(y, curve, period, T0, row, reach, numpy.asarray(widths)[row],
                                      numpy.asarray(span_max, dtype=numpy.float64)[row], template, _row_sums(dy)[curve],
                                      depth_min, min_ses)
        return (_records(_lib.EPHEMERIS_DTYPE, base, live=live),
                _records(_lib.TRANSIT_TIME_DTYPE, base, shape=(int(max_epochs),), live=live))

    def event_vetting(self, t, y, dy, period, T0, row, reach, chase_reach, guard, chase_span, widths, shapes, span_max,
                      curve=None, depth_min=0.0, min_ses=3.0, chase_fraction=0.6, chase_min=0.5, point_fraction=0.5,
                      step_fraction=0.5, max_epochs=1):
        self._note("event_vetting", len(y), len(period), depth_min=depth_min, min_ses=min_ses, chase_fraction=chase_fraction,
                   chase_min=chase_min, point_fraction=point_fraction, step_fraction=step_fraction, max_epochs=max_epochs)
        row = numpy.asarray(row)
        template = numpy.array([math.fsum(s) for s in shapes])[row]
        base, live = self._candidates(y, curve, period, T0, row, reach, chase_reach, guard, chase_span,
                                      numpy.asarray(widths)[row], numpy.asarray(span_max, dtype=numpy.float64)[row], template,
                                      _row_sums(dy)[curve], depth_min, min_ses, chase_fraction, chase_min, point_fraction,
                                      step_fraction)
        return (_records(_lib.EVENT_SUMMARY_DTYPE, base, live=live),
                _records(_lib.EVENT_RECORD_DTYPE, base, shape=(int(max_epochs),), live=live))

    def shape_fit(self, t, y, dy, period, T0, duration, ratios, ingress, shifts, curve=None, window=2.0, min_count=3,
                  depth_min=0.0):
        self._note("shape_fit", len(y), len(period), window=window, min_count=min_count, depth_min=depth_min,
                   tables=len(ratios) * len(ingress) * len(shifts))
        base, live = self._candidates(y, curve, period, T0, duration, _row_sums(dy)[curve], window, min_count, depth_min,
                                      math.fsum(ratios), math.fsum(ingress), math.fsum(shifts))
        out = _records(_lib.SHAPE_DTYPE, base, live=live)
        frac = base - numpy.floor(base)
        out["depth"], out["ingress"] = numpy.where(live, 1e-3 + 1e-2 * frac, numpy.nan), numpy.where(live, 0.5 * frac, numpy.nan)
        out["duration"] = numpy.where(live, numpy.asarray(duration) * (0.9 + 0.2 * frac), numpy.nan)
        return out

    def centroid_test(self, t, y, cx, cy, period, T0, duration, shape, curve=None, window=3.0, min_in=1, min_out=3,
                      max_epochs=_lib.CENTROID_MAX_EPOCHS):
        self._note("centroid_test", len(y), len(period), window=window, min_in=min_in, min_out=min_out, max_epochs=max_epochs)
        base, live = self._candidates(y, curve, period, T0, duration, _row_sums(cx)[curve], _row_sums(cy)[curve],
                                      math.fsum(shape), window, min_in, min_out, max_epochs)
        out = _records(_lib.CENTROID_DTYPE, base, live=live)
        out["depth"] = numpy.where(live, 1e-3 + 1e-2 * (base - numpy.floor(base)), numpy.nan)
        return out

    def folded_views(self, t, y, period, T0, duration, curve=None, secondary_phase=None, n_global=2001, n_local=201,
                     local_durations=4.0, local_width=0.16):
        self._note("folded_views", len(y), len(period), secondary=secondary_phase is not None, n_global=n_global,
                   n_local=n_local, local_durations=local_durations, local_width=local_width)
        phase = numpy.full(len(period), -2.0) if secondary_phase is None else secondary_phase
        base, live = self._candidates(y, curve, period, T0, duration, phase, local_durations, local_width)
        g_med = base[:, None] + numpy.arange(int(n_global), dtype=numpy.float64)
        l_med = base[:, None, None] * numpy.array([2.0, 3.0, 5.0, 7.0])[None, :, None] + numpy.arange(int(n_local), dtype=numpy.float64)
        dead = ~live
        g_med[dead], l_med[dead] = numpy.nan, numpy.nan
        g_cnt = numpy.where(dead[:, None], 0, 1 + numpy.arange(int(n_global))[None, :]).astype(numpy.int32)
        l_cnt = numpy.where(dead[:, None, None], 0, 2 + numpy.arange(4)[None, :, None]
                            + numpy.arange(int(n_local))[None, None, :]).astype(numpy.int32)
        return _records(_lib.VIEWS_DTYPE, base, live=live), g_med, g_cnt, l_med, l_cnt

    def sine_test(self, t, y, period, curve=None, dy=None, T0=None, duration=None, mask=1.5, harmonics=(0.5, 1.0, 2.0),
                  debug=False):
        self._note("sine_test", len(y), len(period), weighted=dy is not None, mask=mask, harmonics=len(harmonics),
                   harmonic_sum=math.fsum(harmonics))
        weight = numpy.full(len(period), -3.0) if dy is None else _row_sums(dy)[curve]
        base, live = self._candidates(y, curve, period, T0, duration, weight, mask, math.fsum(harmonics))
        return (_records(_lib.SINE_DTYPE, base, live=live),
                _records(_lib.SINE_HARMONIC_DTYPE, base, shape=(len(harmonics),), live=live, first=0.5))

    def ephemeris_match(self, star, period, T0, duration, strength, span, drift_tolerance=0.5, epoch_tolerance=0.5,
                        max_ratio=3):
        star = numpy.asarray(star)
        self._note("ephemeris_match", 0, len(star), span=span, drift_tolerance=drift_tolerance,
                   epoch_tolerance=epoch_tolerance, max_ratio=max_ratio)
        base = _mix(star * 1.0, period, T0, duration, strength, span, drift_tolerance, epoch_tolerance, max_ratio)
        out = _records(_lib.MATCH_DTYPE, base)
        m = len(star)
        # (the first candidate of the next star, of the first star behind the last; -1 for every third candidate and for a
        # lone star: the pipeline's candidates come star by star)
        assert numpy.all(star[1:] >= star[:-1])
        if m:
            best = numpy.searchsorted(star, star, side="right")
            best = numpy.where(best == m, 0, best)
            best = numpy.where((star[best] == star) | (numpy.arange(m) % 3 == 2), -1, best)
            out["best"] = best
        return out

    def noise_profile(self, t, y, widths, span_max, pair_span, clip_upper=5.0, clip_lower=5.0, min_count=3):
        self._note("noise_profile", len(y), 0, widths=len(widths), pair_span=pair_span, clip_upper=clip_upper,
                   clip_lower=clip_lower, min_count=min_count, span_sum=math.fsum(span_max))
        sy = _row_sums(y)
        base = _mix(sy, pair_span, clip_upper, clip_lower, min_count)
        w = numpy.asarray(widths, dtype=numpy.float64)
        records = _records(_lib.NOISE_CURVE_DTYPE, base)
        records["sigma"] = 1e-3 * (1.0 + (sy - numpy.floor(sy)))
        robust = records["sigma"][:, None] / numpy.sqrt(w)[None, :] * (1.0 + numpy.asarray(span_max)[None, :])
        robust[::2, min(1, len(w) - 1)] = numpy.nan           # (every other curve: too few windows at one width)
        count = (numpy.floor(sy)[:, None] + w[None, :]).astype(numpy.int64)
        return records, count, robust, robust * 1.25

    def transit_fit(self, t, y, dy, period, T0, duration, row_first, k_rows, profile, impacts, ratios, shifts, sub, curve=None,
                    window=1.0, min_count=3, delta=1.0):
        self._note("transit_fit", len(y), len(period), window=window, min_count=min_count, delta=delta,
                   tables=len(k_rows) * len(impacts) * len(ratios) * len(shifts), sub=len(sub), sub_sum=math.fsum(sub))
        table = math.fsum(numpy.asarray(profile, dtype=numpy.float64).reshape(-1))
        base, live = self._candidates(y, curve, period, T0, duration, row_first, _row_sums(dy)[curve], table,
                                      math.fsum(k_rows), math.fsum(impacts), math.fsum(ratios), math.fsum(shifts),
                                      math.fsum(sub), window, min_count, delta)
        out = _records(_lib.TRANSIT_FIT_DTYPE, base, live=live)
        frac = base - numpy.floor(base)
        out["k"], out["b"] = numpy.where(live, 0.02 + 0.1 * frac, numpy.nan), numpy.where(live, 0.9 * frac, numpy.nan)
        out["duration"] = numpy.where(live, numpy.asarray(duration) * (0.9 + 0.2 * frac), numpy.nan)
        out["shift"] = numpy.where(live, 0.01 * (frac - 0.5), numpy.nan)
        return out


class FakeGroup(object):
    """What survey._on_devices and survey._first_context ask of a DeviceGroup: two contexts that share one log, a lock, and
    _threads -- here one slice after the other, so that the log has one order."""

    def __init__(self, n=2):
        self.log = []
        self.contexts = [FakeContext("ctx%d" % r, self.log) for r in range(n)]
        self._lock = threading.Lock()

    def _threads(self, work):
        for r in range(len(self.contexts)):
            work(r)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
N_POINTS, N_PEAKS = 400, 3
KW = dict(period_min=2.0, period_max=3.0, oversampling_factor=2)
STAGES = ("transit_times", "shape_fit", "sine_test", "ephemeris_match", "views", "event_vetting", "centroids", "noise",
          "transit_fit")
# (every stage with an option that is not its default, so that a swapped option shows; the smallest view tables there are)
OPTIONS = dict(
    phase_scan=dict(phase_scan=True, phase_scan_max_bins=512, phase_scan_min_count=2),
    transit_times=dict(transit_times=True, transit_times_search=1.5, transit_times_min_ses=2.5),
    shape_fit=dict(shape_fit=True, shape_fit_window=2.5, shape_fit_min_count=4),
    sine_test=dict(sine_test=True, sine_test_mask=1.25, sine_test_harmonics=(0.5, 1.0, 2.0, 3.0)),
    ephemeris_match=dict(ephemeris_match=True, ephemeris_match_drift=0.75, ephemeris_match_epoch=0.25,
                         ephemeris_match_max_ratio=4),
    views=dict(views=True, views_global_bins=2, views_local_bins=2, views_local_durations=3.0, views_local_width=0.25),
    event_vetting=dict(event_vetting=True, event_vetting_search=1.25, event_vetting_chase_window=0.2, event_vetting_guard=2.0,
                       event_vetting_min_ses=2.0, event_vetting_chase_fraction=0.7, event_vetting_chase_min=0.4,
                       event_vetting_point_fraction=0.6, event_vetting_step_fraction=0.3),
    centroids=dict(centroid_window=3.5, centroid_min_in=2, centroid_min_out=4),
    noise=dict(noise=True),
    transit_fit=dict(transit_fit=dict(window=0.9, n_sub=3)),
)


def batch(n_curves, n_points=N_POINTS):
    """(t, flux, dy, cx, cy): rows whose values are small multiples of 2^-20, so that no sum of theirs depends on its order."""
    rng = numpy.random.default_rng(20)
    t = numpy.linspace(1.0, 21.0, n_points)
    flux = 1.0 + rng.integers(-512, 512, size=(n_curves, n_points)) / 2.0 ** 20
    dy = numpy.full((n_curves, n_points), 2.0 ** -10)
    cx = 5.0 + rng.integers(-512, 512, size=(n_curves, n_points)) / 2.0 ** 12
    cy = 7.0 + rng.integers(-512, 512, size=(n_curves, n_points)) / 2.0 ** 12
    return t, flux, dy, cx, cy


def stage_keywords(names, cx, cy):
    """power_batch's keywords for the stages `names` (and "phase_scan") with OPTIONS."""
    kw = {}
    for name in names:
        kw.update(OPTIONS[name])
        if name == "centroids":
            kw["centroids"] = (cx, cy)
    return kw


def run(survey, n_curves, names, context=None, dy=True, n_points=N_POINTS, peaks=N_PEAKS):
    """(summary, found, log) of power_batch(peaks, peak_fits=True) with the stages `names` on the batch of n_curves, on a
    new FakeContext (or the given one; a FakeGroup's log is its own)."""
    t, flux, dy_batch, cx, cy = batch(n_curves, n_points)
    ctx = FakeContext() if context is None else context
    out = survey.power_batch(t, flux, dy_batch if dy else None, context=ctx, peaks=peaks, peak_fits=True,
                             **dict(stage_keywords(names, cx, cy), **KW))
    return out[0], out[-1], ctx.log


def flatten(prefix, summary, found):
    """The arrays of a result under flat names: the summary's and the peaks' bytes and dtypes, every extra array."""
    out = {prefix + "summary": numpy.frombuffer(summary.tobytes(), dtype=numpy.uint8),
           prefix + "summary_dtype": numpy.array(json.dumps(summary.dtype.descr)),
           prefix + "peaks": numpy.frombuffer(numpy.ascontiguousarray(found["peaks"]).tobytes(), dtype=numpy.uint8),
           prefix + "peaks_dtype": numpy.array(json.dumps(found["peaks"].dtype.descr)),
           prefix + "peaks_shape": numpy.array(found["peaks"].shape)}
    for key, value in found.items():
        if key == "peaks":
            continue
        for sub, v in (value.items() if isinstance(value, dict) else [(None, value)]):
            name = prefix + key + ("" if sub is None else "." + sub)
            v = numpy.ascontiguousarray(v)
            if v.dtype.names:
                out[name + "_dtype"] = numpy.array(json.dumps(v.dtype.descr))
                out[name + "_shape"] = numpy.array(v.shape)
                v = numpy.frombuffer(v.tobytes(), dtype=numpy.uint8)
            out[name] = v
    return out


ALL = ("phase_scan",) + STAGES


def field_bytes(records, names):
    """The bytes of the fields `names` of a structured array, field by field."""
    return numpy.frombuffer(b"".join(numpy.ascontiguousarray(records[k]).tobytes() for k in names), dtype=numpy.uint8)


def golden(survey):
    """What tests/golden/peak_stages_host.npz records: the all-on call on 3 curves, the same on 5 curves over two slices
    (survey._resolve replaced by a two-context FakeGroup), the sine test alone without a dy_batch, and power_batch's
    signature."""
    import inspect
    out = {}
    summary, found, log = run(survey, 3, ALL)
    out.update(flatten("one.", summary, found))
    out["one.log"] = numpy.array(json.dumps(log))
    group = FakeGroup()
    resolve = survey._resolve
    survey._resolve = lambda devices, device, context, n_curves: ("group", group)
    try:
        t, flux, dy, cx, cy = batch(5)
        res = survey.power_batch(t, flux, dy, devices=[0, 1], peaks=N_PEAKS, peak_fits=True,
                                 **dict(stage_keywords(ALL, cx, cy), **KW))
    finally:
        survey._resolve = resolve
    out.update(flatten("two.", res[0], res[-1]))
    out["two.log"] = numpy.array(json.dumps(group.log))
    summary, found, log = run(survey, 3, ("sine_test",), dy=False)
    out["nody.sine"] = field_bytes(found["peaks"], [k for k in found["peaks"].dtype.names if k.startswith("sine_")])
    out["nody.log"] = numpy.array(json.dumps([c for c in log if c[1] == "sine_test"]))
    sig = inspect.signature(survey.power_batch)
    out["signature"] = numpy.array(json.dumps([[k, repr(p.default), str(p.kind)] for k, p in sig.parameters.items()]))
    return out
