"""ctypes binding of libtls_amd.so -- the C ABI declared in include/tls_amd.h.

Thin by design: numpy arrays in, numpy arrays out, every non-zero return code
raised as RuntimeError with the library's message.  No torch, no fallback: if the
shared library is missing, or no GPU is usable, the error surfaces here.
"""
import ctypes
import operator
import os
import weakref

import numpy

from . import _checks

_HERE = os.path.dirname(os.path.abspath(__file__))
# Developer switch for A/B timing of two builds of the same source (tls_amd/csrc/Makefile `variant`, `debug`): another
# library is loaded only when TLS_AMD_DEBUG=1 says this is a developer session AND TLS_AMD_LIB names it -- a stray
# TLS_AMD_LIB in a user's environment does not redirect the product.
LIB_PATH = os.path.join(_HERE, "libtls_amd.so")
if os.environ.get("TLS_AMD_DEBUG") == "1" and os.environ.get("TLS_AMD_LIB"):
    LIB_PATH = os.environ["TLS_AMD_LIB"]
ABI_VERSION = 8   # include/tls_amd.h TLS_AMD_ABI_VERSION: checked against the library at load time
MEDFILT_MAX_KERNEL = 4095   # include/tls_amd.h TLS_MEDFILT_MAX_KERNEL: the largest kernel size tls_medfilt_detrend takes
# include/tls_amd.h TLS_BIWEIGHT_*: the most points of one window of tls_biweight_detrend, and the estimator's fixed constants
BIWEIGHT_MAX_WINDOW = 4095
BIWEIGHT_C = 5.0
BIWEIGHT_FTOL = 1e-6
BIWEIGHT_MAX_ITER = 50
# include/tls_amd.h TLS_SYSREM_*: the lanes of a row sum and the rows of a column sum's chunk (both part of tls_sysrem's
# definition), the most components and the most iterations per component
SYSREM_LANES = 256
SYSREM_ROW_CHUNK = 32
SYSREM_MAX_COMPONENTS = 8
SYSREM_MAX_ITER = 1000
# include/tls_amd.h TLS_PEAKS_*: the most peaks per row and the most harmonic ratios tls_find_peaks takes
PEAKS_MAX_K = 32
PEAKS_MAX_RATIOS = 16
# include/tls_amd.h TLS_PHASE_SCAN_*: the range of max_bins of the phase scan
PHASE_SCAN_MIN_BINS = 16
PHASE_SCAN_MAX_BINS = 4096
PHASE_SCAN_CHUNK = 2048   # tls_phase_scan.hip.h kPhaseChunk: the points of a light curve the scan stages in LDS at a time
# include/tls_amd.h TLS_SINGLE_*: the widest row and the most events a curve of tls_single_transits; tls_single.hip.h
# kSingleMinWidth, kSingleTile (the centres of a workgroup of the statistic kernel) and kSingleMaxPoints
SINGLE_MAX_WIDTH = 4096
SINGLE_MAX_K = 32
SINGLE_MIN_WIDTH = 3
SINGLE_TILE = 256
SINGLE_MAX_POINTS = 1 << 20
# include/tls_amd.h TLS_TIMES_*: the widest reach and the most epochs a candidate of tls_transit_times
TIMES_MAX_REACH = 4096
TIMES_MAX_EPOCHS = 65536
TIMES_MAX_POINTS = 1 << 30   # tls_times.hip.h kTimesMaxPoints
EVENTS_MAX_CHASE = 8192      # include/tls_amd.h TLS_EVENTS_MAX_CHASE: the widest chase reach of a candidate of tls_event_vetting
# include/tls_amd.h TLS_ALIAS_MAX: the most aliases of a pair of tls_event_periods; tls_aliases.hip.h kAliasTile (the centres of a
# workgroup of the plane kernel), kAliasLdsPoints (a longer series is read from device memory, not from the LDS) and
# kAliasMaxPoints
ALIAS_MAX = 4096
ALIAS_TILE = 256
ALIAS_LDS_POINTS = 6400
ALIAS_MAX_POINTS = 1 << 20
# include/tls_amd.h TLS_SHAPE_MAX_UNITS: the most (duration, ingress, shift) units of tls_shape_fit; tls_shape.hip.h
# kShapeMaxPoints and kShapeLdsMembers (the members of a candidate the LDS holds; more are staged through it in tiles)
SHAPE_MAX_UNITS = 65536
SHAPE_MAX_POINTS = 1 << 22
SHAPE_LDS_MEMBERS = 2048
# include/tls_amd.h TLS_CENTROID_MAX_EPOCHS, TLS_CENTROID_MAX_SHAPE: the most epochs of a candidate of tls_centroid_test and
# the most samples of its shape; tls_centroid.hip.h kCentroidMaxPoints, kCentroidThreads and kCentroidLdsEpochs (the epochs of
# a candidate the LDS holds; later ones keep their sums in device scratch); CENTROID_SHAPE_SAMPLES: the samples
# survey.centroid_test takes of the reference transit
CENTROID_MAX_EPOCHS = 65536
CENTROID_MAX_SHAPE = 1 << 20
CENTROID_MAX_POINTS = 1 << 22
CENTROID_THREADS = 256
CENTROID_LDS_EPOCHS = 256
CENTROID_SHAPE_SAMPLES = 1025
# include/tls_amd.h TLS_VIEWS_MAX_BINS: the most bins of a view of tls_folded_views; tls_views.hip.h kViewsMaxPoints,
# kViewsLdsPoints (the points of a series the LDS holds; a longer one is ordered in device scratch), kViewsLaneMembers (a bin
# of up to this many members is selected by one lane, a larger one by a wave) and kViewsSlab (the candidates of a launch)
VIEWS_MAX_BINS = 65536
VIEWS_MAX_POINTS = 1 << 20
VIEWS_LDS_POINTS = 4608
VIEWS_LANE_MEMBERS = 8
VIEWS_SLAB = 1024
# include/tls_amd.h TLS_GLS_MAX_POINTS, TLS_GLS_MAX_FREQUENCIES, TLS_SINE_MAX_HARMONICS; tls_gls.hip.h kGlsRowTile,
# kGlsSmallRows (batches of at most this many rows take the 32-row kernel), kGlsFreqTile, kGlsChunk, kSineThreads
GLS_MAX_POINTS = 1 << 22
GLS_MAX_FREQUENCIES = 1 << 24
GLS_ROW_TILE = 128
GLS_SMALL_ROWS = 32
GLS_FREQ_TILE = 64
GLS_CHUNK = 32
SINE_MAX_HARMONICS = 8
SINE_LANES = 256
# include/tls_amd.h TLS_PREWHITEN_MAX_TERMS, TLS_PREWHITEN_LDS_POINTS (a row of at most this many points is fitted in the LDS)
PREWHITEN_MAX_TERMS = 32
PREWHITEN_LDS_POINTS = 6144
# include/tls_amd.h TLS_MATCH_*: the most candidates and the largest max_ratio of tls_ephemeris_match; tls_match.hip.h
# kMatchTile (the candidates of a workgroup, and of a staged tile of the other side), kMatchTargetGroups and kMatchMaxChunks
# (match_chunks below)
MATCH_MAX_CANDIDATES = 1 << 20
MATCH_MAX_RATIO = 64
MATCH_TILE = 256
MATCH_TARGET_GROUPS = 1024
MATCH_MAX_CHUNKS = 16
# include/tls_amd.h TLS_NOISE_*: the widest window, the most widths and the longest row of tls_noise_profile, and the points
# of a row the LDS holds (a longer one is measured in device scratch); tls_noise.hip.h kNoiseThreads
NOISE_MAX_WIDTH = 4096
NOISE_MAX_WIDTHS = 64
NOISE_MAX_POINTS = 1 << 22
NOISE_LDS_POINTS = 8192
NOISE_THREADS = 256
# include/tls_amd.h TLS_DECOR_*: the most columns and clip rounds of tls_decorrelate, the pivot below which a column counts as
# collinear, and the points of a segment whose membership mask the LDS holds (a longer one keeps it in device scratch)
DECOR_MAX_TERMS = 16
DECOR_MAX_ITER = 16
DECOR_PIVOT = 1e-10
DECOR_LDS_POINTS = 32768
# include/tls_amd.h TLS_SPLINE_*: the most knot spacings and clip rounds of tls_spline_detrend, the most coefficients of one
# segment (the band the LDS holds), the points of the longest segment a call keeps in the LDS (a longer one runs on device
# scratch), and the pivot below which the band counts as singular
SPLINE_MAX_SPACINGS = 16
SPLINE_MAX_ITER = 16
SPLINE_MAX_COEF = 512
SPLINE_LDS_POINTS = 5120
SPLINE_PIVOT = 1e-10
# include/tls_amd.h TLS_CLEAN_*: the most clip rounds of tls_clean_rows, and the points of a row whose residuals a round keeps
# in the LDS (the noise profile's selection: NOISE_LDS_POINTS; a longer row runs on device memory)
CLEAN_MAX_ITER = 16
CLEAN_LDS_POINTS = 8192
PEAKS_LDS_PERIODS = 1 << 20   # tls_peaks.hip.h kPeaksLdsPeriods: a longer grid keeps its alive mask in device memory, not in LDS

# every symbol include/tls_amd.h declares (tests check the export list against the header)
SYMBOLS = (
    "tls_device_count", "tls_ctx_create", "tls_ctx_destroy", "tls_last_error", "tls_version", "tls_abi_version",
    "tls_device_name", "tls_get_options", "tls_set_options", "tls_debug_set_switch", "tls_debug_get_switches", "tls_search", "tls_search_batch", "tls_power_batch", "tls_prepare", "tls_update_flux", "tls_execute",
    "tls_synchronize", "tls_fetch", "tls_execute_timed", "tls_plan_info", "tls_last_kernel", "tls_grid_cells", "tls_period_costs", "tls_debug_candidate_slabs", "tls_t0_fit", "tls_pink_noise", "tls_spectra", "tls_kernel_timing", "tls_debug_phase_cycles", "tls_debug_cumsum", "tls_debug_folded", "tls_debug_prefix", "tls_debug_check_counts", "tls_debug_poison_lds", "tls_debug_period_cycles", "tls_debug_batch_group_ms",
    "tls_debug_post_search", "tls_debug_device_bytes", "tls_debug_perm_table", "tls_debug_lanes", "tls_debug_launch_ms", "tls_power_batch_stats", "tls_debug_transit_stats",
    "tls_power_batch_models", "tls_debug_transit_models",
    "tls_inject_transits", "tls_null_rows", "tls_debug_null_words", "tls_medfilt_detrend",
    "tls_biweight_detrend", "tls_sysrem", "tls_find_peaks", "tls_power_batch_peaks", "tls_power_batch_peak_fits", "tls_debug_peak_fits",
    "tls_phase_scan", "tls_power_batch_phase_scan", "tls_debug_peak_phase_scans", "tls_single_transits",
    "tls_transit_times", "tls_shape_fit", "tls_nudft", "tls_lomb_scargle", "tls_sine_test", "tls_prewhiten",
    "tls_ephemeris_match", "tls_folded_views", "tls_event_vetting", "tls_centroid_test", "tls_noise_profile",
    "tls_transit_fit",
    "tls_transit_mask", "tls_biweight_detrend_masked", "tls_prewhiten_masked",
    "tls_remove_transits", "tls_event_periods", "tls_decorrelate", "tls_spline_detrend", "tls_clean_rows",
    "tls_comm_unique_id", "tls_comm_init", "tls_comm_destroy", "tls_comm_info", "tls_comm_allgather_results", "tls_comm_allgather_device", "tls_comm_fetch_gathered",
    "tls_comm_stage_results", "tls_comm_allgather_staged", "tls_comm_fetch_staged",
    "tls_comm_barrier", "tls_comm_max",
)

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int64_p = ctypes.POINTER(ctypes.c_int64)


class _Template(ctypes.Structure):
    _fields_ = [("values", _c_double_p), ("offset", _c_int64_p), ("length", _c_int64_p),
                ("width", _c_int64_p), ("overshoot", _c_double_p), ("n_rows", ctypes.c_int64)]


class _Params(ctypes.Structure):
    _fields_ = [("transit_depth_min", ctypes.c_double), ("R_star_min", ctypes.c_double),
                ("R_star_max", ctypes.c_double), ("M_star_min", ctypes.c_double),
                ("M_star_max", ctypes.c_double), ("T0_fit_margin", ctypes.c_double)]


class Options(ctypes.Structure):
    """tls_options: the two switches of a context a caller may set (include/tls_amd.h).  -1 = the library decides."""
    _fields_ = [("exact_prefix", ctypes.c_int32), ("slim", ctypes.c_int32)]

    NAMES = ("exact_prefix", "slim")


# every switch tls_debug_set_switch knows (the two public ones included): Context.set_options(**switches) takes them all
SWITCH_NAMES = ("exact_prefix", "slim", "prune", "screen32", "no_screen", "fast_slab", "x_staged", "split", "split_batch", "sort2",
                "threads", "blocks", "plan_threads", "t0_rot", "prune_min_live", "perm_table", "reg_scan", "dense_hoist",
                "claim_ahead", "band_max", "lanes")


def switches_text(switches):
    """"name=value,..." (what tls_period_costs and tls_debug_get_switches speak) from a dict; None values are left out."""
    unknown = set(switches or {}) - set(SWITCH_NAMES)
    if unknown:
        raise TypeError("unknown switches %s" % sorted(unknown))
    return ",".join("%s=%.17g" % (k, float(v)) for k, v in sorted((switches or {}).items()) if v is not None)


class PowerSummary(ctypes.Structure):
    """tls_power_summary: what main.py:198-283 derives from the search results of one light curve."""
    _fields_ = [("SDE", ctypes.c_double), ("SDE_raw", ctypes.c_double), ("chi2_min", ctypes.c_double),
                ("period", ctypes.c_double), ("T0", ctypes.c_double), ("depth", ctypes.c_double),
                ("index_best", ctypes.c_int64), ("index_power", ctypes.c_int64), ("best_row", ctypes.c_int64),
                ("no_fit", ctypes.c_int64)]


POWER_SUMMARY_DTYPE = numpy.dtype([("SDE", "f8"), ("SDE_raw", "f8"), ("chi2_min", "f8"), ("period", "f8"), ("T0", "f8"),
                                   ("depth", "f8"), ("index_best", "i8"), ("index_power", "i8"), ("best_row", "i8"),
                                   ("no_fit", "i8")])


TRANSIT_STATS_FIELDS = ("period_uncertainty", "duration_days", "depth_mean", "depth_mean_std", "depth_mean_even",
                        "depth_mean_even_std", "depth_mean_odd", "depth_mean_odd_std", "snr", "odd_even_mismatch",
                        "transit_count", "distinct_transit_count", "empty_transit_count", "in_transit_count",
                        "after_transit_count", "before_transit_count")


class TransitStats(ctypes.Structure):
    """tls_transit_stats: the per-transit vetting statistics of power() (api.py:175-241) for one light curve."""
    _fields_ = [(k, ctypes.c_double) for k in TRANSIT_STATS_FIELDS]


TRANSIT_STATS_DTYPE = numpy.dtype([(k, "f8") for k in TRANSIT_STATS_FIELDS])
# rows of the per-transit output [n_curves][6][max_epochs]
PER_TRANSIT_FIELDS = ("transit_times", "per_transit_count", "transit_depths", "transit_depths_uncertainties",
                      "snr_per_transit", "snr_pink_per_transit")
# rows of the folded output [n_curves][3][n] and of the model light curve output [n_curves][2][lc_cap]
FOLDED_FIELDS = ("folded_phase", "folded_y", "order")
LIGHTCURVE_FIELDS = ("model_lightcurve_time", "model_lightcurve_model")


class ModelTemplate(object):
    """What tls_power_batch_models needs of the template shape: the in-transit slice of the supersampled curve
    (template.py:52-53) and the ends of reference_transit's linspace; maxw = int(max(durations) * n) (api.py:140)."""

    def __init__(self, curve_t, curve_f, lo, hi, maxw):
        self.curve_t, self.curve_f = _f8(curve_t), _f8(curve_f)
        self.lo, self.hi, self.maxw = float(lo), float(hi), float(maxw)

    def args(self, lc_cap, out):
        folded, model, lc, lc_len = out
        return [_dp(self.curve_t), _dp(self.curve_f), len(self.curve_t), self.lo, self.hi, self.maxw, int(lc_cap),
                _dp(folded), _dp(model), _dp(lc), _ip(lc_len)]


# the per-period arrays of the power-batch entries, in the order of their C arguments, and the arrays of the models stage
PER_PERIOD_OUTPUTS = ("chi2", "row", "depth", "power", "SR", "power_raw")
MODEL_OUTPUTS = ("folded", "model_folded", "lightcurve", "lc_len")


def _model_outputs(n_c, n, lc_cap):
    return (numpy.empty((n_c, len(FOLDED_FIELDS), n)), numpy.empty((n_c, n)),
            numpy.empty((n_c, len(LIGHTCURVE_FIELDS), int(lc_cap))), numpy.empty(n_c, dtype=numpy.int64))


class Peak(ctypes.Structure):
    """tls_peak: one peak of a periodogram (include/tls_amd.h), 48 bytes."""
    _fields_ = [("period", ctypes.c_double), ("power", ctypes.c_double), ("chi2", ctypes.c_double),
                ("depth", ctypes.c_double), ("index", ctypes.c_int64), ("row", ctypes.c_int64)]


PEAK_DTYPE = numpy.dtype([("period", "f8"), ("power", "f8"), ("chi2", "f8"), ("depth", "f8"), ("index", "i8"), ("row", "i8")])


class PeakFit(ctypes.Structure):
    """tls_peak_fit: the final T0 fit and the statistics record of one peak (include/tls_amd.h), 18 doubles."""
    _fields_ = [("T0", ctypes.c_double), ("status", ctypes.c_double), ("stats", TransitStats)]


PEAK_FIT_DTYPE = numpy.dtype([("T0", "f8"), ("status", "f8")] + [(k, "f8") for k in TRANSIT_STATS_FIELDS])
# tls_peak_fit.status
PEAK_FITTED, PEAK_NONE, PEAK_UNFITTED = 0, 1, 2


# tls_phase_record (include/tls_amd.h): the phase scan of one candidate, 12 doubles
PHASE_SCAN_FIELDS = ("status", "n_bins", "n_windows", "primary_depth", "primary_count", "secondary_depth", "secondary_phase",
                     "secondary_count", "bump_depth", "bump_phase", "scan_mean", "scan_std")


class PhaseRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in PHASE_SCAN_FIELDS]


PHASE_SCAN_DTYPE = numpy.dtype([(k, "f8") for k in PHASE_SCAN_FIELDS])
# tls_phase_record.status
PHASE_SCANNED, PHASE_NOTHING = 0, 1


def phase_scan_arguments(max_bins, min_count):
    """(max_bins, min_count) as the phase scan takes them, checked as tls_phase_scan checks them: max_bins an integer in
    [PHASE_SCAN_MIN_BINS, PHASE_SCAN_MAX_BINS], min_count an integer >= 1; ValueError otherwise."""
    what = "phase scan"
    for name, v in (("max_bins", max_bins), ("min_count", min_count)):
        _checks.integer(what, name, v)
    return (_checks.integer(what, "max_bins", max_bins, PHASE_SCAN_MIN_BINS, PHASE_SCAN_MAX_BINS,
                            "must be in [%d, %d]" % (PHASE_SCAN_MIN_BINS, PHASE_SCAN_MAX_BINS)),
            _checks.integer(what, "min_count", min_count, 1, 2 ** 31 - 1, "must be at least 1"))


# tls_match_record (include/tls_amd.h): the ephemeris match of one candidate, 10 doubles
MATCH_FIELDS = ("status", "n_same", "n_period", "n_match", "best", "best_ratio", "best_dt", "best_drift", "best_strength", "child")


class MatchRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in MATCH_FIELDS]


MATCH_DTYPE = numpy.dtype([(k, "f8") for k in MATCH_FIELDS])
# tls_match_record.status
MATCH_MATCHED, MATCH_BAD = 0, 1


def match_chunks(n):
    """The first candidate of every chunk of the g range tls_ephemeris_match cuts n candidates into, and n at the end
    (tls_match.hip.h match_chunks): whole tiles of MATCH_TILE, enough chunks to reach MATCH_TARGET_GROUPS workgroups, at most
    MATCH_MAX_CHUNKS and at most one a tile; chunk c holds the tiles [c * tiles // chunks, (c + 1) * tiles // chunks)."""
    n = int(n)
    tiles = -(-n // MATCH_TILE)
    if tiles == 0:
        return [0]
    chunks = min(-(-MATCH_TARGET_GROUPS // tiles), tiles, MATCH_MAX_CHUNKS)
    return [min(n, MATCH_TILE * (c * tiles // chunks)) for c in range(chunks)] + [n]


def ephemeris_match_arguments(star, period, T0, duration, strength, span, drift_tolerance=0.5, epoch_tolerance=0.5, max_ratio=3):
    """What tls_ephemeris_match takes, checked as it checks them: a dict with star (int64 [M], any values), period, T0,
    duration and strength (float64 [M], any values: a bad candidate gets status 1), M <= MATCH_MAX_CANDIDATES, span finite
    and > 0, drift_tolerance and epoch_tolerance finite and >= 0, max_ratio an integer in [1, MATCH_MAX_RATIO].  ValueError
    otherwise.  GPU-free."""
    what = "ephemeris match"
    for name, v in (("span", span), ("drift_tolerance", drift_tolerance), ("epoch_tolerance", epoch_tolerance)):
        _checks.real(what, name, v)
    span = _checks.finite_positive(what, "span", span)
    drift_tolerance = _checks.finite_at_least(what, "drift_tolerance", drift_tolerance)
    epoch_tolerance = _checks.finite_at_least(what, "epoch_tolerance", epoch_tolerance)
    max_ratio = _checks.integer(what, "max_ratio", max_ratio, 1, MATCH_MAX_RATIO)
    star = numpy.atleast_1d(numpy.asarray(star))
    if star.size and star.dtype.kind not in "iu":
        raise ValueError("%s: star must hold integers" % what)
    try:
        star = numpy.ascontiguousarray(star, dtype=numpy.int64)
        period, T0, duration, strength = (numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(v, dtype=numpy.float64)))
                                          for v in (period, T0, duration, strength))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: star must hold 64-bit integers, period, T0, duration and strength numbers" % what)
    if star.ndim != 1 or not star.shape == period.shape == T0.shape == duration.shape == strength.shape:
        raise ValueError("%s: star, period, T0, duration and strength must all be [M]" % what)
    if len(star) > MATCH_MAX_CANDIDATES:
        raise ValueError("%s: at most %d candidates, got %d" % (what, MATCH_MAX_CANDIDATES, len(star)))
    return dict(star=star, period=period, T0=T0, duration=duration, strength=strength, span=span,
                drift_tolerance=drift_tolerance, epoch_tolerance=epoch_tolerance, max_ratio=max_ratio)


# tls_noise_curve (include/tls_amd.h): the per-curve part of a noise profile, 6 doubles
NOISE_CURVE_FIELDS = ("status", "n_clipped", "n_pairs", "median", "sigma", "sigma_p2p")


class NoiseCurve(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in NOISE_CURVE_FIELDS]


NOISE_CURVE_DTYPE = numpy.dtype([(k, "f8") for k in NOISE_CURVE_FIELDS])
# tls_noise_curve.status
NOISE_MEASURED, NOISE_NO_SIGMA = 0, 1


def noise_arguments(t, y, widths, span_max, pair_span, clip_upper=5.0, clip_lower=5.0, min_count=3):
    """What tls_noise_profile takes, checked as it checks them: a dict with t (float64 [n], finite and ascending, or None), y
    (float64 [n_curves, n], finite; one row becomes [1, n]), n in [3, NOISE_MAX_POINTS], widths (int64 [W], W in
    [1, NOISE_MAX_WIDTHS], integers, strictly ascending in [1, min(n, NOISE_MAX_WIDTH)]), span_max (float64 [W], >= 0, inf
    allowed), pair_span (>= 0, inf allowed), clip_upper and clip_lower (>= 0, inf allowed) and min_count (an integer >= 1).
    ValueError otherwise.  GPU-free."""
    what = "noise profile"
    try:
        y = numpy.asarray(y, dtype=numpy.float64)
        t = None if t is None else numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise ValueError("%s: the light curves and t must hold numbers" % what)
    y, _ = _checks.row_shapes(what, t, y, names="flux")
    n = y.shape[1]
    if not 3 <= n <= NOISE_MAX_POINTS:
        raise ValueError("%s: n must lie in [3, %d], got %d" % (what, NOISE_MAX_POINTS, n))
    if t is not None:
        _checks.time_values(what, t, "ascending")
    y, _ = _checks.row_values(what, y, noun="the flux")
    raw = numpy.atleast_1d(numpy.asarray(widths))
    if raw.ndim != 1 or not 1 <= len(raw) <= NOISE_MAX_WIDTHS:
        raise ValueError("%s: widths must be [W] with W in [1, %d]" % (what, NOISE_MAX_WIDTHS))
    if raw.dtype.kind == "f" and numpy.all(numpy.isfinite(raw)) and numpy.all(raw == numpy.floor(raw)):
        raw = raw.astype(numpy.int64)
    if raw.dtype.kind not in "iu":
        raise ValueError("%s: the widths must be integers, got %r" % (what, widths))
    w = numpy.ascontiguousarray(raw, dtype=numpy.int64)
    if w.min() < 1 or w.max() > min(n, NOISE_MAX_WIDTH) or not numpy.all(w[1:] > w[:-1]):
        raise ValueError("%s: the widths must ascend strictly within [1, min(n, %d)] = [1, %d], got %r"
                         % (what, NOISE_MAX_WIDTH, min(n, NOISE_MAX_WIDTH), w.tolist()))
    try:
        span = numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(span_max, dtype=numpy.float64)))
    except (TypeError, ValueError):
        raise ValueError("%s: span_max must hold numbers" % what)
    if span.shape != w.shape or not numpy.all(span >= 0.0):
        raise ValueError("%s: span_max must hold one value >= 0 a width" % what)
    pair_span, clip_upper, clip_lower = (_checks.not_negative(what, name, v) for name, v in (
        ("pair_span", pair_span), ("clip_upper", clip_upper), ("clip_lower", clip_lower)))
    min_count = _checks.integer(what, "min_count", min_count, 1, 2 ** 31 - 1, "must be an integer >= 1")
    return dict(t=t, y=y, widths=w, span_max=span, pair_span=pair_span, clip_upper=clip_upper, clip_lower=clip_lower,
                min_count=min_count)


# tls_single_event (include/tls_amd.h): one single-transit event, 8 doubles
SINGLE_EVENT_FIELDS =("index", "time", "ses", "depth", "row", "width", "t_first", "t_last")


class SingleEvent(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in SINGLE_EVENT_FIELDS]


SINGLE_EVENT_DTYPE = numpy.dtype([(k, "f8") for k in SINGLE_EVENT_FIELDS])


def _single_number(name, value, low=0.0, what="single transits"):
    """value as a float, finite and >= low; ValueError otherwise (a bool or a non-number included)."""
    _checks.real(what, name, value)
    return _checks.finite_at_least(what, name, value, low)


def single_widths(widths, what="single transits"):
    """The widths as an int64 array, checked as tls_single_transits checks them: integers, at least one, strictly ascending,
    in [SINGLE_MIN_WIDTH, SINGLE_MAX_WIDTH]; ValueError otherwise, its message headed by `what`."""
    try:
        if any(isinstance(v, (bool, numpy.bool_)) for v in widths):
            raise TypeError
        width = numpy.array([operator.index(v) for v in widths], dtype=numpy.int64)
    except TypeError:
        raise ValueError("%s: the widths must be integers, got %r" % (what, widths,))
    if len(width) < 1:
        raise ValueError("%s: at least one width is needed" % what)
    if width.min() < SINGLE_MIN_WIDTH or width.max() > SINGLE_MAX_WIDTH:
        raise ValueError("%s: every width must be in [%d, %d], got %d to %d"
                         % (what, SINGLE_MIN_WIDTH, SINGLE_MAX_WIDTH, width.min(), width.max()))
    if not numpy.all(width[1:] > width[:-1]):
        raise ValueError("%s: the widths must be strictly ascending" % what)
    return width


def single_options(depth_min=0.0, k=8, min_ses=0.0, separation=0.5):
    """(depth_min, k, min_ses, separation) as tls_single_transits takes them, checked as it checks them: depth_min and
    separation finite and >= 0, k an integer in [1, SINGLE_MAX_K], min_ses no NaN (None: -inf, no threshold); ValueError
    otherwise."""
    k = _checks.integer("single transits", "k", k, 1, SINGLE_MAX_K)
    depth_min = _single_number("depth_min", depth_min)
    separation = _single_number("separation", separation)
    min_ses = _checks.no_nan("single transits", "min_ses", -numpy.inf if min_ses is None else min_ses)
    return depth_min, k, min_ses, separation


def single_arguments(t, y, dy, widths, shapes, span_max, depth_min=0.0, k=8, min_ses=0.0, separation=0.5,
                     what="single transits", max_points=SINGLE_MAX_POINTS):
    """What tls_single_transits takes, checked as it checks them and packed for it -- a dict with t [n], y and dy
    [n_curves, n], width [n_rows] (int64), shape_values (the rows of `shapes` back to back), shape_offset [n_rows] (int64),
    span_max [n_rows], depth_min, k, min_ses, separation.  t is 1-D with n in [1, SINGLE_MAX_POINTS], finite and
    non-decreasing; y and dy are [n] or [n_curves, n], dy finite and > 0, y finite; widths are integers, strictly ascending,
    in [SINGLE_MIN_WIDTH, SINGLE_MAX_WIDTH], at least one; shapes[r] holds widths[r] finite values; span_max[r], depth_min
    and separation are finite and >= 0; k is an integer in [1, SINGLE_MAX_K]; min_ses is no NaN (None: -inf, no threshold).
    ValueError otherwise.  GPU-free.  tls_transit_times takes the same t, y, dy and rows: `what` heads the messages and
    max_points is the entry's limit of n."""
    t = _checks.times(what, t, max_points)
    y, dy = _checks.rows(what, t, y, dy)
    width = single_widths(widths, what)
    if len(shapes) != len(width):
        raise ValueError("%s: %d shapes for %d widths" % (what, len(shapes), len(width)))
    rows = [numpy.asarray(b, dtype=numpy.float64) for b in shapes]
    for r, b in enumerate(rows):
        if b.shape != (width[r],) or not numpy.all(numpy.isfinite(b)):
            raise ValueError("%s: shape %d must hold %d finite values" % (what, r, width[r]))
    span = numpy.asarray(span_max, dtype=numpy.float64)
    if span.shape != width.shape or not numpy.all(numpy.isfinite(span) & (span >= 0.0)):
        raise ValueError("%s: span_max must hold one finite value >= 0 a width" % what)
    depth_min, k, min_ses, separation = single_options(depth_min, k, min_ses, separation)
    offset = numpy.zeros(len(width), dtype=numpy.int64)
    offset[1:] = numpy.cumsum(width)[:-1]
    return dict(t=t, y=y, dy=dy, width=width,
                shape_values=numpy.ascontiguousarray(numpy.concatenate(rows)), shape_offset=offset,
                span_max=numpy.ascontiguousarray(span), depth_min=depth_min, k=k, min_ses=min_ses,
                separation=separation)


# tls_ephemeris and tls_transit_time (include/tls_amd.h): a candidate's refitted ephemeris, 12 doubles, and one of its
# transits, 8 doubles
EPHEMERIS_FIELDS = ("status", "n_epochs", "n_timed", "epoch_first", "period", "period_err", "T0", "T0_err", "ttv_chi2",
                    "ttv_rms", "ttv_max_sigma", "ttv_max_epoch")
TRANSIT_TIME_FIELDS = ("epoch", "status", "time_linear", "time", "time_err", "ses", "depth", "index")


class Ephemeris(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in EPHEMERIS_FIELDS]


class TransitTime(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in TRANSIT_TIME_FIELDS]


EPHEMERIS_DTYPE = numpy.dtype([(k, "f8") for k in EPHEMERIS_FIELDS])
TRANSIT_TIME_DTYPE = numpy.dtype([(k, "f8") for k in TRANSIT_TIME_FIELDS])


def transit_times_options(depth_min=0.0, min_ses=3.0, max_epochs=1, what="transit times"):
    """(depth_min, min_ses, max_epochs) as tls_transit_times takes them, checked as it checks them: depth_min finite and
    >= 0, min_ses a number and no NaN, max_epochs an integer in [1, TIMES_MAX_EPOCHS]; ValueError otherwise, headed `what`."""
    return (_checks.finite_at_least(what, "depth_min", depth_min), _checks.no_nan(what, "min_ses", min_ses),
            _checks.integer(what, "max_epochs", max_epochs, 1, TIMES_MAX_EPOCHS))


def transit_times_arguments(t, y, dy, period, T0, row, reach, widths, shapes, span_max, curve=None, depth_min=0.0,
                            min_ses=3.0, max_epochs=1, what="transit times"):
    """What tls_transit_times takes, checked as it checks them and packed for it -- the dict of single_arguments for t, y,
    dy and the rows (width, shape_values, shape_offset, span_max: n up to TIMES_MAX_POINTS), plus period, T0 [n_fits]
    (float64, any value: the device gives a candidate without an ephemeris status 1), curve (None: one candidate a curve,
    in order), row and reach [n_fits] (int64; curve in [0, n_curves), row in [0, n_rows), reach in [1, TIMES_MAX_REACH]),
    depth_min, min_ses, max_epochs (transit_times_options).  ValueError otherwise, headed `what`: tls_event_vetting takes
    the same.  GPU-free."""
    depth_min, min_ses, max_epochs = transit_times_options(depth_min, min_ses, max_epochs, what)
    a = single_arguments(t, y, dy, widths, shapes, span_max, depth_min, what=what, max_points=TIMES_MAX_POINTS)
    period, T0 = _checks.columns(what, "period and T0", (period, T0))
    n_fits, n_curves = len(period), len(a["y"])
    if curve is None:
        if n_fits != n_curves:
            raise _checks.one_a_curve(what, n_fits, n_curves)
        curve = numpy.arange(n_curves)
    ints = _checks.integer_columns(what, period.shape, (("curve", curve, 0, n_curves - 1), ("row", row, 0, len(a["width"]) - 1),
                                                        ("reach", reach, 1, TIMES_MAX_REACH)))
    for k in ("k", "separation"):
        del a[k]
    a.update(ints, period=period, T0=T0, depth_min=depth_min, min_ses=min_ses, max_epochs=max_epochs)
    return a


# tls_event_pair and tls_event_alias (include/tls_amd.h): the period aliases of a pair of events, 16 doubles, and one alias,
# 8 doubles
EVENT_PAIR_FIELDS = ("status", "dT", "n_aliases", "n_evaluated", "n_allowed", "pair_mes", "pair_depth", "best_k", "best_period",
                     "best_mes", "best_n_covered", "best_n_seen", "longest_k", "longest_period", "shortest_k",
                     "shortest_period")
EVENT_ALIAS_FIELDS = ("period", "n_epochs", "n_covered", "n_seen", "mes", "depth", "worst_sigma", "worst_epoch")


class EventPair(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in EVENT_PAIR_FIELDS]


class EventAlias(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in EVENT_ALIAS_FIELDS]


EVENT_PAIR_DTYPE = numpy.dtype([(k, "f8") for k in EVENT_PAIR_FIELDS])
EVENT_ALIAS_DTYPE = numpy.dtype([(k, "f8") for k in EVENT_ALIAS_FIELDS])


def event_periods_options(period_min, max_aliases=256, min_ses=3.0, veto_sigma=3.0):
    """(period_min, max_aliases, min_ses, veto_sigma) as tls_event_periods takes them, checked as it checks them: period_min
    finite and > 0, max_aliases an integer in [1, ALIAS_MAX], min_ses and veto_sigma numbers and no NaN (veto_sigma +inf: no
    veto); ValueError otherwise."""
    what = "event periods"
    return (_checks.finite_positive(what, "period_min", period_min),
            _checks.integer(what, "max_aliases", max_aliases, 1, ALIAS_MAX),
            _checks.no_nan(what, "min_ses", min_ses), _checks.no_nan(what, "veto_sigma", veto_sigma))


def event_periods_arguments(t, y, dy, curve, index_a, index_b, row, reach, offset, widths, shapes, span_max, period_min,
                            max_aliases=256, min_ses=3.0, veto_sigma=3.0):
    """What tls_event_periods takes, checked as it checks them and packed for it -- the dict of single_arguments for t, y, dy
    and the rows (n up to ALIAS_MAX_POINTS), plus curve, index_a, index_b, row and reach [n_pairs] (int64; curve in
    [0, n_curves), 0 <= index_a < index_b < n, row in [0, n_rows), reach in [1, TIMES_MAX_REACH]), offset [n_pairs] (float64,
    finite and >= 0 days) and period_min, max_aliases, min_ses, veto_sigma (event_periods_options; (t[n-1] - t[0]) / period_min
    + 2 is at most TIMES_MAX_EPOCHS).  ValueError otherwise.  GPU-free."""
    what = "event periods"
    period_min, max_aliases, min_ses, veto_sigma = event_periods_options(period_min, max_aliases, min_ses, veto_sigma)
    a = single_arguments(t, y, dy, widths, shapes, span_max, what=what, max_points=ALIAS_MAX_POINTS)
    n, n_curves = len(a["t"]), len(a["y"])
    if not (a["t"][-1] - a["t"][0]) / period_min + 2.0 <= TIMES_MAX_EPOCHS:
        raise ValueError("%s: period_min %r gives an alias more than %d epochs over %r days"
                         % (what, period_min, TIMES_MAX_EPOCHS, a["t"][-1] - a["t"][0]))
    shape = numpy.atleast_1d(numpy.asarray(curve)).shape
    ints = _checks.integer_columns(what, shape, (
        ("curve", curve, 0, n_curves - 1), ("index_a", index_a, 0, n - 1), ("index_b", index_b, 0, n - 1),
        ("row", row, 0, len(a["width"]) - 1), ("reach", reach, 1, TIMES_MAX_REACH)), "pair")
    if not numpy.all(ints["index_a"] < ints["index_b"]):
        raise ValueError("%s: index_a must lie in front of index_b" % what)
    offset = _checks.float_column(what, "offset", offset, shape, "pair", not_numbers="must be numbers")
    for k in ("k", "separation", "depth_min", "min_ses"):
        del a[k]
    a.update(ints, offset=offset, period_min=period_min, max_aliases=max_aliases, min_ses=min_ses, veto_sigma=veto_sigma)
    return a


# tls_event_summary and tls_event_record (include/tls_amd.h): a candidate's event vetting, 15 doubles, and one of its events,
# 14 doubles
EVENT_SUMMARY_FIELDS = ("status", "n_epochs", "epoch_first", "n_held", "n_good", "mes", "mes_good", "mes_rest", "ses_max",
                        "ses_max_epoch", "dominance", "depth_mean", "depth_chi2", "chases_min", "chases_mean")
EVENT_RECORD_FIELDS = ("epoch", "status", "time_linear", "ses", "depth", "depth_err", "index", "point_share", "before", "after",
                       "chases", "chase_dt", "n_chased", "flags")


class EventSummary(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in EVENT_SUMMARY_FIELDS]


class EventRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in EVENT_RECORD_FIELDS]


EVENT_SUMMARY_DTYPE = numpy.dtype([(k, "f8") for k in EVENT_SUMMARY_FIELDS])
EVENT_RECORD_DTYPE = numpy.dtype([(k, "f8") for k in EVENT_RECORD_FIELDS])


def event_vetting_options(chase_fraction=0.6, chase_min=0.5, point_fraction=0.5, step_fraction=0.5):
    """(chase_fraction, chase_min, point_fraction, step_fraction) as tls_event_vetting takes them, checked as it checks them:
    numbers, chase_fraction in (0, 1], chase_min in [0, 1], point_fraction and step_fraction > 0; ValueError otherwise."""
    what = "event vetting"
    return (_checks.within(what, "chase_fraction", chase_fraction, 0.0, 1.0, low_open=True),
            _checks.within(what, "chase_min", chase_min, 0.0, 1.0),
            _checks.positive(what, "point_fraction", point_fraction),
            _checks.positive(what, "step_fraction", step_fraction))


def event_vetting_arguments(t, y, dy, period, T0, row, reach, chase_reach, guard, chase_span, widths, shapes, span_max,
                            curve=None, depth_min=0.0, min_ses=3.0, chase_fraction=0.6, chase_min=0.5, point_fraction=0.5,
                            step_fraction=0.5, max_epochs=1):
    """What tls_event_vetting takes, checked as it checks them and packed for it: the dict of transit_times_arguments (its
    messages headed "event vetting"), plus chase_reach and guard [n_fits] (int64; chase_reach in [0, EVENTS_MAX_CHASE],
    guard >= 0), chase_span [n_fits] (float64, finite and > 0) and the four parameters (event_vetting_options).  ValueError
    otherwise.  GPU-free."""
    options = event_vetting_options(chase_fraction, chase_min, point_fraction, step_fraction)
    what = "event vetting"
    a = transit_times_arguments(t, y, dy, period, T0, row, reach, widths, shapes, span_max, curve, depth_min, min_ses,
                                max_epochs, what)
    shape = a["period"].shape
    a.update(_checks.integer_columns(what, shape, (("chase_reach", chase_reach, 0, EVENTS_MAX_CHASE),
                                                   ("guard", guard, 0, None))))
    span = _checks.float_column(what, "chase_span", chase_span, shape, "candidate", above=">")
    a.update(chase_span=span, chase_fraction=options[0], chase_min=options[1], point_fraction=options[2],
             step_fraction=options[3])
    return a


# tls_shape_record (include/tls_amd.h): a candidate's trapezoid shape fit, 16 doubles
SHAPE_FIELDS = ("status", "n_points", "n_in", "ses", "depth", "depth_err", "duration", "ingress", "shift", "i_duration",
                "i_ingress", "i_shift", "ses_box", "duration_box", "ses_vee", "duration_vee")


class ShapeRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in SHAPE_FIELDS]


SHAPE_DTYPE = numpy.dtype([(k, "f8") for k in SHAPE_FIELDS])


def shape_fit_tables(ratios, ingress, shifts, window=2.0, min_count=3, depth_min=0.0):
    """(ratio, ingress, shift, window, min_count, depth_min) as tls_shape_fit takes them, checked as it checks them: every
    table 1-D, not empty, finite and non-decreasing; every ratio > 0; ingress[0] == 0.0 and ingress[-1] == 0.5; between 1 and
    SHAPE_MAX_UNITS units; window finite and at least 0.5 * max(ratio) + max|shift| (the model must lie inside the window);
    min_count an integer >= 1; depth_min finite and >= 0.  ValueError otherwise."""
    what = "shape fit"
    ratio, ingress, shift = (_checks.table(what, name, v)
                             for name, v in (("ratios", ratios), ("ingress", ingress), ("shifts", shifts)))
    if not ratio[0] > 0.0:
        raise ValueError("shape fit: every ratio must be > 0, got %r" % ratio[0])
    if ingress[0] != 0.0 or ingress[-1] != 0.5:
        raise ValueError("shape fit: ingress must run from 0.0 (a box) to 0.5 (a V), got %r to %r" % (ingress[0], ingress[-1]))
    units = len(ratio) * len(ingress) * len(shift)
    if not 1 <= units <= SHAPE_MAX_UNITS:
        raise ValueError("shape fit: %d units, outside [1, %d]" % (units, SHAPE_MAX_UNITS))
    window = _checks.fit_window(what, window, ratio, shift)
    return (ratio, ingress, shift, window, _checks.integer(what, "min_count", min_count, 1),
            _checks.finite_at_least(what, "transit_depth_min", depth_min))


def shape_fit_candidates(period, T0, duration, curve, n_curves, what="shape fit"):
    """(period, T0, duration [n_fits] float64, curve [n_fits] int64) of tls_shape_fit, checked: numbers of one 1-D shape (any
    value: the device gives a candidate without an ephemeris status 1), curve (None: one candidate a curve, in order) integers
    in [0, n_curves).  ValueError otherwise, headed `what`."""
    return tuple(_checks.candidates(what, period, T0, duration, curve, n_curves))


def candidate_series(what, t, y, dy, period, T0, duration, curve, max_points):
    """The light curves and candidates of a per-candidate stage, checked: a dict with t [n] (1-D, n in [1, max_points],
    finite and non-decreasing), y and dy [n_curves, n] (y finite, dy finite and > 0) and period, T0, duration, curve
    [n_fits] (shape_fit_candidates).  ValueError otherwise, headed `what`."""
    t = _checks.times(what, t, max_points)
    y, dy = _checks.rows(what, t, y, dy)
    period, T0, duration, curve = _checks.candidates(what, period, T0, duration, curve, len(y))
    return dict(t=t, y=y, dy=dy, period=period, T0=T0, duration=duration, curve=curve)


def shape_fit_arguments(t, y, dy, period, T0, duration, ratios, ingress, shifts, curve=None, window=2.0, min_count=3,
                        depth_min=0.0):
    """What tls_shape_fit takes, checked as it checks them and packed for it -- a dict with t [n] (n up to
    SHAPE_MAX_POINTS), y and dy [n_curves, n], period, T0, duration, curve [n_fits] (candidate_series), ratio, ingress,
    shift, window, min_count, depth_min (shape_fit_tables).  ValueError otherwise.  GPU-free."""
    ratio, ingress, shift, window, min_count, depth_min = shape_fit_tables(ratios, ingress, shifts, window, min_count, depth_min)
    return dict(candidate_series("shape fit", t, y, dy, period, T0, duration, curve, SHAPE_MAX_POINTS), ratio=ratio,
                ingress=ingress, shift=shift, window=window, min_count=min_count, depth_min=depth_min)


# tls_transit_fit_record (include/tls_amd.h): a candidate's limb-darkened transit fit, 24 doubles; the limits of
# tls_transit_fit (TLS_TRANSIT_FIT_MAX_*; tls_transit_fit.hip.h kTransitMax*)
TRANSIT_FIT_FIELDS = ("status", "n_points", "n_in", "row_first", "row", "ses", "amplitude", "k", "b", "duration", "shift",
                      "i_impact", "i_duration", "i_shift", "x2", "k_lo", "k_hi", "b_lo", "b_hi", "duration_lo", "duration_hi",
                      "shift_lo", "shift_hi", "reserved")
TRANSIT_FIT_MAX_UNITS = 65536
TRANSIT_FIT_MAX_M = 4096
TRANSIT_FIT_MAX_SUB = 16
TRANSIT_FIT_MAX_ROWS = 4096
TRANSIT_FIT_SLAB = 512


class TransitFitRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in TRANSIT_FIT_FIELDS]


TRANSIT_FIT_DTYPE = numpy.dtype([(k, "f8") for k in TRANSIT_FIT_FIELDS])


def transit_fit_tables(k_rows, profile, impacts, ratios, shifts, sub, window=1.0, min_count=3, delta=1.0, what="transit fit"):
    """(k_rows, profile, impact, ratio, shift, sub, window, min_count, delta) as tls_transit_fit takes them, checked as it
    checks them: k_rows [nK] finite, ascending and > 0, nK <= TRANSIT_FIT_MAX_ROWS; profile [nK, M + 1] finite with M in
    [1, TRANSIT_FIT_MAX_M]; impacts, ratios, shifts 1-D, not empty, finite and ascending, impacts in [0, 1), ratios > 0, at
    most TRANSIT_FIT_MAX_UNITS units; sub [S] finite, S in [1, TRANSIT_FIT_MAX_SUB]; window finite and at least
    0.5 * max(ratio) + max|shift|; min_count an integer >= 1; delta finite and >= 0.  ValueError otherwise, headed `what`:
    tls_remove_transits takes the same k_rows, profile and sub."""
    k_rows, impact, ratio, shift = (_checks.table(what, name, v) for name, v in (
        ("k_rows", k_rows), ("impacts", impacts), ("ratios", ratios), ("shifts", shifts)))
    sub = _checks.table(what, "sub", sub, ascending=False)
    if not k_rows[0] > 0.0 or len(k_rows) > TRANSIT_FIT_MAX_ROWS:
        raise _checks.refusal(what, "k_rows must hold at most %d values > 0" % TRANSIT_FIT_MAX_ROWS)
    try:
        profile = numpy.ascontiguousarray(numpy.asarray(profile, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise _checks.refusal(what, "profile must hold numbers")
    if profile.ndim != 2 or profile.shape[0] != len(k_rows) or not 1 <= profile.shape[1] - 1 <= TRANSIT_FIT_MAX_M:
        raise _checks.refusal(what, "profile must be [len(k_rows), M + 1] with M in [1, %d], got shape %s"
                              % (TRANSIT_FIT_MAX_M, profile.shape))
    if not numpy.all(numpy.isfinite(profile)):
        raise _checks.refusal(what, "profile must be finite")
    if not (impact[0] >= 0.0 and impact[-1] < 1.0):
        raise _checks.refusal(what, "every impact must be in [0, 1)")
    if not ratio[0] > 0.0:
        raise _checks.refusal(what, "every ratio must be > 0, got %r" % ratio[0])
    if len(sub) > TRANSIT_FIT_MAX_SUB:
        raise _checks.refusal(what, "n_sub %d outside [1, %d]" % (len(sub), TRANSIT_FIT_MAX_SUB))
    units = len(impact) * len(ratio) * len(shift)
    if not 1 <= units <= TRANSIT_FIT_MAX_UNITS:
        raise _checks.refusal(what, "%d units, outside [1, %d]" % (units, TRANSIT_FIT_MAX_UNITS))
    window = _checks.fit_window(what, window, ratio, shift)
    return (k_rows, profile, impact, ratio, shift, sub, window, _checks.integer(what, "min_count", min_count, 1),
            _checks.finite_at_least(what, "delta", delta))


def transit_fit_window_holds(duration, ratio, shift, sub, window):
    """Whether the window of every candidate with a finite duration > 0 holds the widest, farthest shifted model plus half an
    exposure, as tls_transit_fit checks it: window * d >= (0.5 * ratio[-1] + max|shift|) * d + max|sub|."""
    d = numpy.asarray(duration, dtype=numpy.float64)
    reach = 0.5 * float(ratio[-1]) + max(abs(float(shift[0])), abs(float(shift[-1])))
    sub_reach = float(numpy.max(numpy.fabs(sub)))
    with numpy.errstate(all="ignore"):
        checked = numpy.isfinite(d) & (d > 0.0)
        return bool(numpy.all(~checked | (float(window) * d >= reach * d + sub_reach)))


def transit_fit_arguments(t, y, dy, period, T0, duration, row_first, k_rows, profile, impacts, ratios, shifts, sub, curve=None,
                          window=1.0, min_count=3, delta=1.0):
    """What tls_transit_fit takes, checked as it checks them and packed for it -- a dict with t [n], y and dy [n_curves, n],
    period, T0, duration, curve [n_fits] (candidate_series, n up to SHAPE_MAX_POINTS), row_first [n_fits] int64 in [0, nK),
    and k_rows, profile, impact, ratio, shift, sub, window, min_count, delta (transit_fit_tables).  ValueError otherwise.
    GPU-free."""
    k_rows, profile, impact, ratio, shift, sub, window, min_count, delta = transit_fit_tables(
        k_rows, profile, impacts, ratios, shifts, sub, window, min_count, delta)
    a = candidate_series("transit fit", t, y, dy, period, T0, duration, curve, SHAPE_MAX_POINTS)
    rows = _checks.indices("transit fit", "row_first", row_first, a["period"].shape, len(k_rows), "row")
    if not transit_fit_window_holds(a["duration"], ratio, shift, sub, window):
        raise ValueError("transit fit: window %r does not hold the widest, farthest shifted model plus half an exposure for "
                         "the shortest duration" % (window,))
    return dict(a, row_first=rows, k_rows=k_rows, profile=profile, impact=impact, ratio=ratio, shift=shift, sub=sub,
                window=window, min_count=min_count, delta=delta)


# tls_centroid_record (include/tls_amd.h): a candidate's centroid-shift test, 16 doubles
CENTROID_FIELDS = ("status", "n_epochs", "n_skipped", "n_points", "n_in", "depth", "depth_err", "shift_x", "shift_x_err",
                   "shift_y", "shift_y_err", "rms_x", "rms_y", "chi2_depth", "chi2_x", "chi2_y")


class CentroidRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in CENTROID_FIELDS]


CENTROID_DTYPE = numpy.dtype([(k, "f8") for k in CENTROID_FIELDS])


def centroid_options(window=3.0, min_in=1, min_out=3, max_epochs=CENTROID_MAX_EPOCHS):
    """(window, min_in, min_out, max_epochs) as tls_centroid_test takes them, checked as it checks them: window a finite
    number >= 1; min_in and min_out integers >= 1; max_epochs an integer in [1, CENTROID_MAX_EPOCHS].  ValueError otherwise."""
    what = "centroid test"
    return (_checks.finite_at_least(what, "window", window, 1.0), _checks.integer(what, "min_in", min_in, 1),
            _checks.integer(what, "min_out", min_out, 1), _checks.integer(what, "max_epochs", max_epochs, 1, CENTROID_MAX_EPOCHS))


def centroid_rows(cx, cy, shape):
    """(cx, cy) as float64 arrays of `shape` = flux_batch's ([n_curves, n]; one row [n] is taken as [1, n]); any value, NaN
    and infinities included (the device skips such a point).  ValueError for anything else."""
    rows = []
    for name, v in (("cx", cx), ("cy", cy)):
        try:
            v = numpy.asarray(v, dtype=numpy.float64)
        except (TypeError, ValueError):
            raise ValueError("centroid test: %s must hold numbers" % name)
        if v.ndim == 1:
            v = v[None, :]
        if v.shape != tuple(shape):
            raise ValueError("centroid test: %s must have the shape of the flux, %s, got %s" % (name, tuple(shape), v.shape))
        rows.append(numpy.ascontiguousarray(v))
    return rows[0], rows[1]


def centroid_arguments(t, y, cx, cy, period, T0, duration, shape, curve=None, window=3.0, min_in=1, min_out=3,
                       max_epochs=CENTROID_MAX_EPOCHS):
    """What tls_centroid_test takes, checked as it checks them and packed for it -- a dict with t [n] (1-D, n in
    [1, CENTROID_MAX_POINTS], finite and non-decreasing), y [n_curves, n] (finite), cx and cy of y's shape (centroid_rows),
    period, T0, duration, curve [n_fits] (shape_fit_candidates), shape [L] (1-D, L in [2, CENTROID_MAX_SHAPE], finite) and
    window, min_in, min_out, max_epochs (centroid_options).  ValueError otherwise.  GPU-free."""
    window, min_in, min_out, max_epochs = centroid_options(window, min_in, min_out, max_epochs)
    try:
        shape = numpy.ascontiguousarray(numpy.asarray(shape, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise ValueError("centroid test: the shape must hold numbers")
    if shape.ndim != 1 or not 2 <= len(shape) <= CENTROID_MAX_SHAPE:
        raise ValueError("centroid test: the shape must be [L] with L in [2, %d], got %s" % (CENTROID_MAX_SHAPE, shape.shape))
    if not numpy.all(numpy.isfinite(shape)):
        raise ValueError("centroid test: the shape must be finite")
    t = _checks.times("centroid test", t, CENTROID_MAX_POINTS)
    y = _checks.flux_rows("centroid test", t, y)
    cx, cy = centroid_rows(cx, cy, y.shape)
    period, T0, duration, curve = _checks.candidates("centroid test", period, T0, duration, curve, len(y))
    return dict(t=t, y=y, cx=cx, cy=cy, period=period, T0=T0, duration=duration, curve=curve, shape=shape, window=window,
                min_in=min_in, min_out=min_out, max_epochs=max_epochs)


# tls_views_record (include/tls_amd.h): a candidate's folded views, 7 doubles; the local views in the order of the arrays
VIEWS_FIELDS = ("status", "secondary_status", "n_global", "n_local", "n_local_even", "n_local_odd", "n_secondary")
VIEWS_LOCAL = ("local", "local_even", "local_odd", "secondary")


class ViewsRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in VIEWS_FIELDS]


VIEWS_DTYPE = numpy.dtype([(k, "f8") for k in VIEWS_FIELDS])


def folded_views_tables(n_global=2001, n_local=201, local_durations=4.0, local_width=0.16):
    """(n_global, n_local, local_durations, local_width) as tls_folded_views takes them, checked as it checks them: the bin
    counts integers in [2, VIEWS_MAX_BINS]; local_durations finite and > 0; local_width finite, > 0 and at most
    2 * local_durations (a bin no wider than the view).  ValueError otherwise."""
    what = "folded views"
    n_global = _checks.integer(what, "n_global", n_global, 2, VIEWS_MAX_BINS)
    n_local = _checks.integer(what, "n_local", n_local, 2, VIEWS_MAX_BINS)
    for name, v in (("local_durations", local_durations), ("local_width", local_width)):
        _checks.finite_positive(what, name, v)
    if float(local_width) > 2.0 * float(local_durations):
        raise ValueError("folded views: local_width %r is wider than the view, 2 * local_durations = %r"
                         % (local_width, 2.0 * float(local_durations)))
    return n_global, n_local, float(local_durations), float(local_width)


def folded_views_arguments(t, y, period, T0, duration, curve=None, secondary_phase=None, n_global=2001, n_local=201,
                           local_durations=4.0, local_width=0.16):
    """What tls_folded_views takes, checked as it checks them and packed for it -- a dict with t [n] (1-D, n in
    [1, VIEWS_MAX_POINTS], finite and non-decreasing), y [n_curves, n] (finite), period, T0, duration, curve [n_fits]
    (shape_fit_candidates: any value, curve in [0, n_curves)), secondary_phase [n_fits] or None, and the four table
    parameters (folded_views_tables).  ValueError otherwise.  GPU-free."""
    n_global, n_local, k, width = folded_views_tables(n_global, n_local, local_durations, local_width)
    t = _checks.times("folded views", t, VIEWS_MAX_POINTS)
    y = _checks.flux_rows("folded views", t, y)
    period, T0, duration, curve = _checks.candidates("folded views", period, T0, duration, curve, len(y))
    if secondary_phase is not None:
        secondary_phase, = _checks.floats("folded views", [secondary_phase], "secondary_phase must hold numbers")
        if secondary_phase.shape != period.shape:
            raise ValueError("folded views: secondary_phase must be [n_fits], one phase a candidate")
    return dict(t=t, y=y, period=period, T0=T0, duration=duration,
                curve=curve, secondary_phase=secondary_phase, n_global=n_global, n_local=n_local, local_durations=k,
                local_width=width)


# tls_sine_record and tls_sine_harmonic (include/tls_amd.h): the sine test of a candidate, 4 doubles and 5 a harmonic
SINE_FIELDS = ("status", "n_used", "mean", "variance")
SINE_HARMONIC_FIELDS = ("power", "amplitude", "phase", "amplitude_err", "significance")
GLS_SUMS = ("YC", "YS", "C", "S", "C2", "S2")


class SineRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in SINE_FIELDS]


class SineHarmonic(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in SINE_HARMONIC_FIELDS]


SINE_DTYPE = numpy.dtype([(k, "f8") for k in SINE_FIELDS])
SINE_HARMONIC_DTYPE = numpy.dtype([(k, "f8") for k in SINE_HARMONIC_FIELDS])


def gls_axes(t, frequencies, n_min=3):
    """(t [n], frequencies [F]) float64 and contiguous as the periodogram takes them: t 1-D, n in [n_min, GLS_MAX_POINTS],
    finite and non-decreasing; frequencies 1-D, F in [1, GLS_MAX_FREQUENCIES], finite and > 0.  ValueError otherwise."""
    try:
        t = numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64))
        f = numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(frequencies, dtype=numpy.float64)))
    except (TypeError, ValueError):
        raise ValueError("periodogram: t and frequencies must hold numbers")
    t = _checks.times("periodogram", t, GLS_MAX_POINTS, n_min, "ascending")
    if f.ndim != 1 or not 1 <= len(f) <= GLS_MAX_FREQUENCIES:
        raise ValueError("periodogram: frequencies must have shape [F] with F in [1, %d], got %s" % (GLS_MAX_FREQUENCIES, f.shape))
    if not numpy.all(numpy.isfinite(f) & (f > 0.0)):
        raise ValueError("periodogram: every frequency must be finite and > 0")
    return t, f


def gls_rows(t, y, dy, what="periodogram"):
    """(y, dy) [n_curves, n] float64 and contiguous over the time stamps t [n] (one row becomes [1, n]; dy None stays None):
    y finite, dy finite and > 0 and shaped like y.  ValueError otherwise."""
    try:
        y = numpy.asarray(y, dtype=numpy.float64)
        dy = None if dy is None else numpy.asarray(dy, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: the light curves must hold numbers" % what)
    len(t)      # (the rows lie over an array t: None, which row_shapes takes for "any n", stays the TypeError it was)
    if y.ndim != 1 and dy is not None and dy.ndim == 1:     # (a dy [n] goes with a y [n] only)
        raise _checks.over_t(what, "flux and dy")
    return _checks.row_values(what, *_checks.row_shapes(what, t, y, dy, "flux and dy"), noun="the flux")


def lomb_scargle_arguments(t, y, dy, frequencies, peaks=None, separation=0.02):
    """What tls_lomb_scargle takes, checked as it checks them: a dict with t, frequencies (gls_axes, n >= 3), y, dy
    (gls_rows), k (0: no peaks; else an integer in [1, PEAKS_MAX_K]) and separation (finite, in [0, 1)).  ValueError
    otherwise.  GPU-free."""
    t, f = gls_axes(t, frequencies, 3)
    y, dy = gls_rows(t, y, dy)
    k = 0
    if peaks is not None:
        k, separation = peaks_arguments(peaks, separation, (0.5, 2.0), None)[:2]
    return dict(t=t, frequencies=f, y=y, dy=dy, k=k, separation=float(separation))


# tls_prewhiten_term of include/tls_amd.h, in order: all doubles
PREWHITEN_FIELDS = ("status", "index", "frequency_grid", "power_left", "power_peak", "power_right", "frequency", "mean",
                    "variance", "ca", "sa", "C", "S", "power", "amplitude", "phase")


class PrewhitenTerm(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in PREWHITEN_FIELDS]


PREWHITEN_DTYPE = numpy.dtype([(k, "f8") for k in PREWHITEN_FIELDS])


def prewhiten_arguments(t, y, dy, frequencies, n_terms=3, harmonics=1, min_power=0.0):
    """What tls_prewhiten takes, checked as it checks them: a dict with t, frequencies (gls_axes, n >= 3), y, dy (gls_rows),
    n_terms (an integer in [1, PREWHITEN_MAX_TERMS]), harmonics (an integer in [1, SINE_MAX_HARMONICS]) and min_power (in
    [0, 1]).  ValueError otherwise.  GPU-free."""
    t, f = gls_axes(t, frequencies, 3)
    y, dy = gls_rows(t, y, dy, "prewhiten")
    k = _checks.integer("prewhiten", "n_terms", n_terms, 1, PREWHITEN_MAX_TERMS)
    h = _checks.integer("prewhiten", "harmonics", harmonics, 1, SINE_MAX_HARMONICS)
    min_power = _checks.within("prewhiten", "min_power", min_power, 0.0, 1.0, text="must lie in [0, 1]")
    return dict(t=t, frequencies=f, y=y, dy=dy, n_terms=k, harmonics=h, min_power=min_power)


def sine_test_arguments(t, y, dy, period, T0, duration, curve, mask, harmonics):
    """What tls_sine_test takes, checked as it checks them: a dict with t [n] (n in [1, GLS_MAX_POINTS], finite and
    ascending), y, dy (gls_rows), period [n_fits] (any value: status 1), T0 and duration (both None, or [n_fits]), curve
    (None: one candidate a curve, in order; integers in [0, n_curves)), mask (finite, >= 0) and harmonics (1 to
    SINE_MAX_HARMONICS, finite and > 0).  ValueError otherwise.  GPU-free."""
    try:
        t = numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64))
    except (TypeError, ValueError):
        raise ValueError("sine test: t must hold numbers")
    t = _checks.times("sine test", t, GLS_MAX_POINTS, order="ascending")
    y, dy = gls_rows(t, y, dy, "sine test")
    if (T0 is None) != (duration is None):
        raise ValueError("sine test: T0 and duration come together")
    try:
        period = numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(period, dtype=numpy.float64)))
        if T0 is not None:
            T0, duration = (numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(v, dtype=numpy.float64))) for v in (T0, duration))
        harmonics = numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(harmonics, dtype=numpy.float64)))
    except (TypeError, ValueError):
        raise ValueError("sine test: period, T0, duration and harmonics must be numbers")
    _checks.columns("sine test", "period, T0 and duration", (period,) if T0 is None else (period, T0, duration))
    if harmonics.ndim != 1 or not 1 <= len(harmonics) <= SINE_MAX_HARMONICS \
            or not numpy.all(numpy.isfinite(harmonics) & (harmonics > 0.0)):
        raise ValueError("sine test: harmonics must be 1 to %d finite values > 0" % SINE_MAX_HARMONICS)
    mask = _checks.finite_at_least("sine test", "mask", mask)
    curve = _checks.curves("sine test", curve, len(period), len(y))
    return dict(t=t, y=y, dy=dy, period=period, T0=T0, duration=duration, curve=curve, mask=mask, harmonics=harmonics)


def peaks_arguments(k, separation, ratios, min_power):
    """(k, separation, ratios, min_power) as the peak selection takes them, checked as tls_find_peaks checks them: k an
    integer in [1, PEAKS_MAX_K]; separation finite and in [0, 1); at most PEAKS_MAX_RATIOS ratios, each finite and > 0;
    min_power not NaN (None: -inf, no threshold).  ValueError otherwise."""
    k = _checks.integer("peaks", "k", k, 1, PEAKS_MAX_K)
    try:
        sep = float(separation)
        rat = numpy.array([] if ratios is None else ratios, dtype=numpy.float64).reshape(-1)
        low = -numpy.inf if min_power is None else float(min_power)
    except (TypeError, ValueError):
        raise ValueError("peaks: separation, ratios and min_power must be numbers")
    if not (numpy.isfinite(sep) and 0.0 <= sep < 1.0):
        raise ValueError("peaks: the separation must be finite and in [0, 1), got %r" % (separation,))
    if len(rat) > PEAKS_MAX_RATIOS:
        raise ValueError("peaks: at most %d ratios, got %d" % (PEAKS_MAX_RATIOS, len(rat)))
    if not numpy.all(numpy.isfinite(rat) & (rat > 0.0)):
        raise ValueError("peaks: every ratio must be finite and > 0")
    if numpy.isnan(low):
        raise ValueError("peaks: min_power is NaN")
    return k, sep, numpy.ascontiguousarray(rat), low


INJECTION_FIELDS = ("tp", "period", "rp", "a", "sin_inc", "omega")


class Injection(ctypes.Structure):
    """tls_injection: the constants of one injected planet on a circular orbit (include/tls_amd.h), 48 bytes."""
    _fields_ = [(k, ctypes.c_double) for k in INJECTION_FIELDS]


INJECTION_DTYPE = numpy.dtype([(k, "f8") for k in INJECTION_FIELDS])


class Counters(ctypes.Structure):
    _fields_ = [("grid_cells", ctypes.c_int64), ("evaluated_cells", ctypes.c_int64),
                ("inner_steps", ctypes.c_int64), ("pd_pairs", ctypes.c_int64),
                ("issued_fma", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_lib = None


def load():
    """Load libtls_amd.so once; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "tls_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C tls_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.tls_abi_version.restype = ci
    if lib.tls_abi_version() != ABI_VERSION:
        raise RuntimeError("tls_amd: %s implements ABI version %d, this binding expects %d (struct layouts differ): "
                           "rebuild with `make -C tls_amd/csrc`" % (LIB_PATH, lib.tls_abi_version(), ABI_VERSION))
    lib.tls_device_count.restype = ci
    lib.tls_ctx_create.restype = vp
    lib.tls_ctx_create.argtypes = [ci]
    lib.tls_ctx_destroy.restype = None
    lib.tls_ctx_destroy.argtypes = [vp]
    lib.tls_last_error.restype = ctypes.c_char_p
    lib.tls_last_error.argtypes = [vp]
    lib.tls_version.restype = ctypes.c_char_p
    lib.tls_device_name.restype = ctypes.c_char_p
    lib.tls_device_name.argtypes = [vp]
    lib.tls_get_options.restype = ci
    lib.tls_get_options.argtypes = [vp, ctypes.POINTER(Options)]
    lib.tls_set_options.restype = ci
    lib.tls_set_options.argtypes = [vp, ctypes.POINTER(Options)]
    lib.tls_debug_set_switch.restype = ci
    lib.tls_debug_set_switch.argtypes = [vp, ctypes.c_char_p, dbl]
    lib.tls_debug_get_switches.restype = ci
    lib.tls_debug_get_switches.argtypes = [vp, ctypes.c_char_p, i64]
    tp, pp = ctypes.POINTER(_Template), ctypes.POINTER(_Params)
    cp = ctypes.POINTER(Counters)
    lib.tls_search.restype = ci
    lib.tls_search.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, _c_double_p, i64,
                               tp, pp, _c_double_p, _c_int64_p, _c_double_p, cp]
    lib.tls_search_batch.restype = ci
    lib.tls_search_batch.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, i64,
                                     tp, pp, _c_double_p, _c_int64_p, _c_double_p]
    lib.tls_power_batch.restype = ci
    lib.tls_power_batch.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, i64,
                                    tp, pp, i64, ctypes.c_void_p, _c_double_p, _c_int64_p, _c_double_p, _c_double_p,
                                    _c_double_p, _c_double_p]
    lib.tls_prepare.restype = ci
    lib.tls_prepare.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, _c_double_p, i64,
                                tp, pp]
    lib.tls_update_flux.restype = ci
    lib.tls_update_flux.argtypes = [vp, _c_double_p, _c_double_p]
    lib.tls_execute.restype = ci
    lib.tls_execute.argtypes = [vp, ci]
    lib.tls_synchronize.restype = ci
    lib.tls_synchronize.argtypes = [vp]
    lib.tls_fetch.restype = ci
    lib.tls_fetch.argtypes = [vp, _c_double_p, _c_int64_p, _c_double_p, cp]
    lib.tls_execute_timed.restype = ci
    lib.tls_execute_timed.argtypes = [vp, ci, _c_double_p]
    lib.tls_last_kernel.restype = ctypes.c_char_p
    lib.tls_last_kernel.argtypes = [vp]
    lib.tls_plan_info.restype = ci
    lib.tls_plan_info.argtypes = [vp, cp, _c_int64_p, _c_int64_p, _c_int64_p]
    lib.tls_kernel_timing.restype = ci
    lib.tls_kernel_timing.argtypes = [vp, ci, _c_double_p, _c_int64_p]
    lib.tls_debug_phase_cycles.restype = ci
    lib.tls_debug_phase_cycles.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ci]
    lib.tls_debug_poison_lds.restype = ci
    lib.tls_debug_poison_lds.argtypes = [vp, ctypes.c_uint32]
    lib.tls_debug_check_counts.restype = ci
    lib.tls_debug_check_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ci]
    lib.tls_t0_fit.restype = ci
    lib.tls_t0_fit.argtypes = [vp, _c_double_p, _c_double_p, i64, dbl, _c_double_p, i64, _c_double_p,
                               i64, i64, _c_double_p]
    lib.tls_pink_noise.restype = ci
    lib.tls_pink_noise.argtypes = [vp, _c_double_p, i64, i64, ctypes.c_double, _c_double_p]
    lib.tls_spectra.restype = ci
    lib.tls_spectra.argtypes = [vp, _c_double_p, i64, i64, _c_double_p, _c_double_p, _c_double_p, _c_double_p]
    lib.tls_debug_folded.restype = ci
    lib.tls_debug_folded.argtypes = [vp, _c_double_p, i64]
    lib.tls_debug_prefix.restype = ci
    lib.tls_debug_prefix.argtypes = [vp, _c_double_p, i64, ctypes.POINTER(ctypes.c_int64)]
    lib.tls_debug_period_cycles.restype = ci
    lib.tls_debug_period_cycles.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), i64]
    lib.tls_debug_batch_group_ms.restype = ci
    lib.tls_debug_batch_group_ms.argtypes = [vp, _c_double_p, i64]
    lib.tls_debug_post_search.restype = ci
    lib.tls_debug_post_search.argtypes = [vp, _c_double_p, i64, _c_double_p, _c_int64_p, _c_double_p, i64, ctypes.c_void_p,
                                          _c_double_p, _c_double_p, _c_int64_p, _c_int64_p]
    lib.tls_power_batch_stats.restype = ci
    lib.tls_power_batch_stats.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, i64,
                                          tp, pp, i64, ctypes.c_void_p, _c_double_p, _c_int64_p, _c_double_p, _c_double_p,
                                          _c_double_p, _c_double_p, _c_double_p, dbl, _c_double_p, _c_double_p, i64,
                                          ctypes.c_void_p, i64, _c_double_p, _c_int64_p]
    lib.tls_debug_transit_stats.restype = ci
    lib.tls_debug_transit_stats.argtypes = [vp, _c_double_p, i64, _c_double_p, _c_double_p, _c_int64_p, _c_double_p, _c_int64_p,
                                            _c_int64_p, _c_double_p, _c_double_p, i64, dbl, _c_double_p, _c_double_p, i64, i64,
                                            ctypes.c_void_p,
                                            _c_double_p, _c_int64_p]
    models = [_c_double_p, _c_double_p, i64, dbl, dbl, dbl, i64, _c_double_p, _c_double_p, _c_double_p, _c_int64_p]
    lib.tls_power_batch_models.restype = ci
    lib.tls_power_batch_models.argtypes = lib.tls_power_batch_stats.argtypes + models
    lib.tls_debug_transit_models.restype = ci
    lib.tls_debug_transit_models.argtypes = lib.tls_debug_transit_stats.argtypes + models
    lib.tls_inject_transits.restype = ci
    lib.tls_inject_transits.argtypes = [vp, _c_double_p, i64, _c_double_p, i64, ctypes.POINTER(Injection), i64, dbl, dbl,
                                        _c_double_p, _c_int64_p]
    u64 = ctypes.c_uint64
    lib.tls_null_rows.restype = ci
    lib.tls_null_rows.argtypes = [vp, i64, i64, u64, i64, ci, _c_double_p, i64, _c_double_p, i64, i64, _c_double_p]
    lib.tls_debug_null_words.restype = ci
    lib.tls_debug_null_words.argtypes = [vp, i64, i64, u64, i64, ci, i64, ctypes.POINTER(u64)]
    lib.tls_medfilt_detrend.restype = ci
    lib.tls_medfilt_detrend.argtypes = [vp, _c_double_p, i64, i64, i64, _c_double_p, _c_double_p]
    lib.tls_biweight_detrend.restype = ci
    lib.tls_biweight_detrend.argtypes = [vp, _c_double_p, _c_double_p, i64, i64, ctypes.c_double, ctypes.c_double,
                                         _c_double_p, _c_double_p]
    lib.tls_sysrem.restype = ci
    lib.tls_sysrem.argtypes = [vp, _c_double_p, _c_double_p, i64, i64, i64, i64, ctypes.c_double, _c_double_p, _c_double_p,
                               _c_double_p, _c_double_p, _c_int64_p]
    peaks = [i64, dbl, _c_double_p, i64, dbl, ctypes.c_void_p, _c_int64_p]
    lib.tls_find_peaks.restype = ci
    lib.tls_find_peaks.argtypes = [vp, _c_double_p, _c_double_p, _c_int64_p, _c_double_p, i64, i64, _c_double_p] + peaks
    lib.tls_power_batch_peaks.restype = ci
    lib.tls_power_batch_peaks.argtypes = lib.tls_power_batch_stats.argtypes + peaks
    lib.tls_power_batch_peak_fits.restype = ci
    lib.tls_power_batch_peak_fits.argtypes = lib.tls_power_batch_peaks.argtypes + [ctypes.c_void_p]
    lib.tls_power_batch_phase_scan.restype = ci
    lib.tls_power_batch_phase_scan.argtypes = lib.tls_power_batch_peak_fits.argtypes + [i64, i64, ctypes.c_void_p]
    lib.tls_phase_scan.restype = ci
    lib.tls_phase_scan.argtypes = [vp, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_double_p, _c_double_p, _c_double_p,
                                   i64, i64, i64, ctypes.c_void_p]
    lib.tls_single_transits.restype = ci
    lib.tls_single_transits.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, _c_int64_p, _c_int64_p,
                                        _c_double_p, i64, dbl, i64, dbl, dbl, ctypes.c_void_p, _c_int64_p, _c_double_p,
                                        _c_int64_p, _c_double_p]
    lib.tls_transit_times.restype = ci
    lib.tls_transit_times.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_double_p, _c_double_p,
                                      _c_int64_p, _c_int64_p, i64, _c_double_p, _c_int64_p, _c_int64_p, _c_double_p, i64, dbl,
                                      dbl, i64, ctypes.c_void_p, ctypes.c_void_p]
    lib.tls_event_periods.restype = ci
    lib.tls_event_periods.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_int64_p, _c_int64_p,
                                      _c_int64_p, _c_int64_p, _c_double_p, i64, _c_double_p, _c_int64_p, _c_int64_p, _c_double_p,
                                      i64, dbl, i64, dbl, dbl, ctypes.c_void_p, ctypes.c_void_p]
    lib.tls_event_vetting.restype = ci
    lib.tls_event_vetting.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_double_p, _c_double_p,
                                      _c_int64_p, _c_int64_p, _c_int64_p, _c_int64_p, _c_double_p, i64, _c_double_p, _c_int64_p,
                                      _c_int64_p, _c_double_p, i64, dbl, dbl, dbl, dbl, dbl, dbl, i64, ctypes.c_void_p,
                                      ctypes.c_void_p]
    lib.tls_folded_views.restype = ci
    lib.tls_folded_views.argtypes = [vp, _c_double_p, _c_double_p, i64, i64, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                     _c_int64_p, i64, i64, i64, ctypes.c_double, ctypes.c_double, vp, _c_double_p, vp,
                                     _c_double_p, vp]
    lib.tls_shape_fit.restype = ci
    lib.tls_shape_fit.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, _c_double_p, _c_double_p,
                                  _c_int64_p, i64, _c_double_p, i64, _c_double_p, i64, _c_double_p, i64, dbl, i64, dbl,
                                  ctypes.c_void_p]
    lib.tls_transit_fit.restype = ci
    lib.tls_transit_fit.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_double_p, _c_double_p,
                                    _c_double_p, _c_int64_p, i64, _c_double_p, _c_double_p, i64, i64, _c_double_p, i64,
                                    _c_double_p, i64, _c_double_p, i64, _c_double_p, i64, dbl, i64, dbl, ctypes.c_void_p]
    lib.tls_centroid_test.restype = ci
    lib.tls_centroid_test.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p,
                                      _c_double_p, _c_double_p, _c_int64_p, i64, _c_double_p, i64, dbl, i64, i64, i64,
                                      ctypes.c_void_p]
    lib.tls_nudft.restype = ci
    lib.tls_nudft.argtypes = [vp, _c_double_p, i64, i64, _c_double_p, _c_double_p, i64, _c_double_p]
    lib.tls_lomb_scargle.restype = ci
    lib.tls_lomb_scargle.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, i64, _c_double_p,
                                     _c_double_p, _c_double_p, _c_double_p, _c_double_p, i64, dbl, ctypes.c_void_p, _c_int64_p,
                                     _c_double_p, _c_double_p, _c_double_p]
    lib.tls_sine_test.restype = ci
    lib.tls_sine_test.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, _c_double_p, _c_double_p,
                                  _c_int64_p, i64, _c_double_p, i64, dbl, ctypes.c_void_p, ctypes.c_void_p, _c_double_p]
    lib.tls_prewhiten.restype = ci
    lib.tls_prewhiten.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, i64, i64, _c_double_p, i64, i64, i64, dbl,
                                  _c_double_p, _c_double_p, ctypes.c_void_p, _c_int64_p, _c_double_p, _c_double_p, _c_double_p]
    lib.tls_ephemeris_match.restype = ci
    lib.tls_ephemeris_match.argtypes = [vp, _c_int64_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, i64, dbl, dbl, dbl,
                                        i64, ctypes.c_void_p]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.tls_transit_mask.restype = ci
    lib.tls_transit_mask.argtypes = [vp, _c_double_p, i64, _c_int64_p, _c_double_p, _c_double_p, _c_double_p, i64, dbl, i64, u8p]
    lib.tls_biweight_detrend_masked.restype = ci
    lib.tls_biweight_detrend_masked.argtypes = [vp, _c_double_p, _c_double_p, u8p, i64, i64, dbl, dbl, i64, _c_double_p,
                                                _c_double_p, u8p]
    lib.tls_prewhiten_masked.restype = ci
    lib.tls_prewhiten_masked.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, u8p, i64, i64, _c_double_p, i64, i64, i64, dbl,
                                         _c_double_p, _c_double_p, ctypes.c_void_p, _c_int64_p, _c_double_p, _c_double_p,
                                         _c_double_p]
    lib.tls_remove_transits.restype = ci
    lib.tls_remove_transits.argtypes = [vp, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_double_p, _c_double_p, _c_int64_p,
                                        _c_double_p, _c_double_p, _c_double_p, _c_double_p, i64, _c_double_p, _c_double_p, i64,
                                        i64, _c_double_p, i64, _c_double_p, _c_double_p, _c_double_p]
    lib.tls_noise_profile.restype = ci
    lib.tls_noise_profile.argtypes = [vp, _c_double_p, _c_double_p, i64, i64, _c_int64_p, _c_double_p, i64, dbl, dbl, dbl, i64,
                                      ctypes.c_void_p, _c_int64_p, _c_double_p, _c_double_p]
    lib.tls_decorrelate.restype = ci
    lib.tls_decorrelate.argtypes = [vp, _c_double_p, _c_double_p, u8p, i64, i64, _c_double_p, i64, _c_double_p, i64, _c_int64_p,
                                    i64, dbl, i64, dbl, dbl, _c_double_p, _c_double_p, ctypes.c_void_p, _c_double_p, _c_double_p,
                                    _c_double_p]
    lib.tls_spline_detrend.restype = ci
    lib.tls_spline_detrend.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p, u8p, i64, i64, _c_double_p, i64, dbl, dbl, i64, dbl,
                                       dbl, _c_double_p, _c_double_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.tls_clean_rows.restype = ci
    lib.tls_clean_rows.argtypes = [vp, _c_double_p, _c_double_p, u8p, i64, i64, dbl, dbl, dbl, dbl, i64, i64, i64, _c_double_p, u8p,
                                   ctypes.c_void_p]
    lib.tls_debug_peak_phase_scans.restype = ci
    lib.tls_debug_peak_phase_scans.argtypes = [vp, _c_double_p, i64, ctypes.c_void_p, _c_int64_p, i64, _c_double_p, _c_double_p,
                                               i64, dbl, _c_double_p, _c_double_p, i64, i64, ctypes.c_void_p, i64, i64,
                                               ctypes.c_void_p]
    lib.tls_debug_peak_fits.restype = ci
    lib.tls_debug_peak_fits.argtypes = [vp, _c_double_p, i64, ctypes.c_void_p, _c_int64_p, i64, _c_double_p, _c_double_p, i64,
                                        dbl, _c_double_p, _c_double_p, i64, i64, ctypes.c_void_p, _c_double_p, _c_double_p,
                                        _c_int64_p]
    lib.tls_debug_device_bytes.restype = ci
    lib.tls_debug_device_bytes.argtypes = [vp, _c_int64_p, _c_int64_p]
    lib.tls_debug_perm_table.restype = ci
    lib.tls_debug_perm_table.argtypes = [vp, _c_int64_p, _c_int64_p, _c_int64_p]
    if hasattr(lib, "tls_debug_lanes"):   # (an A/B run against a library built from older sources has none)
        lib.tls_debug_lanes.restype = ci
        lib.tls_debug_lanes.argtypes = [vp, _c_int64_p, _c_int64_p, _c_int64_p]
        lib.tls_debug_launch_ms.restype = ci
        lib.tls_debug_launch_ms.argtypes = [vp, _c_double_p, i64]
    lib.tls_debug_cumsum.restype = ci
    lib.tls_debug_cumsum.argtypes = [vp, _c_double_p, i64, _c_double_p, ci]
    lib.tls_grid_cells.restype = ci
    lib.tls_grid_cells.argtypes = [_c_double_p, i64, _c_double_p, i64, tp, pp, _c_int64_p]
    lib.tls_debug_candidate_slabs.restype = ci
    lib.tls_debug_candidate_slabs.argtypes = [_c_int64_p, i64, i64, i64, _c_int64_p, _c_int64_p, _c_int64_p, _c_int64_p]
    lib.tls_period_costs.restype = ci
    lib.tls_period_costs.argtypes = [_c_double_p, i64, _c_double_p, i64, tp, pp, dbl, _c_int64_p, _c_double_p, _c_double_p,
                                     _c_int64_p, ctypes.c_char_p]
    lib.tls_comm_unique_id.restype = ci
    lib.tls_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.tls_comm_init.restype = ci
    lib.tls_comm_init.argtypes = [vp, ci, ci, ctypes.c_char_p]
    lib.tls_comm_destroy.restype = ci
    lib.tls_comm_destroy.argtypes = [vp]
    lib.tls_comm_info.restype = ci
    lib.tls_comm_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.tls_comm_allgather_results.restype = ci
    lib.tls_comm_allgather_results.argtypes = [vp, i64, _c_double_p, _c_int64_p, _c_double_p]
    lib.tls_comm_allgather_device.restype = ci
    lib.tls_comm_allgather_device.argtypes = [vp, i64]
    lib.tls_comm_fetch_gathered.restype = ci
    lib.tls_comm_fetch_gathered.argtypes = [vp, i64, _c_double_p, _c_int64_p, _c_double_p]
    lib.tls_comm_stage_results.restype = ci
    lib.tls_comm_stage_results.argtypes = [vp, i64, i64, i64]
    lib.tls_comm_allgather_staged.restype = ci
    lib.tls_comm_allgather_staged.argtypes = [vp, i64, i64]
    lib.tls_comm_fetch_staged.restype = ci
    lib.tls_comm_fetch_staged.argtypes = [vp, i64, i64, i64, _c_double_p, _c_int64_p, _c_double_p]
    lib.tls_comm_barrier.restype = ci
    lib.tls_comm_barrier.argtypes = [vp]
    lib.tls_comm_max.restype = ci
    lib.tls_comm_max.argtypes = [vp, _c_double_p]
    _lib = lib
    return lib


def medfilt_kernel(kernel, n):
    """The kernel size as an int, checked as tls_medfilt_detrend checks it for rows of n points; ValueError for an even
    size, one < 1, > n or > MEDFILT_MAX_KERNEL, and a non-integer or bool (scipy.signal.medfilt only warns for a kernel
    larger than the row, and returns zeros in the trend there)."""
    if isinstance(kernel, (bool, numpy.bool_)):
        raise ValueError("the kernel size must be an odd integer, got %r" % (kernel,))
    try:
        k = operator.index(kernel)
    except TypeError:
        raise ValueError("the kernel size must be an odd integer, got %r" % (kernel,))
    if k < 1 or k % 2 == 0:
        raise ValueError("the kernel size must be odd and >= 1, got %d" % k)
    if k > n:
        raise ValueError("the kernel size %d exceeds the %d points of a row" % (k, n))
    if k > MEDFILT_MAX_KERNEL:
        raise ValueError("the kernel size %d exceeds MEDFILT_MAX_KERNEL = %d" % (k, MEDFILT_MAX_KERNEL))
    return k


def medfilt_arguments(y, kernel):
    """(rows [n_rows, n] float64, kernel) from y [n] or [n_rows, n], checked as tls_medfilt_detrend checks them
    (medfilt_kernel; every value finite and > 0); ValueError otherwise."""
    rows = numpy.asarray(y, dtype=numpy.float64)
    if rows.ndim == 1:
        rows = rows[None, :]
    if rows.ndim != 2 or not 1 <= rows.shape[1] <= 100000000:
        raise ValueError("flux must have shape [n] or [n_rows, n] with n in [1, 1e8], got %s" % (numpy.shape(y),))
    k = medfilt_kernel(kernel, rows.shape[1])
    _checks.positive_values(None, rows, "flux", "the median filter")
    return numpy.ascontiguousarray(rows), k


def _days(name, value, allow_inf):
    """value as a float, > 0 and finite (or +inf where allow_inf); ValueError otherwise (a bool or a non-number included)."""
    _checks.real(None, name, value, "must be a number of days")
    return _checks.positive(None, name, value, "must be > 0") if allow_inf else _checks.finite_positive(None, name, value)


def biweight_windows(t, window_length, break_tolerance):
    """(t, window_length, break_tolerance, lo, hi), checked as tls_biweight_detrend checks them: t 1-D with n in [1, 1e8]
    points, finite and non-decreasing; window_length finite and > 0; break_tolerance > 0 (inf: never split).  [lo[i], hi[i])
    is the window of point i: every j of i's segment (a new one starts at every t[j] - t[j-1] > break_tolerance) with
    abs(t[j] - t[i]) <= 0.5 * window_length, found by bisection with that exact test.  ValueError for a bad argument and for
    a window of more than BIWEIGHT_MAX_WINDOW points."""
    wl = _days("window_length", window_length, False)
    bt = _days("break_tolerance", break_tolerance, True)
    t = _checks.times(None, t, _checks.MAX_ROW_POINTS)
    n = len(t)
    idx = numpy.arange(n)
    brk = numpy.ones(n, dtype=bool)
    brk[1:] = (t[1:] - t[:-1]) > bt
    starts = numpy.flatnonzero(brk)
    seg = numpy.cumsum(brk) - 1
    seg_lo, seg_hi = starts[seg], numpy.append(starts[1:], n)[seg]
    half = 0.5 * wl

    def bisect(a, b, first_false):
        # the first j in [a, b) where the test fails (first_false), or the first where it holds; b where there is none
        while True:
            act = a < b
            if not act.any():
                return a
            mid = (a + b) // 2
            ok = numpy.abs(t[numpy.minimum(mid, n - 1)] - t) <= half
            go_right = ok if first_false else ~ok
            a = numpy.where(act & go_right, mid + 1, a)
            b = numpy.where(act & ~go_right, mid, b)

    lo = bisect(seg_lo, idx, False)
    hi = bisect(idx + 1, seg_hi, True)
    widest = int((hi - lo).max())
    if widest > BIWEIGHT_MAX_WINDOW:
        raise ValueError("a window holds %d points, more than BIWEIGHT_MAX_WINDOW = %d" % (widest, BIWEIGHT_MAX_WINDOW))
    return t, wl, bt, lo, hi


def biweight_arguments(t, y, window_length, break_tolerance):
    """(t, rows [n_rows, n] float64, window_length, break_tolerance) from y [n] or [n_rows, n] at the time stamps t [n],
    checked as tls_biweight_detrend checks them (biweight_windows; every flux value finite and > 0); ValueError otherwise."""
    t, wl, bt, _, _ = biweight_windows(t, window_length, break_tolerance)
    rows = numpy.asarray(y, dtype=numpy.float64)
    if rows.ndim == 1:
        rows = rows[None, :]
    if rows.ndim != 2 or rows.shape[1] != len(t):
        raise ValueError("flux must have shape [n] or [n_rows, n] with n = len(t) = %d, got %s" % (len(t), numpy.shape(y)))
    _checks.positive_values(None, rows, "flux", "the biweight filter")
    return t, numpy.ascontiguousarray(rows), wl, bt


def detrend_mask_rows(mask, shape, what="mask"):
    """mask as contiguous uint8 rows of `shape` ([n_rows, n]; a [n] mask serves one row): a uint8 or bool array, any byte
    other than 0 protected.  ValueError for another dtype or shape.  GPU-free."""
    rows = numpy.asarray(mask)
    if rows.dtype != numpy.uint8 and rows.dtype != numpy.bool_:
        raise ValueError("%s must be a uint8 or bool array, got dtype %s" % (what, rows.dtype))
    if rows.ndim == 1 and shape[0] == 1:
        rows = rows[None, :]
    if rows.shape != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), numpy.shape(mask)))
    return numpy.ascontiguousarray(rows.view(numpy.uint8) if rows.dtype == numpy.bool_ else rows)


def _min_points(min_points):
    return _checks.integer(None, "min_points", min_points, 1, 2 ** 31 - 1, "must be an integer >= 1")


def biweight_masked_arguments(t, y, mask, window_length, break_tolerance, min_points=3):
    """(t, rows, mask rows uint8, window_length, break_tolerance, min_points), checked as tls_biweight_detrend_masked checks
    them: biweight_arguments, a mask of the rows' shape (detrend_mask_rows) and min_points an integer >= 1.  ValueError
    otherwise.  GPU-free."""
    t, rows, wl, bt = biweight_arguments(t, y, window_length, break_tolerance)
    return t, rows, detrend_mask_rows(mask, rows.shape), wl, bt, _min_points(min_points)


def transit_mask_arguments(t, period, T0, duration, curve=None, n_curves=None, factor=1.5):
    """What tls_transit_mask takes, checked as it checks them: a dict with t [n] (n in [1, 1e8], finite), period, T0 and
    duration [m] (any values: a candidate that is not finite and > 0 takes no part), curve (None: candidate k belongs to curve
    k; integers in [0, n_curves)), n_curves (None: m without curve, max(curve) + 1 with) and factor (finite, > 0).  ValueError
    otherwise.  GPU-free."""
    try:
        t = numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64))
        period, T0, duration = (numpy.ascontiguousarray(numpy.atleast_1d(numpy.asarray(v, dtype=numpy.float64)))
                                for v in (period, T0, duration))
    except (TypeError, ValueError):
        raise ValueError("transit mask: t, period, T0 and duration must hold numbers")
    t = _checks.times("transit mask", t, _checks.MAX_ROW_POINTS, order=None)
    if period.ndim != 1 or not period.shape == T0.shape == duration.shape:
        raise ValueError("transit mask: period, T0 and duration must have one shape [m], got %s, %s, %s"
                         % (period.shape, T0.shape, duration.shape))
    m = len(period)
    if curve is not None:
        curve = numpy.asarray(curve)
        if curve.shape != (m,) or (m and curve.dtype.kind not in "iu"):
            raise ValueError("transit mask: curve must hold %d integers, got shape %s dtype %s" % (m, curve.shape, curve.dtype))
        curve = numpy.ascontiguousarray(curve, dtype=numpy.int64)
    if n_curves is None:
        n_curves = m if curve is None else (int(curve.max()) + 1 if m else 0)
    n_curves = _checks.integer("transit mask", "n_curves", n_curves, 0)
    if (curve is None and m > n_curves) or (curve is not None and m and not (0 <= curve.min() and curve.max() < n_curves)):
        raise ValueError("transit mask: curve out of range [0, n_curves = %d)" % n_curves)
    factor = _checks.finite_positive("transit mask", "factor", factor)
    return dict(t=t, period=period, T0=T0, duration=duration, curve=curve, n_curves=n_curves, factor=factor)


REMOVE_TRANSITS_FIELDS = ("period", "T0", "fit_row", "fit_amplitude", "fit_b", "fit_duration", "fit_shift")


def remove_transits_arguments(t, y, period, T0, row, amplitude, b, duration, shift, k_rows, profile, sub, curve=None):
    """What tls_remove_transits takes, checked as it checks them and packed for it -- a dict with t [n] (n in [1, 1e8], finite
    and non-decreasing), y [n_curves, n] (one row [n] serves one curve), period, T0, amplitude, b, duration, shift [n_fits]
    (any values: a candidate that cannot take part is skipped), row [n_fits] whole numbers in [0, nK) (integers, or the doubles
    of a transit-fit record; a NaN row belongs to a candidate that is skipped and is sent as row 0), curve [n_fits] int64 in
    [0, n_curves) (None: candidate f belongs to curve f) and k_rows, profile, sub as transit_fit_tables checks them.
    ValueError otherwise.  GPU-free."""
    what = "remove transits"
    tables = transit_fit_tables(k_rows, profile, [0.0], [1.0], [0.0], sub, what=what)
    k_rows, profile, sub = tables[0], tables[1], tables[5]
    no_numbers = "t, y and the candidates' columns must hold numbers"
    try:
        t = numpy.ascontiguousarray(numpy.asarray(t, dtype=numpy.float64))
        y = numpy.asarray(y, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise _checks.refusal(what, no_numbers)
    columns = _checks.floats(what, (period, T0, amplitude, b, duration, shift), no_numbers)
    if y.ndim == 1:
        y = y[None, :]
    if t.ndim != 1 or y.ndim != 2 or y.shape[1] != len(t) or not 1 <= len(t) <= _checks.MAX_ROW_POINTS:
        raise _checks.over_t(what, "y", " with n in [1, 1e8], got %s over %s" % (y.shape, t.shape))
    _checks.time_values(what, t)
    n_fits = len(columns[0])
    if any(v.ndim != 1 or len(v) != n_fits for v in columns):
        raise _checks.refusal(what, "period, T0, amplitude, b, duration and shift must have one shape [n_fits], got %s"
                              % ([v.shape for v in columns],))
    no_row = _checks.refusal(what, "row must hold one row in [0, %d) a candidate" % len(k_rows))
    rows = numpy.atleast_1d(numpy.asarray(row))
    if rows.shape != (n_fits,) or (n_fits and rows.dtype.kind not in "iuf"):
        raise no_row
    if rows.dtype.kind == "f":
        with numpy.errstate(all="ignore"):
            known = numpy.isfinite(rows)
            if not numpy.all(rows[known] == numpy.floor(rows[known])) or not numpy.all(numpy.abs(rows[known]) < 2.0 ** 31):
                raise no_row
            columns[2] = numpy.where(known, columns[2], numpy.nan)       # (no row: no candidate)
            rows = numpy.where(known, rows, 0.0)
    rows = numpy.ascontiguousarray(rows, dtype=numpy.int64)
    if n_fits and (rows.min() < 0 or rows.max() >= len(k_rows)):
        raise no_row
    if curve is not None:
        curve = numpy.asarray(curve)
        if curve.shape != (n_fits,) or (n_fits and curve.dtype.kind not in "iu"):
            raise _checks.refusal(what, "curve must hold %d integers, got shape %s dtype %s" % (n_fits, curve.shape, curve.dtype))
        curve = numpy.ascontiguousarray(curve, dtype=numpy.int64)
    in_range = n_fits <= y.shape[0] if curve is None else not n_fits or (0 <= curve.min() and curve.max() < y.shape[0])
    if not in_range:
        raise _checks.refusal(what, "curve out of range [0, n_curves = %d)" % y.shape[0])
    names = ("period", "T0", "amplitude", "b", "duration", "shift")
    return dict(dict(zip(names, (numpy.ascontiguousarray(v) for v in columns))), t=t, y=numpy.ascontiguousarray(y), row=rows,
                curve=curve, k_rows=k_rows, profile=profile, sub=sub)


def _sysrem_integer(name, value, low, high, what):
    """value as an int in [low, high]; ValueError otherwise (a bool or a non-integer included)."""
    return _checks.index(None, name, value, low, high, what)


def sysrem_arguments(y, n_components=1, dy=None, max_iter=50, tol=1e-6):
    """(rows [n_rows, n] float64, dy rows or None, n_components, max_iter, tol), checked as tls_sysrem checks them: y
    [n_rows, n] with n_rows >= 2 and n in [1, 1e8]; n_components an integer in [1, min(SYSREM_MAX_COMPONENTS, n_rows - 1)];
    max_iter an integer in [1, SYSREM_MAX_ITER]; tol finite and >= 0; every y value, and every dy value of a dy (None, or
    the shape of y), finite and > 0.  ValueError otherwise."""
    rows = numpy.asarray(y, dtype=numpy.float64)
    if rows.ndim != 2 or rows.shape[0] < 2 or not 1 <= rows.shape[1] <= 100000000:
        raise ValueError("flux must have shape [n_rows, n] with n_rows >= 2 (SysRem fits across the rows) and n in [1, 1e8], "
                         "got %s" % (numpy.shape(y),))
    k = _sysrem_integer("n_components", n_components, 1, min(SYSREM_MAX_COMPONENTS, rows.shape[0] - 1),
                        "min(SYSREM_MAX_COMPONENTS = %d, n_rows - 1 = %d)" % (SYSREM_MAX_COMPONENTS, rows.shape[0] - 1))
    iters = _sysrem_integer("max_iter", max_iter, 1, SYSREM_MAX_ITER, "SYSREM_MAX_ITER = %d" % SYSREM_MAX_ITER)
    tol = _checks.finite_at_least(None, "tol", _checks.real(None, "tol", tol))
    _checks.positive_values(None, rows, "flux", "SysRem")
    if dy is not None:
        dy = numpy.asarray(dy, dtype=numpy.float64)
        if dy.shape != rows.shape:
            raise ValueError("dy must be None or have the shape of flux %s, got %s" % (rows.shape, dy.shape))
        _checks.positive_values(None, dy, "dy", "SysRem")
        dy = numpy.ascontiguousarray(dy)
    return numpy.ascontiguousarray(rows), dy, k, iters, tol


# tls_decor_fit of include/tls_amd.h, in order: all doubles
DECOR_FIELDS = ("status", "dropped", "n_fit", "n_clipped", "rounds", "mu", "sigma", "n_live")


class DecorFit(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in DECOR_FIELDS]


DECOR_DTYPE = numpy.dtype([(k, "f8") for k in DECOR_FIELDS])


def decorrelate_arguments(y, own=None, shared=None, dy=None, mask=None, segments=None, ridge=0.0, n_iter=3, sigma_upper=5.0,
                          sigma_lower=5.0):
    """What tls_decorrelate takes, checked as it checks them: a dict with y (float64 [n_curves, n], finite and > 0; one row
    becomes [1, n]), dy (None, or y's shape, finite and > 0), mask (None, or uint8 rows of y's shape: detrend_mask_rows),
    shared [n_shared, n] and own [n_curves, n_own, n] (finite, at least one given, n_shared + n_own in [1, DECOR_MAX_TERMS];
    for one row own may be [n_own, n]), segments (int64, ascending strictly from 0 to n; None: [0, n]), ridge (finite, >= 0),
    n_iter (an integer in [0, DECOR_MAX_ITER]) and sigma_upper, sigma_lower (> 0, inf allowed, no NaN).  ValueError otherwise.
    GPU-free."""
    what = "decorrelation"
    try:
        y = numpy.asarray(y, dtype=numpy.float64)
        dy = None if dy is None else numpy.asarray(dy, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise _checks.refusal(what, "the light curves and dy must hold numbers")
    single = y.ndim == 1
    y, dy = _checks.row_shapes(what, None, y, dy, names="flux" if dy is None else "flux and dy")
    n_c, n = y.shape
    if not 1 <= n <= _checks.MAX_ROW_POINTS:
        raise _checks.refusal(what, "n must lie in [1, 1e8], got %d" % n)
    _checks.positive_values(what, y, "flux", "decorrelation")
    if dy is not None:
        _checks.positive_values(what, dy, "dy", "decorrelation")
    shared, own = _checks.regressors(what, shared, own, n_c, n, DECOR_MAX_TERMS, single)
    return {"y": numpy.ascontiguousarray(y), "dy": None if dy is None else numpy.ascontiguousarray(dy),
            "mask": None if mask is None else detrend_mask_rows(mask, y.shape), "shared": shared, "own": own,
            "segments": _checks.segments(what, segments, n),
            "ridge": _checks.finite_at_least(what, "ridge", ridge),
            "n_iter": _checks.integer(what, "n_iter", n_iter, 0, DECOR_MAX_ITER),
            "sigma_upper": _checks.positive(what, "sigma_upper", sigma_upper),
            "sigma_lower": _checks.positive(what, "sigma_lower", sigma_lower), "single": single}


# tls_spline_segment and tls_spline_curve of include/tls_amd.h, in order: all doubles
SPLINE_SEGMENT_FIELDS = ("status", "intervals", "coefficients", "points", "kept", "rounds", "dropped", "sigma", "ssr", "weight")
SPLINE_CURVE_FIELDS = ("choice", "sigma_pp", "flag", "bic")
SPLINE_SEGMENT_DTYPE = numpy.dtype([(k, "f8") for k in SPLINE_SEGMENT_FIELDS])
SPLINE_CURVE_DTYPE = numpy.dtype([(k, "f8") for k in SPLINE_CURVE_FIELDS[:3]] + [("bic", "f8", (SPLINE_MAX_SPACINGS,))])


def spline_arguments(t, y, knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0, sigma_lower=3.0,
                     dy=None, mask=None):
    """What tls_spline_detrend takes, checked as it checks them: a dict with t (float64 [n], finite and non-decreasing), y
    (float64 [n_curves, n] over t, finite and > 0; one row becomes [1, n]), dy (None, or y's shape, finite and > 0), mask
    (None, or uint8 rows of y's shape: detrend_mask_rows), spacings (float64 [k], k in [1, SPLINE_MAX_SPACINGS], each finite
    and > 0), break_tolerance (> 0, inf allowed), penalty (finite, >= 0), n_iter (an integer in [0, SPLINE_MAX_ITER]),
    sigma_upper and sigma_lower (> 0, inf allowed, no NaN), segments (int64 [n_seg + 1]: a new segment behind every gap >
    break_tolerance; none may take more than SPLINE_MAX_COEF coefficients at any spacing), single (y was one row) and
    one_spacing (knot_spacing was one number).  ValueError otherwise.  GPU-free."""
    what = "spline detrending"
    t = _checks.times(what, t, _checks.MAX_ROW_POINTS)
    try:
        y = numpy.asarray(y, dtype=numpy.float64)
        dy = None if dy is None else numpy.asarray(dy, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise _checks.refusal(what, "the light curves and dy must hold numbers")
    single = y.ndim == 1
    y, dy = _checks.row_shapes(what, t, y, dy, names="flux" if dy is None else "flux and dy")
    _checks.positive_values(what, y, "flux", "spline detrending")
    if dy is not None:
        _checks.positive_values(what, dy, "dy", "spline detrending")
    spacing, one = _checks.spacings(what, knot_spacing, SPLINE_MAX_SPACINGS)
    bt = _checks.positive(what, "break_tolerance", break_tolerance)
    out = {"t": t, "y": numpy.ascontiguousarray(y), "dy": None if dy is None else numpy.ascontiguousarray(dy),
           "mask": None if mask is None else detrend_mask_rows(mask, y.shape), "spacings": spacing, "break_tolerance": bt,
           "penalty": _checks.finite_at_least(what, "penalty", penalty),
           "n_iter": _checks.integer(what, "n_iter", n_iter, 0, SPLINE_MAX_ITER),
           "sigma_upper": _checks.positive(what, "sigma_upper", sigma_upper),
           "sigma_lower": _checks.positive(what, "sigma_lower", sigma_lower), "single": single, "one_spacing": one}
    out["segments"] = _checks.knot_segments(what, t, bt, spacing, SPLINE_MAX_COEF)
    return out


# tls_clean_record of include/tls_amd.h, in order: all doubles
CLEAN_FIELDS = ("status", "n_missing", "n_bad", "n_high", "n_low", "n_filled", "longest_run", "rounds", "center", "sigma")
CLEAN_DTYPE = numpy.dtype([(k, "f8") for k in CLEAN_FIELDS])


def clean_arguments(t, y, window_length=None, break_tolerance=0.5, sigma_upper=4.0, sigma_lower=float("inf"), max_run=1, n_iter=3,
                    min_points=3, bad=None):
    """What tls_clean_rows takes, checked as it checks them: a dict with t (float64 [n], finite and non-decreasing), y (float64
    [n_curves, n] over t; ANY values, NaN and infinities included; one row becomes [1, n]), bad (None, or uint8 rows of y's
    shape: detrend_mask_rows), window_length (None: the row's median; else finite and > 0, no window over BIWEIGHT_MAX_WINDOW
    points), break_tolerance (> 0, inf allowed), sigma_upper and sigma_lower (> 0, inf allowed, no NaN), max_run (an integer
    >= 1), n_iter (an integer in [0, CLEAN_MAX_ITER]), min_points (an integer >= 1) and single (y was one row).  ValueError
    otherwise.  GPU-free."""
    what = "cleaning"
    t = _checks.times(what, t, _checks.MAX_ROW_POINTS)
    try:
        y = numpy.asarray(y, dtype=numpy.float64)
    except (TypeError, ValueError):
        raise _checks.refusal(what, "the light curves must hold numbers")
    single = y.ndim == 1
    y, _ = _checks.row_shapes(what, t, y, names="flux")
    bt = _checks.positive(what, "break_tolerance", break_tolerance)
    if window_length is not None:
        window_length = _checks.finite_positive(what, "window_length", window_length, "must be None or finite and > 0")
        try:
            biweight_windows(t, window_length, bt)
        except ValueError as e:
            raise _checks.refusal(what, str(e))
    return {"t": t, "y": numpy.ascontiguousarray(y), "bad": None if bad is None else detrend_mask_rows(bad, y.shape, "bad"),
            "window_length": window_length, "break_tolerance": bt,
            "sigma_upper": _checks.positive(what, "sigma_upper", sigma_upper),
            "sigma_lower": _checks.positive(what, "sigma_lower", sigma_lower),
            "max_run": _checks.integer(what, "max_run", max_run, 1, 2 ** 62),
            "n_iter": _checks.integer(what, "n_iter", n_iter, 0, CLEAN_MAX_ITER),
            "min_points": _checks.integer(what, "min_points", min_points, 1, 2 ** 31 - 1), "single": single}


def _f8(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64)


def _i8(a):
    return numpy.ascontiguousarray(a, dtype=numpy.int64)


def _root_count(root, root_count):
    """The second k ** 0.5 table of the statistics entries as float64: the caller's, or (None) stats.count_roots' own for as
    many counts as `root` covers."""
    if root_count is None:
        from .stats import count_roots
        return count_roots(len(root) - 1)[1]
    return _f8(root_count)


def _dp(a):
    return a.ctypes.data_as(_c_double_p)


def _ip(a):
    return a.ctypes.data_as(_c_int64_p)


class Context(object):
    """One GPU + one HIP stream (tls_ctx).  Not re-entrant."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = self._lib.tls_ctx_create(int(device))
        if not self._h:
            raise RuntimeError("tls_amd: cannot create a GPU context: "
                               + self._lib.tls_last_error(None).decode())
        self.device = int(device)
        self._n_periods = 0
        self._resident_chi2 = None   # (weak reference to the chi2 array the last fetch returned, generation): see holds
        self._generation = 0         # bumped by every call that launches a search or touches its inputs / result buffers

    # -- plumbing
    def close(self):
        if getattr(self, "_h", None):
            self._lib.tls_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError("tls_amd error %d: %s"
                               % (rc, self._lib.tls_last_error(self._h).decode()))

    @property
    def name(self):
        return self._lib.tls_device_name(self._h).decode()

    # -- switches (tls_options): the environment is read once per process, when the library is first used; a context
    #    starts with those values and changes them only through these calls
    def get_options(self):
        """Every switch of the context by name (the public tls_options and the developer switches): -1 = the library decides."""
        buf = ctypes.create_string_buffer(1024)
        rc = self._lib.tls_debug_get_switches(self._h, buf, len(buf))
        if rc != 0:
            raise RuntimeError("tls_amd error %d: tls_debug_get_switches" % rc)
        out = {}
        for item in buf.value.decode().split(","):
            k, _, v = item.partition("=")
            out[k] = float(v) if k == "band_max" else int(float(v))
        return out

    def set_options(self, **switches):
        """Set the named switches (None: back to "the library decides"); the others keep their values.  Drops a
        prepared plan: the next prepare()/search() plans again.  exact_prefix and slim go through the public
        tls_set_options, the developer switches through tls_debug_set_switch."""
        for k in switches:
            if k not in SWITCH_NAMES:
                raise TypeError("unknown switch %r (known: %s)" % (k, ", ".join(SWITCH_NAMES)))
        self._invalidate_results()
        public = {k: v for k, v in switches.items() if k in Options.NAMES}
        if public:
            o = Options()
            self._check(self._lib.tls_get_options(self._h, ctypes.byref(o)))
            for k, v in public.items():
                setattr(o, k, -1 if v is None else int(v))
            self._check(self._lib.tls_set_options(self._h, ctypes.byref(o)))
        for k, v in switches.items():
            if k not in Options.NAMES:
                self._check(self._lib.tls_debug_set_switch(self._h, k.encode(), -1.0 if v is None else float(v)))

    def reset_options(self):
        """Every switch back to "the library decides" (NOT to the process environment's values)."""
        self.set_options(**{k: None for k in SWITCH_NAMES})

    @staticmethod
    def _pack(table, params):
        arrays = (_f8(table.values), _i8(table.offset), _i8(table.length), _i8(table.width),
                  _f8(table.overshoot))
        tm = _Template(_dp(arrays[0]), _ip(arrays[1]), _ip(arrays[2]), _ip(arrays[3]),
                       _dp(arrays[4]), len(arrays[3]))
        pr = _Params(*[float(params[k]) for k in (
            "transit_depth_min", "R_star_min", "R_star_max", "M_star_min", "M_star_max",
            "T0_fit_margin")])
        return arrays, tm, pr

    # -- one-shot
    def search(self, t, y, dy, periods, table, params, count_work=False):
        """chi2, row, depth (and counters dict) for every period, in `periods` order.

        Consecutive searches on the same time stamps, period list, template table and parameters
        (a survey, or repeated power() calls) reuse the prepared plan: tls_prepare recognises them
        (byte comparison inside the library) and only replaces the flux and the weights."""
        self.prepare(t, y, dy, periods, table, params)
        self.execute(count_work=count_work)
        return self.fetch(with_counters=True)

    # -- staged
    def search_batch(self, t, y_batch, dy_batch, periods, table, params):
        """Survey mode: chi2, row, depth of shape [n_curves, n_periods] for light curves that share
        t, the grids and the template table (tls_search_batch)."""
        t, periods = _f8(t), _f8(periods)
        y_batch = numpy.ascontiguousarray(y_batch, dtype=numpy.float64)
        dy_batch = numpy.ascontiguousarray(dy_batch, dtype=numpy.float64)
        if y_batch.ndim != 2 or y_batch.shape != dy_batch.shape or y_batch.shape[1] != len(t):
            raise ValueError("y_batch and dy_batch must both have shape [n_curves, len(t)]")
        arrays, tm, pr = self._pack(table, params)
        n_c, n_p = y_batch.shape[0], len(periods)
        chi2 = numpy.empty((n_c, n_p), dtype=numpy.float64)
        row = numpy.empty((n_c, n_p), dtype=numpy.int64)
        depth = numpy.empty((n_c, n_p), dtype=numpy.float64)
        self._invalidate_results()
        self._check(self._lib.tls_search_batch(self._h, _dp(t), _dp(y_batch), _dp(dy_batch), len(t), n_c,
                                               _dp(periods), n_p, ctypes.byref(tm), ctypes.byref(pr),
                                               _dp(chi2), _ip(row), _dp(depth)))
        self._n_periods = n_p
        return chi2, row, depth

    def power_batch(self, t, y_batch, dy_batch, periods, table, params, median_kernel, with_arrays=False,
                    with_power=False, with_spectra=False):
        """Survey-mode power(): structured array (POWER_SUMMARY_DTYPE) with one record per light curve -- SDE,
        SDE_raw, chi2_min, period, T0, depth, the argmin/argmax indices, the template row -- from search,
        spectra and final T0 fit on the device (tls_power_batch); optionally the per-period arrays.
        with_spectra: also SR and power_raw (returned as two more arrays behind `power`)."""
        r = self._power_batch(t, y_batch, dy_batch, periods, table, params, median_kernel, with_arrays=with_arrays,
                              with_power=with_power, with_spectra=with_spectra)
        return tuple(r[k] for k in ("summary",) + PER_PERIOD_OUTPUTS[:4 + 2 * bool(with_spectra)])

    def power_batch_stats(self, t, y_batch, dy_batch, periods, table, params, median_kernel, fill_factor, root, max_epochs,
                          per_transit=False, with_arrays=False, with_spectra=False, models=None, lc_cap=0, root_count=None):
        """power_batch plus the per-transit statistics of every light curve (tls_power_batch_stats): (summary, stats
        (TRANSIT_STATS_DTYPE), per_transit [n_curves, 6, max_epochs] or None, n_epochs or None, chi2, row, depth, power).
        table.duration is the fractional duration of every template row; root and root_count are the two tables of
        stats.count_roots(len(t)): root[k] = float(k) ** 0.5 and root_count[k] = numpy.sum(k) ** 0.5, k = 0 .. len(t)
        (the entry reads as many entries as the shorter one has; root_count None: stats.count_roots' own, as long as root).
        with_spectra: SR and power_raw [n_curves, n_periods] follow.  models (a ModelTemplate): tls_power_batch_models, and
        (folded [n_curves, 3, n], model_folded [n_curves, n], lightcurve [n_curves, 2, lc_cap], lc_len [n_curves]) follow."""
        r = self._power_batch(t, y_batch, dy_batch, periods, table, params, median_kernel, with_arrays=with_arrays,
                              with_power=with_arrays, with_spectra=with_spectra,
                              statistics=(fill_factor, root, _root_count(root, root_count), max_epochs),
                              per_transit=per_transit, models=models, lc_cap=lc_cap)
        names = ("summary", "stats", "per_transit", "n_epochs") + PER_PERIOD_OUTPUTS[:4 + 2 * bool(with_spectra)]
        return tuple(r[k] for k in names + (MODEL_OUTPUTS if models is not None else ()))

    def _power_batch(self, t, y_batch, dy_batch, periods, table, params, median_kernel, with_arrays=False, with_power=False,
                     with_spectra=False, statistics=None, per_transit=False, models=None, lc_cap=0, peaks=None,
                     peak_fits=None, phase_scan=None):
        """The power-batch entries: tls_power_batch; with statistics = (fill_factor, root, root_count, max_epochs)
        tls_power_batch_stats; with models (a ModelTemplate) as well, tls_power_batch_models.  A dict of the outputs by name:
        summary; chi2, row, depth (with_arrays), power (with_power), SR and power_raw (with_spectra), None where not asked
        for; with statistics also stats, per_transit and n_epochs (None without per_transit); with models MODEL_OUTPUTS.
        peaks = (k, separation, ratios, min_power) (peaks_arguments): tls_power_batch_peaks, with or without statistics, and
        peaks (PEAK_DTYPE [n_curves, k]) and n_peaks [n_curves] as well; no entry carries peaks and models (ValueError).
        peak_fits = (fill_factor, root, root_count, max_epochs), with peaks only: tls_power_batch_peak_fits, and peak_fits
        (PEAK_FIT_DTYPE [n_curves, k]: T0, status and the statistics record of every peak) as well, with or without statistics.
        phase_scan = (max_bins, min_count), with peak_fits only: tls_power_batch_phase_scan, and phase_scans (PHASE_SCAN_DTYPE
        [n_curves, k]) as well."""
        if peaks is not None and models is not None:
            raise ValueError("peaks and models cannot be combined: no entry point carries both")
        if peak_fits is not None and peaks is None:
            raise ValueError("peak_fits needs peaks: the fits are those of the peaks")
        if phase_scan is not None and peak_fits is None:
            raise ValueError("phase_scan needs peak_fits: the scans read T0 and duration of the fits")
        if phase_scan is not None:
            phase_scan = phase_scan_arguments(*phase_scan)
        if peaks is not None:
            peaks = peaks_arguments(*peaks)
        t, periods = _f8(t), _f8(periods)
        y_batch = numpy.ascontiguousarray(y_batch, dtype=numpy.float64)
        dy_batch = numpy.ascontiguousarray(dy_batch, dtype=numpy.float64)
        if y_batch.ndim != 2 or y_batch.shape != dy_batch.shape or y_batch.shape[1] != len(t):
            raise ValueError("y_batch and dy_batch must both have shape [n_curves, len(t)]")
        arrays, tm, pr = self._pack(table, params)
        n_c, n_p = y_batch.shape[0], len(periods)
        out = {"summary": numpy.zeros(n_c, dtype=POWER_SUMMARY_DTYPE)}
        assert out["summary"].dtype.itemsize == ctypes.sizeof(PowerSummary)
        wanted = (with_arrays, with_arrays, with_arrays, with_power, with_spectra, with_spectra)
        for k, want in zip(PER_PERIOD_OUTPUTS, wanted):
            out[k] = numpy.empty((n_c, n_p), dtype=numpy.int64 if k == "row" else numpy.float64) if want else None
        args = [self._h, _dp(t), _dp(y_batch), _dp(dy_batch), len(t), n_c, _dp(periods), n_p, ctypes.byref(tm),
                ctypes.byref(pr), int(median_kernel), out["summary"].ctypes.data_as(ctypes.c_void_p)]
        args += [None if out[k] is None else _ip(out[k]) if k == "row" else _dp(out[k]) for k in PER_PERIOD_OUTPUTS]
        entry = self._lib.tls_power_batch
        if statistics is not None:
            fill_factor, root, root_count, max_epochs = statistics
            row_duration, root, root_count, max_epochs = _f8(table.duration), _f8(root), _f8(root_count), int(max_epochs)
            out["stats"] = numpy.zeros(n_c, dtype=TRANSIT_STATS_DTYPE)
            assert out["stats"].dtype.itemsize == ctypes.sizeof(TransitStats)
            out["per_transit"] = numpy.empty((n_c, len(PER_TRANSIT_FIELDS), max_epochs)) if per_transit else None
            out["n_epochs"] = numpy.empty(n_c, dtype=numpy.int64) if per_transit else None
            args += [_dp(row_duration), float(fill_factor), _dp(root), _dp(root_count), min(len(root), len(root_count)),
                     out["stats"].ctypes.data_as(ctypes.c_void_p), max_epochs,
                     None if out["per_transit"] is None else _dp(out["per_transit"]),
                     None if out["n_epochs"] is None else _ip(out["n_epochs"])]
            entry = self._lib.tls_power_batch_stats
            if models is not None:
                model_out = _model_outputs(n_c, len(t), lc_cap)
                out.update(zip(MODEL_OUTPUTS, model_out))
                args += models.args(lc_cap, model_out)
                entry = self._lib.tls_power_batch_models
        if peaks is not None:
            if statistics is None and peak_fits is not None:   # (out_stats NULL: the fits read the inputs all the same)
                fill_factor, root, root_count, max_epochs = peak_fits
                row_duration, root, root_count = _f8(table.duration), _f8(root), _f8(root_count)
                args += [_dp(row_duration), float(fill_factor), _dp(root), _dp(root_count),
                         min(len(root), len(root_count)), None, int(max_epochs), None, None]
            elif statistics is None:   # (out_stats NULL: no statistics, their inputs are not read)
                args += [None, 0.0, None, None, 0, None, 1, None, None]
            k, sep, ratios, low = peaks
            out["peaks"] = numpy.zeros((n_c, k), dtype=PEAK_DTYPE)
            assert PEAK_DTYPE.itemsize == ctypes.sizeof(Peak)
            out["n_peaks"] = numpy.zeros(n_c, dtype=numpy.int64)
            args += [k, sep, _dp(ratios), len(ratios), low, out["peaks"].ctypes.data_as(ctypes.c_void_p), _ip(out["n_peaks"])]
            entry = self._lib.tls_power_batch_peaks
            if peak_fits is not None:
                out["peak_fits"] = numpy.zeros((n_c, k), dtype=PEAK_FIT_DTYPE)
                assert PEAK_FIT_DTYPE.itemsize == ctypes.sizeof(PeakFit)
                args += [out["peak_fits"].ctypes.data_as(ctypes.c_void_p)]
                entry = self._lib.tls_power_batch_peak_fits
            if phase_scan is not None:
                out["phase_scans"] = numpy.zeros((n_c, k), dtype=PHASE_SCAN_DTYPE)
                assert PHASE_SCAN_DTYPE.itemsize == ctypes.sizeof(PhaseRecord)
                args += [phase_scan[0], phase_scan[1], out["phase_scans"].ctypes.data_as(ctypes.c_void_p)]
                entry = self._lib.tls_power_batch_phase_scan
        self._invalidate_results()
        self._check(entry(*args))
        self._n_periods = n_p
        return out

    def debug_transit_stats(self, y_batch, period, T0, best_row, depth, no_fit, index_power, power, row_duration,
                            fill_factor, root, max_epochs, root_count=None):
        """Developer/test entry: the statistics kernel of power_batch_stats on the prepared plan (prepare()) with injected
        picks -- period, T0, best_row, depth, no_fit, index_power per curve, power [n_curves, n_periods] -- and flux
        y_batch [n_curves, n]; root and root_count as power_batch_stats takes them; (stats, per_transit [n_curves, 6,
        max_epochs], n_epochs)."""
        return self._debug_transit(y_batch, period, T0, best_row, depth, no_fit, index_power, power, row_duration,
                                   fill_factor, root, max_epochs, root_count=root_count)

    def debug_transit_models(self, y_batch, period, T0, best_row, depth, no_fit, index_power, power, row_duration,
                             fill_factor, root, max_epochs, models, lc_cap, root_count=None):
        """Developer/test entry: the statistics and model stages of power_batch_stats(models=...) on injected picks, as
        debug_transit_stats; (stats, per_transit, n_epochs, folded, model_folded, lightcurve, lc_len)."""
        return self._debug_transit(y_batch, period, T0, best_row, depth, no_fit, index_power, power, row_duration,
                                   fill_factor, root, max_epochs, models, lc_cap, root_count=root_count)

    def _debug_transit(self, y_batch, period, T0, best_row, depth, no_fit, index_power, power, row_duration, fill_factor,
                       root, max_epochs, models=None, lc_cap=0, root_count=None):
        """tls_debug_transit_stats, or with models tls_debug_transit_models."""
        y_batch = numpy.ascontiguousarray(y_batch, dtype=numpy.float64)
        power = numpy.ascontiguousarray(power, dtype=numpy.float64)
        n_c = len(y_batch)
        if y_batch.ndim != 2 or power.shape != (n_c, self._n_periods):
            raise ValueError("power must have shape [n_curves, n_periods] of the prepared plan, y_batch [n_curves, n]")
        period, T0, depth = (_f8(numpy.broadcast_to(v, (n_c,))) for v in (period, T0, depth))
        best_row, no_fit, index_power = (_i8(numpy.broadcast_to(v, (n_c,))) for v in (best_row, no_fit, index_power))
        row_duration, root, max_epochs = _f8(row_duration), _f8(root), int(max_epochs)
        root_count = _root_count(root, root_count)
        n_root = min(len(root), len(root_count))
        stats = numpy.zeros(n_c, dtype=TRANSIT_STATS_DTYPE)
        rows = numpy.empty((n_c, len(PER_TRANSIT_FIELDS), max_epochs))
        n_epochs = numpy.empty(n_c, dtype=numpy.int64)
        args = [self._h, _dp(y_batch), n_c, _dp(period), _dp(T0), _ip(best_row), _dp(depth), _ip(no_fit), _ip(index_power),
                _dp(power), _dp(row_duration), len(row_duration), float(fill_factor), _dp(root),
                _dp(root_count), n_root, max_epochs, stats.ctypes.data_as(ctypes.c_void_p),
                _dp(rows), _ip(n_epochs)]
        out = () if models is None else _model_outputs(n_c, y_batch.shape[1], lc_cap)
        self._invalidate_results()
        if models is None:
            self._check(self._lib.tls_debug_transit_stats(*args))
        else:
            self._check(self._lib.tls_debug_transit_models(*(args + models.args(lc_cap, out))))
        return (stats, rows, n_epochs) + out

    def debug_peak_fits(self, y_batch, peaks, n_peaks, power, row_duration, fill_factor, root, max_epochs, with_fits=False,
                        phase_scan=None, root_count=None):
        """Developer/test entry: the peak-fit stage of power_batch(peaks=K, peak_fits=True) on the prepared plan (prepare())
        with injected peak records (tls_debug_peak_fits) -- flux y_batch [n_curves, n], peaks [n_curves, k] with the fields
        of PEAK_DTYPE (more are ignored), n_peaks [n_curves], the detrended power [n_curves, n_periods], root and
        root_count (a keyword) as power_batch_stats takes them: the fits
        (PEAK_FIT_DTYPE [n_curves, k]); with_fits: also every fit's trial epochs and residuals [n_curves, k, n] and n_epochs
        [n_curves, k].  phase_scan = (max_bins, min_count), without with_fits: (fits, scans) with the fits' phase scans
        (PHASE_SCAN_DTYPE [n_curves, k]) as power_batch(phase_scan=True) runs them (tls_debug_peak_phase_scans)."""
        y_batch = numpy.ascontiguousarray(y_batch, dtype=numpy.float64)
        power = numpy.ascontiguousarray(power, dtype=numpy.float64)
        n_c = len(y_batch)
        if y_batch.ndim != 2 or power.shape != (n_c, self._n_periods):
            raise ValueError("power must have shape [n_curves, n_periods] of the prepared plan, y_batch [n_curves, n]")
        peaks = numpy.asarray(peaks)
        if peaks.ndim != 2 or len(peaks) != n_c:
            raise ValueError("peaks must have shape [n_curves, k]")
        k = peaks.shape[1]
        rec = numpy.zeros((n_c, k), dtype=PEAK_DTYPE)
        for name in PEAK_DTYPE.names:
            rec[name] = peaks[name]
        n_peaks = _i8(numpy.broadcast_to(n_peaks, (n_c,)))
        row_duration, root = _f8(row_duration), _f8(root)
        root_count = _root_count(root, root_count)
        n_root = min(len(root), len(root_count))
        rc_p = _dp(root_count)
        fits = numpy.zeros((n_c, k), dtype=PEAK_FIT_DTYPE)
        assert PEAK_FIT_DTYPE.itemsize == ctypes.sizeof(PeakFit)
        n = y_batch.shape[1]
        epochs = numpy.full((n_c, k, n), numpy.nan) if with_fits else None
        residuals = numpy.full((n_c, k, n), numpy.nan) if with_fits else None
        n_epochs = numpy.zeros((n_c, k), dtype=numpy.int64) if with_fits else None
        self._invalidate_results()
        if phase_scan is not None:
            if with_fits:
                raise ValueError("phase_scan and with_fits cannot be combined")
            max_bins, min_count = phase_scan_arguments(*phase_scan)
            scans = numpy.zeros((n_c, k), dtype=PHASE_SCAN_DTYPE)
            self._check(self._lib.tls_debug_peak_phase_scans(
                self._h, _dp(y_batch), n_c, rec.ctypes.data_as(ctypes.c_void_p), _ip(n_peaks), k, _dp(power), _dp(row_duration),
                len(row_duration), float(fill_factor), _dp(root), rc_p, n_root, int(max_epochs),
                fits.ctypes.data_as(ctypes.c_void_p), max_bins, min_count, scans.ctypes.data_as(ctypes.c_void_p)))
            return fits, scans
        self._check(self._lib.tls_debug_peak_fits(
            self._h, _dp(y_batch), n_c, rec.ctypes.data_as(ctypes.c_void_p), _ip(n_peaks), k, _dp(power), _dp(row_duration),
            len(row_duration), float(fill_factor), _dp(root), rc_p, n_root, int(max_epochs),
            fits.ctypes.data_as(ctypes.c_void_p),
            None if epochs is None else _dp(epochs), None if residuals is None else _dp(residuals),
            None if n_epochs is None else _ip(n_epochs)))
        return (fits, epochs, residuals, n_epochs) if with_fits else fits

    def _invalidate_results(self):
        """Every call that launches a search, replaces its inputs or reuses the result buffers: the chi2 array an
        earlier fetch returned is no longer what the device holds (see holds)."""
        self._resident_chi2 = None
        self._generation += 1

    def prepare(self, t, y, dy, periods, table, params):
        self._invalidate_results()
        t, y, dy, periods = _f8(t), _f8(y), _f8(dy), _f8(periods)
        if not (t.ndim == y.ndim == dy.ndim == 1 and len(t) == len(y) == len(dy)):
            raise ValueError("t, y, dy must be 1-dimensional and of equal length")
        arrays, tm, pr = self._pack(table, params)
        self._check(self._lib.tls_prepare(self._h, _dp(t), _dp(y), _dp(dy), len(t), _dp(periods),
                                          len(periods), ctypes.byref(tm), ctypes.byref(pr)))
        self._n_periods = len(periods)

    def update_flux(self, y, dy):
        self._invalidate_results()
        y, dy = _f8(y), _f8(dy)
        self._check(self._lib.tls_update_flux(self._h, _dp(y), _dp(dy)))

    def execute(self, count_work=False, phase_clock=False):
        self._invalidate_results()
        self._check(self._lib.tls_execute(self._h, (1 if count_work else 0) | (2 if phase_clock else 0)))

    def t0_fit_residuals(self, t, y, period, signal, epochs, roll):
        """Residual of the depth-scaled template at every trial epoch (stats.py:178-195)."""
        t, y, signal, epochs = _f8(t), _f8(y), _f8(signal), _f8(epochs)
        out = numpy.empty(len(epochs), dtype=numpy.float64)
        self._check(self._lib.tls_t0_fit(self._h, _dp(t), _dp(y), len(t), float(period), _dp(signal),
                                         len(signal), _dp(epochs), len(epochs), int(roll), _dp(out)))
        return out

    @staticmethod
    def _fingerprint(chi2):
        """Cheap value check of a fetched array (one pass): catches an in-place edit between fetch and spectra."""
        if len(chi2) == 0:
            return (0, 0.0)
        return (len(chi2), float(numpy.sum(chi2)), float(chi2[0]), float(chi2[-1]), float(chi2[len(chi2) // 2]))

    def holds(self, chi2):
        """True if `chi2` is the very array the last fetch of this context returned, no call has launched a search,
        replaced the flux or reused the result buffers since (every such method bumps the context's generation), and
        the array still has the values it was handed out with: the device then holds the same values and tls_spectra
        may read them in place.  Anything else is uploaded."""
        ref = self._resident_chi2
        return (ref is not None and ref[0]() is chi2 and ref[1] == self._generation and len(chi2) == self._n_periods
                and ref[2] == self._fingerprint(chi2))

    def spectra(self, kernel, chi2=None):
        """SR, power_raw, power, SDE_raw, SDE (stats.py:105-132) on the device; chi2=None takes the
        chi^2 of the search that has just finished (still resident in HBM)."""
        n = self._n_periods if chi2 is None else len(chi2)
        block = numpy.empty(3 * n + 2, dtype=numpy.float64)     # one block: one device-to-host copy
        SR, praw, power, sde = block[:n], block[n:2 * n], block[2 * n:3 * n], block[3 * n:]
        c = None if chi2 is None else _f8(chi2)
        self._check(self._lib.tls_spectra(self._h, None if c is None else _dp(c), n, int(kernel), _dp(SR), _dp(praw),
                                          _dp(power), _dp(sde)))
        return SR, praw, power, float(sde[0]), float(sde[1])

    def pink_noise(self, data, width):
        """Mean over all windows of `width` points of std(window) / width ** 0.5 (stats.py:72-77) on the device, with
        the roundings of the reference's loop over numpy.std."""
        d = _f8(data)
        out = numpy.empty(1, dtype=numpy.float64)
        self._check(self._lib.tls_pink_noise(self._h, _dp(d), len(d), int(width), float(int(width) ** 0.5), _dp(out)))
        return float(out[0])

    def inject_transits(self, t, flux, constants, u1, u2):
        """(rows [n_inj, n], n_in_transit [n_inj]): flux (one row [n] shared by every injection, or [n_inj, n]) times the
        transit model of every injection (tls_inject_transits); `constants` an INJECTION_DTYPE array (or anything with its
        fields), u1 / u2 the quadratic law's coefficients (u2 = 0 for the linear law, both 0 for the uniform one)."""
        t = _f8(t)
        f = _f8(flux)
        c = numpy.zeros(numpy.size(constants["tp"]), dtype=INJECTION_DTYPE)
        for k in INJECTION_FIELDS:
            c[k] = numpy.ravel(constants[k])
        n, n_inj = len(t), len(c)
        if f.ndim == 1:
            f = f[None, :]
        if f.ndim != 2 or f.shape[1] != n:
            raise ValueError("flux must have shape [len(t)] or [n_injections, len(t)]")
        rows = numpy.empty((n_inj, n), dtype=numpy.float64)
        count = numpy.zeros(n_inj, dtype=numpy.int64)
        self._check(self._lib.tls_inject_transits(self._h, _dp(t), n, _dp(f), f.shape[0],
                                                  c.ctypes.data_as(ctypes.POINTER(Injection)), n_inj, float(u1), float(u2),
                                                  _dp(rows), _ip(count)))
        return rows, count

    def null_rows(self, n, n_rows, seed, first_trial=0, sigma=None, source=None, block=None):
        """Null light curves [n_rows, n] for trials first_trial .. first_trial + n_rows - 1 (tls_null_rows): white noise
        1 + sigma z (mode 0, `sigma` a scalar or [n_rows]) when `source` is None, else a block bootstrap of the rows of
        `source` ([n] or [n_src, n], mode 1; trial R copies row R mod n_src in blocks of `block` points)."""
        n, n_rows = int(n), int(n_rows)
        out = numpy.empty((n_rows, n), dtype=numpy.float64)
        if source is None:
            s = _f8(numpy.atleast_1d(sigma))
            if s.ndim != 1:
                raise ValueError("sigma must be a scalar or [n_rows]")
            self._check(self._lib.tls_null_rows(self._h, n, n_rows, int(seed), int(first_trial), 0, _dp(s), len(s), None, 0,
                                                0, _dp(out)))
        else:
            src = _f8(source)
            if src.ndim == 1:
                src = src[None, :]
            if src.ndim != 2 or src.shape[1] != n:
                raise ValueError("source must have shape [n] or [n_src, n]")
            self._check(self._lib.tls_null_rows(self._h, n, n_rows, int(seed), int(first_trial), 1, None, 0, _dp(src),
                                                src.shape[0], int(block), _dp(out)))
        return out

    def medfilt_detrend(self, y, kernel, return_trend=False):
        """flat = y / trend with trend = scipy.signal.medfilt(y, kernel) (tls_medfilt_detrend: a window of `kernel` samples,
        zero padding at both ends, bit-equal to scipy) for y [n] or [n_rows, n]; (flat, trend) with return_trend=True.
        ValueError for the arguments medfilt_arguments refuses."""
        rows, k = medfilt_arguments(y, kernel)
        flat = numpy.empty_like(rows)
        trend = numpy.empty_like(rows) if return_trend else None
        self._check(self._lib.tls_medfilt_detrend(self._h, _dp(rows), rows.shape[1], rows.shape[0], k, _dp(flat),
                                                  None if trend is None else _dp(trend)))
        if numpy.ndim(y) == 1:
            flat, trend = flat[0], None if trend is None else trend[0]
        return (flat, trend) if return_trend else flat

    def biweight_detrend(self, t, y, window_length, break_tolerance, return_trend=False):
        """flat = y / trend with trend the time-windowed biweight location of every point (tls_biweight_detrend: windows of
        window_length days split at gaps > break_tolerance) for y [n] or [n_rows, n] at the time stamps t [n]; (flat, trend)
        with return_trend=True.  ValueError for the arguments biweight_arguments refuses."""
        t, rows, wl, bt = biweight_arguments(t, y, window_length, break_tolerance)
        flat = numpy.empty_like(rows)
        trend = numpy.empty_like(rows) if return_trend else None
        self._check(self._lib.tls_biweight_detrend(self._h, _dp(t), _dp(rows), rows.shape[1], rows.shape[0], wl, bt,
                                                   _dp(flat), None if trend is None else _dp(trend)))
        if numpy.ndim(y) == 1:
            flat, trend = flat[0], None if trend is None else trend[0]
        return (flat, trend) if return_trend else flat

    def sysrem(self, y, n_components=1, dy=None, max_iter=50, tol=1e-6, return_trend=False, return_components=False):
        """SysRem over the rows of y [n_rows, n] (tls_sysrem: n_components rank-1 terms c_i a_j of the residual matrix
        y_ij / mean_i - 1, fitted across the rows by alternating least squares weighted with dy [n_rows, n], or with each
        row's variance where dy is None, up to max_iter iterations a component until a moves by at most tol of its largest
        value): flat = y / trend; then trend with return_trend=True; then (c [n_rows, K], a [K, n], iters [K]) with
        return_components=True.  ValueError for the arguments sysrem_arguments refuses; RuntimeError where the fit drives a
        trend value to 0 or below (wildly unequal dy)."""
        rows, dy, k, iters, tol = sysrem_arguments(y, n_components, dy, max_iter, tol)
        n_rows, n = rows.shape
        flat = numpy.empty_like(rows)
        trend = numpy.empty_like(rows) if return_trend else None
        c = numpy.empty((n_rows, k)) if return_components else None
        a = numpy.empty((k, n)) if return_components else None
        ran = numpy.zeros(k, dtype=numpy.int64) if return_components else None
        self._check(self._lib.tls_sysrem(self._h, _dp(rows), None if dy is None else _dp(dy), n, n_rows, k, iters, tol,
                                         _dp(flat), None if trend is None else _dp(trend), None if c is None else _dp(c),
                                         None if a is None else _dp(a), None if ran is None else _ip(ran)))
        out = (flat,) + ((trend,) if return_trend else ()) + (((c, a, ran),) if return_components else ())
        return out[0] if len(out) == 1 else out

    def find_peaks(self, power, periods, k, separation=0.02, ratios=(), min_power=None, chi2=None, row=None, depth=None):
        """The k harmonic-aware peaks of every row of power [n_rows, n_periods] (or one row) over `periods`, selected on the
        device (tls_find_peaks; the selection: include/tls_amd.h, tests/peaks_spec.py): (peaks (PEAK_DTYPE [n_rows, k]),
        n_peaks [n_rows]).  chi2, row and depth (each None or shaped like power) fill the fields of their names; a field
        without a source, and every entry past a row's n_peaks, is NaN or -1."""
        k, sep, ratios, low = peaks_arguments(k, separation, ratios, min_power)
        periods = _f8(periods)
        rows = numpy.ascontiguousarray(numpy.atleast_2d(numpy.asarray(power, dtype=numpy.float64)))
        if rows.ndim != 2 or periods.ndim != 1 or rows.shape[1] != len(periods) or len(periods) < 1:
            raise ValueError("power must be [n_periods] or [n_rows, n_periods] over at least one period")

        def like(a, dtype):
            if a is None:
                return None
            a = numpy.ascontiguousarray(numpy.atleast_2d(numpy.asarray(a, dtype=dtype)))
            if a.shape != rows.shape:
                raise ValueError("chi2, row and depth must have the shape of power")
            return a
        chi2, row, depth = like(chi2, numpy.float64), like(row, numpy.int64), like(depth, numpy.float64)
        peaks = numpy.zeros((rows.shape[0], k), dtype=PEAK_DTYPE)
        n_peaks = numpy.zeros(rows.shape[0], dtype=numpy.int64)
        self._check(self._lib.tls_find_peaks(
            self._h, _dp(rows), None if chi2 is None else _dp(chi2), None if row is None else _ip(row),
            None if depth is None else _dp(depth), rows.shape[0], rows.shape[1], _dp(periods), k, sep, _dp(ratios),
            len(ratios), low, peaks.ctypes.data_as(ctypes.c_void_p), _ip(n_peaks)))
        return peaks, n_peaks

    def phase_scan(self, t, y, period, T0, duration, curve=None, max_bins=PHASE_SCAN_MAX_BINS, min_count=3):
        """The phase scans (tls_phase_scan; the scan: include/tls_amd.h, tests/phase_scan_spec.py) of the candidates
        (period[f], T0[f], duration[f] in days) on light curve curve[f] (None: one fit a curve, in order) of y [n_curves, n]
        (or one row) over the finite time stamps t [n]: PHASE_SCAN_DTYPE [n_fits].  ValueError for the arguments
        phase_scan_arguments refuses, for shapes that do not agree and for a curve out of range."""
        max_bins, min_count = phase_scan_arguments(max_bins, min_count)
        t = _f8(t)
        rows = numpy.ascontiguousarray(numpy.atleast_2d(numpy.asarray(y, dtype=numpy.float64)))
        if t.ndim != 1 or rows.ndim != 2 or rows.shape[1] != len(t) or len(t) < 1:
            raise _checks.over_t(None, "y")
        _checks.time_values("phase scan", t, None, "the time stamps")
        # (numbers or numpy's own error, as ever; the shapes as every stage checks them)
        period, T0, duration = (_f8(numpy.atleast_1d(numpy.asarray(a, dtype=numpy.float64))) for a in (period, T0, duration))
        _checks.columns(None, "period, T0 and duration", (period, T0, duration))
        if curve is None:
            if len(period) != len(rows):
                raise ValueError("curve=None takes one fit a light curve: %d fits, %d curves" % (len(period), len(rows)))
            curve = numpy.arange(len(rows))
        curve = _i8(numpy.atleast_1d(numpy.asarray(curve)))
        if curve.shape != period.shape:
            raise ValueError("curve must be [n_fits]")
        if len(curve) and (curve.min() < 0 or curve.max() >= len(rows)):
            raise ValueError("phase scan: curve out of range [0, %d)" % len(rows))
        out = numpy.zeros(len(period), dtype=PHASE_SCAN_DTYPE)
        assert PHASE_SCAN_DTYPE.itemsize == ctypes.sizeof(PhaseRecord)
        self._check(self._lib.tls_phase_scan(self._h, _dp(t), _dp(rows), rows.shape[1], rows.shape[0], _ip(curve), _dp(period),
                                             _dp(T0), _dp(duration), len(period), max_bins, min_count,
                                             out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def single_transits(self, t, y, dy, widths, shapes, span_max, depth_min=0.0, k=8, min_ses=0.0, separation=0.5,
                        with_arrays=False):
        """The single-transit events (tls_single_transits; the search: include/tls_amd.h, tests/single_transit_spec.py) of
        the curves y, dy [n_curves, n] (or one row) over t [n], for the rows (widths[r], shapes[r], span_max[r]):
        (events SINGLE_EVENT_DTYPE [n_curves, k], n_events [n_curves]), with_arrays: and the planes ses, row, depth
        [n_curves, n].  ValueError for what single_arguments refuses."""
        a = single_arguments(t, y, dy, widths, shapes, span_max, depth_min, k, min_ses, separation)
        n_c, n = a["y"].shape
        events = numpy.zeros((n_c, a["k"]), dtype=SINGLE_EVENT_DTYPE)
        n_events = numpy.zeros(n_c, dtype=numpy.int64)
        assert SINGLE_EVENT_DTYPE.itemsize == ctypes.sizeof(SingleEvent)
        ses = depth = row = None
        if with_arrays:
            ses, depth, row = numpy.empty((n_c, n)), numpy.empty((n_c, n)), numpy.empty((n_c, n), dtype=numpy.int64)
        self._check(self._lib.tls_single_transits(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["dy"]), n, n_c, _dp(a["shape_values"]), _ip(a["shape_offset"]),
            _ip(a["width"]), _dp(a["span_max"]), len(a["width"]), a["depth_min"], a["k"], a["min_ses"], a["separation"],
            events.ctypes.data_as(ctypes.c_void_p), _ip(n_events), None if ses is None else _dp(ses),
            None if row is None else _ip(row), None if depth is None else _dp(depth)))
        return (events, n_events, ses, row, depth) if with_arrays else (events, n_events)

    def transit_times(self, t, y, dy, period, T0, row, reach, widths, shapes, span_max, curve=None, depth_min=0.0,
                      min_ses=3.0, max_epochs=1):
        """The transit times and refitted ephemerides (tls_transit_times; the statement: include/tls_amd.h,
        tests/transit_times_spec.py) of the candidates (period[f], T0[f], row[f], reach[f]) on the curves curve[f] (None: one
        candidate a curve, in order) of y, dy [n_curves, n] (or one row) over t [n], for the rows (widths[r], shapes[r],
        span_max[r]): (EPHEMERIS_DTYPE [n_fits], TRANSIT_TIME_DTYPE [n_fits, max_epochs]).  ValueError for what
        transit_times_arguments refuses."""
        a = transit_times_arguments(t, y, dy, period, T0, row, reach, widths, shapes, span_max, curve, depth_min, min_ses,
                                    max_epochs)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        eph = numpy.zeros(n_fits, dtype=EPHEMERIS_DTYPE)
        times = numpy.zeros((n_fits, a["max_epochs"]), dtype=TRANSIT_TIME_DTYPE)
        assert EPHEMERIS_DTYPE.itemsize == ctypes.sizeof(Ephemeris) and TRANSIT_TIME_DTYPE.itemsize == ctypes.sizeof(TransitTime)
        self._check(self._lib.tls_transit_times(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["dy"]), n, n_c, _ip(a["curve"]), _dp(a["period"]), _dp(a["T0"]),
            _ip(a["row"]), _ip(a["reach"]), n_fits, _dp(a["shape_values"]), _ip(a["shape_offset"]), _ip(a["width"]),
            _dp(a["span_max"]), len(a["width"]), a["depth_min"], a["min_ses"], a["max_epochs"],
            eph.ctypes.data_as(ctypes.c_void_p), times.ctypes.data_as(ctypes.c_void_p)))
        return eph, times

    def event_vetting(self, t, y, dy, period, T0, row, reach, chase_reach, guard, chase_span, widths, shapes, span_max,
                      curve=None, depth_min=0.0, min_ses=3.0, chase_fraction=0.6, chase_min=0.5, point_fraction=0.5,
                      step_fraction=0.5, max_epochs=1):
        """The per-transit event vetting (tls_event_vetting; the statement: include/tls_amd.h, tests/event_vetting_spec.py)
        of the candidates (period[f], T0[f], row[f], reach[f], chase_reach[f], guard[f], chase_span[f]) on the curves curve[f]
        (None: one candidate a curve, in order) of y, dy [n_curves, n] (or one row) over t [n], for the rows (widths[r],
        shapes[r], span_max[r]): (EVENT_SUMMARY_DTYPE [n_fits], EVENT_RECORD_DTYPE [n_fits, max_epochs]).  ValueError for what
        event_vetting_arguments refuses."""
        a = event_vetting_arguments(t, y, dy, period, T0, row, reach, chase_reach, guard, chase_span, widths, shapes, span_max,
                                    curve, depth_min, min_ses, chase_fraction, chase_min, point_fraction, step_fraction,
                                    max_epochs)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        out = numpy.zeros(n_fits, dtype=EVENT_SUMMARY_DTYPE)
        events = numpy.zeros((n_fits, a["max_epochs"]), dtype=EVENT_RECORD_DTYPE)
        assert EVENT_SUMMARY_DTYPE.itemsize == ctypes.sizeof(EventSummary) and EVENT_RECORD_DTYPE.itemsize == ctypes.sizeof(EventRecord)
        self._check(self._lib.tls_event_vetting(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["dy"]), n, n_c, _ip(a["curve"]), _dp(a["period"]), _dp(a["T0"]),
            _ip(a["row"]), _ip(a["reach"]), _ip(a["chase_reach"]), _ip(a["guard"]), _dp(a["chase_span"]), n_fits,
            _dp(a["shape_values"]), _ip(a["shape_offset"]), _ip(a["width"]), _dp(a["span_max"]), len(a["width"]),
            a["depth_min"], a["min_ses"], a["chase_fraction"], a["chase_min"], a["point_fraction"], a["step_fraction"],
            a["max_epochs"], out.ctypes.data_as(ctypes.c_void_p), events.ctypes.data_as(ctypes.c_void_p)))
        return out, events

    def shape_fit(self, t, y, dy, period, T0, duration, ratios, ingress, shifts, curve=None, window=2.0, min_count=3,
                  depth_min=0.0):
        """The trapezoid shape fits (tls_shape_fit; the statement: include/tls_amd.h, tests/shape_fit_spec.py) of the
        candidates (period[f], T0[f], duration[f] in days) on the curves curve[f] (None: one candidate a curve, in order) of
        y, dy [n_curves, n] (or one row) over t [n], over the units of the tables ratios, ingress, shifts: SHAPE_DTYPE
        [n_fits].  ValueError for what shape_fit_arguments refuses."""
        a = shape_fit_arguments(t, y, dy, period, T0, duration, ratios, ingress, shifts, curve, window, min_count, depth_min)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        out = numpy.zeros(n_fits, dtype=SHAPE_DTYPE)
        assert SHAPE_DTYPE.itemsize == ctypes.sizeof(ShapeRecord)
        self._check(self._lib.tls_shape_fit(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["dy"]), n, n_c, _dp(a["period"]), _dp(a["T0"]), _dp(a["duration"]),
            _ip(a["curve"]), n_fits, _dp(a["ratio"]), len(a["ratio"]), _dp(a["ingress"]), len(a["ingress"]), _dp(a["shift"]),
            len(a["shift"]), a["window"], a["min_count"], a["depth_min"], out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def centroid_test(self, t, y, cx, cy, period, T0, duration, shape, curve=None, window=3.0, min_in=1, min_out=3,
                      max_epochs=CENTROID_MAX_EPOCHS):
        """The centroid-shift tests (tls_centroid_test; the statement: include/tls_amd.h, tests/centroid_spec.py) of the
        candidates (period[f], T0[f], duration[f] in days) on the curves curve[f] (None: one candidate a curve, in order) of
        y, cx, cy [n_curves, n] (or one row) over t [n], with the shape [L] (0 out of transit, 1 at the bottom):
        CENTROID_DTYPE [n_fits].  ValueError for what centroid_arguments refuses."""
        a = centroid_arguments(t, y, cx, cy, period, T0, duration, shape, curve, window, min_in, min_out, max_epochs)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        out = numpy.zeros(n_fits, dtype=CENTROID_DTYPE)
        assert CENTROID_DTYPE.itemsize == ctypes.sizeof(CentroidRecord)
        self._check(self._lib.tls_centroid_test(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["cx"]), _dp(a["cy"]), n, n_c, _dp(a["period"]), _dp(a["T0"]),
            _dp(a["duration"]), _ip(a["curve"]), n_fits, _dp(a["shape"]), len(a["shape"]), a["window"], a["min_in"],
            a["min_out"], a["max_epochs"], out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def folded_views(self, t, y, period, T0, duration, curve=None, secondary_phase=None, n_global=2001, n_local=201,
                     local_durations=4.0, local_width=0.16):
        """The folded, median-binned views (tls_folded_views; the statement: include/tls_amd.h, tests/folded_views_spec.py)
        of the candidates (period[f], T0[f], duration[f] in days, secondary_phase[f]; None: no secondary view) on the rows
        curve[f] (None: one candidate a curve, in order) of y [n_curves, n] (or one row) over t [n]: (records VIEWS_DTYPE
        [n_fits], global_median [n_fits, n_global], global_count (int32), local_median [n_fits, 4, n_local] in the order
        VIEWS_LOCAL, local_count).  ValueError for what folded_views_arguments refuses."""
        a = folded_views_arguments(t, y, period, T0, duration, curve, secondary_phase, n_global, n_local, local_durations,
                                   local_width)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        out = numpy.zeros(n_fits, dtype=VIEWS_DTYPE)
        g_med = numpy.empty((n_fits, a["n_global"]))
        g_cnt = numpy.empty((n_fits, a["n_global"]), dtype=numpy.int32)
        l_med = numpy.empty((n_fits, len(VIEWS_LOCAL), a["n_local"]))
        l_cnt = numpy.empty((n_fits, len(VIEWS_LOCAL), a["n_local"]), dtype=numpy.int32)
        assert VIEWS_DTYPE.itemsize == ctypes.sizeof(ViewsRecord)
        phi = a["secondary_phase"]
        self._check(self._lib.tls_folded_views(
            self._h, _dp(a["t"]), _dp(a["y"]), n, n_c, _dp(a["period"]), _dp(a["T0"]), _dp(a["duration"]),
            None if phi is None else _dp(phi), _ip(a["curve"]), n_fits, a["n_global"], a["n_local"], a["local_durations"],
            a["local_width"], out.ctypes.data_as(ctypes.c_void_p), _dp(g_med), g_cnt.ctypes.data_as(ctypes.c_void_p),
            _dp(l_med), l_cnt.ctypes.data_as(ctypes.c_void_p)))
        return out, g_med, g_cnt, l_med, l_cnt

    def nudft(self, rows, t, frequencies):
        """The non-uniform DFT of the rows [n_rows, n] (or one row) over t [n] at `frequencies` [F] (tls_nudft; the statement:
        include/tls_amd.h, tests/gls_spec.py): [n_rows, F, 2] with (sum_i rows[r, i] cos phi_ki, sum_i rows[r, i] sin phi_ki),
        phi_ki = 2 pi frac(f_k (t_i - t_0)).  ValueError for what gls_axes refuses and for rows that are not finite."""
        t, f = gls_axes(t, frequencies, 1)
        rows = gls_rows(t, rows, None, "nudft")[0]
        out = numpy.zeros((len(rows), len(f), 2))
        self._check(self._lib.tls_nudft(self._h, _dp(rows), len(rows), len(t), _dp(t), _dp(f), len(f), _dp(out)))
        return out

    def lomb_scargle(self, t, y, frequencies, dy=None, peaks=None, separation=0.02, with_arrays=True, debug=False):
        """The generalised Lomb-Scargle periodogram (tls_lomb_scargle; the statement: include/tls_amd.h, tests/gls_spec.py) of
        y [n_curves, n] (or one row; dy: per-point errors, None: uniform weights) over t [n] at `frequencies` [F]: a dict with
        mean, variance [n_curves]; with_arrays: power, amplitude, phase [n_curves, F]; peaks=K: peaks (PEAK_DTYPE
        [n_curves, K], period = 1 / frequency) and n_peaks, selected on the device; debug: rows (a [n_curves, n]), weights
        ([n_curves, n] with dy, [n] without) and sums [n_curves, F, 6] (GLS_SUMS).  ValueError for what
        lomb_scargle_arguments refuses."""
        a = lomb_scargle_arguments(t, y, dy, frequencies, peaks, separation)
        n_c, n = a["y"].shape
        F, k = len(a["frequencies"]), a["k"]
        out = dict(mean=numpy.zeros(n_c), variance=numpy.zeros(n_c))
        if with_arrays:
            out.update(power=numpy.zeros((n_c, F)), amplitude=numpy.zeros((n_c, F)), phase=numpy.zeros((n_c, F)))
        if k:
            out.update(peaks=numpy.zeros((n_c, k), dtype=PEAK_DTYPE), n_peaks=numpy.zeros(n_c, dtype=numpy.int64))
            assert PEAK_DTYPE.itemsize == ctypes.sizeof(Peak)
        if debug:
            out.update(rows=numpy.zeros((n_c, n)), weights=numpy.zeros(n if a["dy"] is None else (n_c, n)),
                       sums=numpy.zeros((n_c, F, 6)))

        def ptr(name):
            return _dp(out[name]) if name in out else None
        self._check(self._lib.tls_lomb_scargle(
            self._h, _dp(a["t"]), _dp(a["y"]), None if a["dy"] is None else _dp(a["dy"]), n, n_c, _dp(a["frequencies"]), F,
            _dp(out["mean"]), _dp(out["variance"]), ptr("power"), ptr("amplitude"), ptr("phase"), k, a["separation"],
            out["peaks"].ctypes.data_as(ctypes.c_void_p) if k else None, _ip(out["n_peaks"]) if k else None,
            ptr("rows"), ptr("weights"), ptr("sums")))
        return out

    def sine_test(self, t, y, period, curve=None, dy=None, T0=None, duration=None, mask=1.5, harmonics=(0.5, 1.0, 2.0),
                  debug=False):
        """The sine tests (tls_sine_test; the statement: include/tls_amd.h, tests/gls_spec.py) of the candidates (period[f],
        and T0[f], duration[f] in days where the transits are to be masked) on the curves curve[f] (None: one candidate a
        curve, in order) of y [n_curves, n] (or one row; dy: per-point errors) over t [n]: (records SINE_DTYPE [n_fits],
        harmonic records SINE_HARMONIC_DTYPE [n_fits, n_harmonics]) and, with debug, the sums [n_fits, n_harmonics, 6]
        (GLS_SUMS).  ValueError for what sine_test_arguments refuses."""
        a = sine_test_arguments(t, y, dy, period, T0, duration, curve, mask, harmonics)
        n_c, n = a["y"].shape
        n_fits, nH = len(a["period"]), len(a["harmonics"])
        out = numpy.zeros(n_fits, dtype=SINE_DTYPE)
        out_h = numpy.zeros((n_fits, nH), dtype=SINE_HARMONIC_DTYPE)
        sums = numpy.zeros((n_fits, nH, 6)) if debug else None
        assert SINE_DTYPE.itemsize == ctypes.sizeof(SineRecord) and SINE_HARMONIC_DTYPE.itemsize == ctypes.sizeof(SineHarmonic)
        self._check(self._lib.tls_sine_test(
            self._h, _dp(a["t"]), _dp(a["y"]), None if a["dy"] is None else _dp(a["dy"]), n, n_c, _dp(a["period"]),
            None if a["T0"] is None else _dp(a["T0"]), None if a["duration"] is None else _dp(a["duration"]), _ip(a["curve"]),
            n_fits, _dp(a["harmonics"]), nH, a["mask"], out.ctypes.data_as(ctypes.c_void_p),
            out_h.ctypes.data_as(ctypes.c_void_p), None if sums is None else _dp(sums)))
        return (out, out_h, sums) if debug else (out, out_h)

    def prewhiten(self, t, y, frequencies, n_terms=3, harmonics=1, min_power=0.0, dy=None, return_trend=False,
                  return_terms=False, debug=False):
        """Iterative sinusoid pre-whitening (tls_prewhiten; the statement: include/tls_amd.h, tests/prewhiten_spec.py) of
        y [n_curves, n] (or one row; dy: per-point errors, None: uniform weights) over t [n] on the grid `frequencies` [F]:
        flat [n_curves, n] (one row: [n]); then trend with return_trend=True; then a dict with terms (PREWHITEN_DTYPE
        [n_curves, n_terms, harmonics]), n_iterations and status [n_curves] with return_terms=True; with debug the dict also
        holds steps [n_terms * harmonics + 1, n_curves, n] (the row entering every (iteration, harmonic), then the final
        row) and sums [n_curves, n_terms, harmonics, 6] (GLS_SUMS).  ValueError for what prewhiten_arguments refuses."""
        a = prewhiten_arguments(t, y, dy, frequencies, n_terms, harmonics, min_power)
        n_c, n = a["y"].shape
        K, H = a["n_terms"], a["harmonics"]
        flat = numpy.empty_like(a["y"])
        trend = numpy.empty_like(a["y"]) if return_trend else None
        terms = numpy.zeros((n_c, K, H), dtype=PREWHITEN_DTYPE)
        info = dict(terms=terms, n_iterations=numpy.zeros(n_c, dtype=numpy.int64), status=numpy.zeros(n_c))
        if debug:
            info.update(steps=numpy.zeros((K * H + 1, n_c, n)), sums=numpy.zeros((n_c, K, H, 6)))
        assert PREWHITEN_DTYPE.itemsize == ctypes.sizeof(PrewhitenTerm)
        self._check(self._lib.tls_prewhiten(
            self._h, _dp(a["t"]), _dp(a["y"]), None if a["dy"] is None else _dp(a["dy"]), n, n_c, _dp(a["frequencies"]),
            len(a["frequencies"]), K, H, a["min_power"], _dp(flat), None if trend is None else _dp(trend),
            terms.ctypes.data_as(ctypes.c_void_p), _ip(info["n_iterations"]), _dp(info["status"]),
            _dp(info["steps"]) if debug else None, _dp(info["sums"]) if debug else None))
        if numpy.ndim(y) == 1:   # (one row comes back as [n]; the records keep their leading axis)
            flat, trend = flat[0], None if trend is None else trend[0]
        out = (flat,) + ((trend,) if return_trend else ()) + ((info,) if return_terms or debug else ())
        return out[0] if len(out) == 1 else out

    def ephemeris_match(self, star, period, T0, duration, strength, span, drift_tolerance=0.5, epoch_tolerance=0.5,
                        max_ratio=3):
        """The ephemeris match (tls_ephemeris_match; the statement: include/tls_amd.h, tests/ephemeris_match_spec.py) of the
        candidates (star[f], period[f], T0[f], duration[f] in days, strength[f]) against one another: MATCH_DTYPE [M].
        ValueError for what ephemeris_match_arguments refuses."""
        a = ephemeris_match_arguments(star, period, T0, duration, strength, span, drift_tolerance, epoch_tolerance, max_ratio)
        out = numpy.zeros(len(a["star"]), dtype=MATCH_DTYPE)
        assert MATCH_DTYPE.itemsize == ctypes.sizeof(MatchRecord)
        self._check(self._lib.tls_ephemeris_match(
            self._h, _ip(a["star"]), _dp(a["period"]), _dp(a["T0"]), _dp(a["duration"]), _dp(a["strength"]), len(a["star"]),
            a["span"], a["drift_tolerance"], a["epoch_tolerance"], a["max_ratio"], out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def event_periods(self, t, y, dy, curve, index_a, index_b, row, reach, offset, widths, shapes, span_max, period_min,
                      max_aliases=256, min_ses=3.0, veto_sigma=3.0, with_aliases=True):
        """The period aliases (tls_event_periods; the statement: include/tls_amd.h, tests/event_periods_spec.py) of the event
        pairs (curve[f], index_a[f] < index_b[f], row[f], reach[f], offset[f] in days) on the curves of y, dy [n_curves, n] (or
        one row) over t [n], for the rows (widths[r], shapes[r], span_max[r]): (EVENT_PAIR_DTYPE [n_pairs], EVENT_ALIAS_DTYPE
        [n_pairs, max_aliases], or None without with_aliases).  ValueError for what event_periods_arguments refuses."""
        a = event_periods_arguments(t, y, dy, curve, index_a, index_b, row, reach, offset, widths, shapes, span_max, period_min,
                                    max_aliases, min_ses, veto_sigma)
        n_c, n = a["y"].shape
        n_pairs = len(a["curve"])
        pairs = numpy.zeros(n_pairs, dtype=EVENT_PAIR_DTYPE)
        aliases = numpy.zeros((n_pairs, a["max_aliases"]), dtype=EVENT_ALIAS_DTYPE) if with_aliases else None
        assert EVENT_PAIR_DTYPE.itemsize == ctypes.sizeof(EventPair) and EVENT_ALIAS_DTYPE.itemsize == ctypes.sizeof(EventAlias)
        self._check(self._lib.tls_event_periods(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["dy"]), n, n_c, _ip(a["curve"]), _ip(a["index_a"]), _ip(a["index_b"]),
            _ip(a["row"]), _ip(a["reach"]), _dp(a["offset"]), n_pairs, _dp(a["shape_values"]), _ip(a["shape_offset"]),
            _ip(a["width"]), _dp(a["span_max"]), len(a["width"]), a["period_min"], a["max_aliases"], a["min_ses"],
            a["veto_sigma"], pairs.ctypes.data_as(ctypes.c_void_p),
            None if aliases is None else aliases.ctypes.data_as(ctypes.c_void_p)))
        return pairs, aliases

    def noise_profile(self, t, y, widths, span_max, pair_span, clip_upper=5.0, clip_lower=5.0, min_count=3):
        """The noise profiles (tls_noise_profile; the statement: include/tls_amd.h, tests/noise_profile_spec.py) of the curves
        y [n_curves, n] (or one row) over t [n] (None: no gaps) at the window widths `widths` [W] (samples) with the span
        limits span_max [W] and pair_span: (records NOISE_CURVE_DTYPE [n_curves], count int64 [n_curves, W], robust and rms
        [n_curves, W]).  ValueError for what noise_arguments refuses."""
        a = noise_arguments(t, y, widths, span_max, pair_span, clip_upper, clip_lower, min_count)
        n_c, n = a["y"].shape
        W = len(a["widths"])
        records = numpy.zeros(n_c, dtype=NOISE_CURVE_DTYPE)
        count = numpy.zeros((n_c, W), dtype=numpy.int64)
        robust, rms = numpy.zeros((n_c, W)), numpy.zeros((n_c, W))
        assert NOISE_CURVE_DTYPE.itemsize == ctypes.sizeof(NoiseCurve)
        self._check(self._lib.tls_noise_profile(
            self._h, None if a["t"] is None else _dp(a["t"]), _dp(a["y"]), n, n_c, _ip(a["widths"]), _dp(a["span_max"]), W,
            a["pair_span"], a["clip_upper"], a["clip_lower"], a["min_count"], records.ctypes.data_as(ctypes.c_void_p),
            _ip(count), _dp(robust), _dp(rms)))
        return records, count, robust, rms

    def transit_fit(self, t, y, dy, period, T0, duration, row_first, k_rows, profile, impacts, ratios, shifts, sub, curve=None,
                    window=1.0, min_count=3, delta=1.0):
        """The limb-darkened transit fits (tls_transit_fit; the statement: include/tls_amd.h, tests/transit_fit_spec.py) of
        the candidates (period[f], T0[f], duration[f] in days, seed row row_first[f]) on the curves curve[f] (None: one
        candidate a curve, in order) of y, dy [n_curves, n] (or one row) over t [n], with the profile table (k_rows,
        profile), over the units of the tables impacts, ratios, shifts and the sub-exposure offsets sub:
        TRANSIT_FIT_DTYPE [n_fits].  ValueError for what transit_fit_arguments refuses."""
        a = transit_fit_arguments(t, y, dy, period, T0, duration, row_first, k_rows, profile, impacts, ratios, shifts, sub,
                                  curve, window, min_count, delta)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        out = numpy.zeros(n_fits, dtype=TRANSIT_FIT_DTYPE)
        assert TRANSIT_FIT_DTYPE.itemsize == ctypes.sizeof(TransitFitRecord)
        self._check(self._lib.tls_transit_fit(
            self._h, _dp(a["t"]), _dp(a["y"]), _dp(a["dy"]), n, n_c, _ip(a["curve"]), _dp(a["period"]), _dp(a["T0"]),
            _dp(a["duration"]), _ip(a["row_first"]), n_fits, _dp(a["k_rows"]), _dp(a["profile"]), len(a["k_rows"]),
            a["profile"].shape[1] - 1, _dp(a["impact"]), len(a["impact"]), _dp(a["ratio"]), len(a["ratio"]), _dp(a["shift"]),
            len(a["shift"]), _dp(a["sub"]), len(a["sub"]), a["window"], a["min_count"], a["delta"],
            out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def transit_mask(self, t, period, T0, duration, curve=None, n_curves=None, factor=1.5):
        """The in-transit flags uint8 [n_curves, n] (1 = protected) of the candidates (curve[k], period[k], T0[k], duration[k]
        in days) at the time stamps t, `factor` durations wide (tls_transit_mask; the statement: include/tls_amd.h,
        tests/transit_protect_spec.py).  ValueError for what transit_mask_arguments refuses."""
        a = transit_mask_arguments(t, period, T0, duration, curve, n_curves, factor)
        out = numpy.zeros((a["n_curves"], len(a["t"])), dtype=numpy.uint8)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.tls_transit_mask(
            self._h, _dp(a["t"]), len(a["t"]), None if a["curve"] is None else _ip(a["curve"]), _dp(a["period"]), _dp(a["T0"]),
            _dp(a["duration"]), len(a["period"]), a["factor"], a["n_curves"], out.ctypes.data_as(u8)))
        return out

    def biweight_detrend_masked(self, t, y, mask, window_length, break_tolerance, min_points=3, return_trend=False,
                                return_status=False):
        """biweight_detrend with the points of mask (uint8 or bool, y's shape, != 0: protected) left out of every fit
        (tls_biweight_detrend_masked): a window with min_points unprotected points gets their biweight location (status 0), any
        other point the trend interpolated between its nearest fitted neighbours (status 1), a segment without a fitted point
        the plain biweight (status 2).  flat[, trend][, status uint8] in y's shape.  ValueError for what
        biweight_masked_arguments refuses."""
        t, rows, mk, wl, bt, low = biweight_masked_arguments(t, y, mask, window_length, break_tolerance, min_points)
        flat = numpy.empty_like(rows)
        trend = numpy.empty_like(rows) if return_trend else None
        status = numpy.empty(rows.shape, dtype=numpy.uint8) if return_status else None
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.tls_biweight_detrend_masked(
            self._h, _dp(t), _dp(rows), mk.ctypes.data_as(u8), rows.shape[1], rows.shape[0], wl, bt, low, _dp(flat),
            None if trend is None else _dp(trend), None if status is None else status.ctypes.data_as(u8)))
        out = (flat,) + ((trend,) if return_trend else ()) + ((status,) if return_status else ())
        if numpy.ndim(y) == 1:
            out = tuple(v[0] for v in out)
        return out[0] if len(out) == 1 else out

    def prewhiten_masked(self, t, y, mask, frequencies, n_terms=3, harmonics=1, min_power=0.0, dy=None, return_trend=False,
                         return_terms=False, debug=False):
        """prewhiten with the points of mask (uint8 or bool, y's shape, != 0: protected) given weight 0.0 in the periodogram
        and in the fit (tls_prewhiten_masked); the subtraction and the trend cover every point.  A row with fewer than 3
        unprotected points has nothing removed (status 2).  Returns what prewhiten returns.  ValueError for what
        prewhiten_arguments and detrend_mask_rows refuse."""
        a = prewhiten_arguments(t, y, dy, frequencies, n_terms, harmonics, min_power)
        mk = detrend_mask_rows(mask, a["y"].shape)
        n_c, n = a["y"].shape
        K, H = a["n_terms"], a["harmonics"]
        flat = numpy.empty_like(a["y"])
        trend = numpy.empty_like(a["y"]) if return_trend else None
        terms = numpy.zeros((n_c, K, H), dtype=PREWHITEN_DTYPE)
        info = dict(terms=terms, n_iterations=numpy.zeros(n_c, dtype=numpy.int64), status=numpy.zeros(n_c))
        if debug:
            info.update(steps=numpy.zeros((K * H + 1, n_c, n)), sums=numpy.zeros((n_c, K, H, 6)))
        self._check(self._lib.tls_prewhiten_masked(
            self._h, _dp(a["t"]), _dp(a["y"]), None if a["dy"] is None else _dp(a["dy"]),
            mk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, n_c, _dp(a["frequencies"]), len(a["frequencies"]), K, H,
            a["min_power"], _dp(flat), None if trend is None else _dp(trend), terms.ctypes.data_as(ctypes.c_void_p),
            _ip(info["n_iterations"]), _dp(info["status"]), _dp(info["steps"]) if debug else None,
            _dp(info["sums"]) if debug else None))
        if numpy.ndim(y) == 1:
            flat, trend = flat[0], None if trend is None else trend[0]
        out = (flat,) + ((trend,) if return_trend else ()) + ((info,) if return_terms or debug else ())
        return out[0] if len(out) == 1 else out

    def remove_transits(self, t, y, period, T0, row, amplitude, b, duration, shift, k_rows, profile, sub, curve=None,
                        return_model=False, return_status=False):
        """The rows y [n_curves, n] (or one row) over t [n] with the fitted transits of the candidates divided out
        (tls_remove_transits; the statement: include/tls_amd.h, tests/remove_transits_spec.py): candidate f carries period[f]
        and T0[f] of a peak and row[f], amplitude[f], b[f], duration[f], shift[f] of its transit-fit record on the curve
        curve[f] (None: one candidate a curve, in order), with the k_rows, profile and sub of that fit.  rows[, model][, status
        float64 [n_fits]: 0 divided out, 1 skipped].  ValueError for what remove_transits_arguments refuses."""
        a = remove_transits_arguments(t, y, period, T0, row, amplitude, b, duration, shift, k_rows, profile, sub, curve)
        n_c, n = a["y"].shape
        n_fits = len(a["period"])
        rows = numpy.empty_like(a["y"])
        model = numpy.empty_like(a["y"]) if return_model else None
        status = numpy.zeros(n_fits)
        self._check(self._lib.tls_remove_transits(
            self._h, _dp(a["t"]), _dp(a["y"]), n, n_c, None if a["curve"] is None else _ip(a["curve"]), _dp(a["period"]),
            _dp(a["T0"]), _ip(a["row"]), _dp(a["amplitude"]), _dp(a["b"]), _dp(a["duration"]), _dp(a["shift"]), n_fits,
            _dp(a["k_rows"]), _dp(a["profile"]), len(a["k_rows"]), a["profile"].shape[1] - 1, _dp(a["sub"]), len(a["sub"]),
            _dp(rows), None if model is None else _dp(model), _dp(status)))
        if numpy.ndim(y) == 1:
            rows, model = rows[0], None if model is None else model[0]
        out = (rows,) + ((model,) if return_model else ()) + ((status,) if return_status else ())
        return out[0] if len(out) == 1 else out

    def decorrelate(self, y, own=None, shared=None, dy=None, mask=None, segments=None, ridge=0.0, n_iter=3, sigma_upper=5.0,
                    sigma_lower=5.0, return_trend=False, return_fit=False):
        """Regression detrending (tls_decorrelate; the statement: include/tls_amd.h, tests/decorrelate_spec.py) of the curves
        y [n_curves, n] (or one row) against the columns shared [n_shared, n] and own [n_curves, n_own, n], every
        (curve, segment) fitted on its own with up to n_iter clip rounds: flat; then trend with return_trend=True; then, with
        return_fit=True, a dict with record (DECOR_DTYPE [n_curves, n_seg]), coef, mean and scale [n_curves, n_seg, m],
        coefficients (coef / scale: in the units of the raw columns, 0.0 for a column that is not in the fit) and segments.
        ValueError for what decorrelate_arguments refuses."""
        a = decorrelate_arguments(y, own, shared, dy, mask, segments, ridge, n_iter, sigma_upper, sigma_lower)
        n_c, n = a["y"].shape
        n_shared, n_own = a["shared"].shape[0], a["own"].shape[1]
        m, S = n_shared + n_own, len(a["segments"]) - 1
        flat = numpy.empty_like(a["y"])
        trend = numpy.empty_like(a["y"]) if return_trend else None
        record = numpy.zeros((n_c, S), dtype=DECOR_DTYPE)
        coef, mean, scale = (numpy.zeros((n_c, S, m)) if return_fit else None for _ in range(3))
        assert DECOR_DTYPE.itemsize == ctypes.sizeof(DecorFit)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.tls_decorrelate(
            self._h, _dp(a["y"]), None if a["dy"] is None else _dp(a["dy"]),
            None if a["mask"] is None else a["mask"].ctypes.data_as(u8p), n, n_c, _dp(a["shared"]) if n_shared else None, n_shared,
            _dp(a["own"]) if n_own else None, n_own, _ip(a["segments"]), S, a["ridge"], a["n_iter"], a["sigma_upper"],
            a["sigma_lower"], _dp(flat), None if trend is None else _dp(trend), record.ctypes.data_as(ctypes.c_void_p),
            None if coef is None else _dp(coef), None if mean is None else _dp(mean), None if scale is None else _dp(scale)))
        if a["single"]:
            flat, trend = flat[0], None if trend is None else trend[0]
        out = (flat,) + ((trend,) if return_trend else ())
        if return_fit:
            with numpy.errstate(all="ignore"):
                raw = numpy.where(coef != 0.0, coef / scale, 0.0)
            out += ({"record": record, "coef": coef, "mean": mean, "scale": scale, "coefficients": raw,
                     "segments": a["segments"]},)
        return out[0] if len(out) == 1 else out

    def spline_detrend(self, t, y, knot_spacing=0.75, break_tolerance=0.5, penalty=1e-3, n_iter=5, sigma_upper=3.0,
                       sigma_lower=3.0, dy=None, mask=None, return_trend=False, return_fit=False):
        """Robust B-spline detrending (tls_spline_detrend; the statement: include/tls_amd.h, tests/spline_spec.py) of the curves
        y [n_curves, n] (or one row) over t: flat; then trend with return_trend=True; then, with return_fit=True, a dict with
        segment (SPLINE_SEGMENT_DTYPE [n_curves, n_seg]), curve (SPLINE_CURVE_DTYPE [n_curves]), segments (the index
        boundaries) and spacings.  ValueError for what spline_arguments refuses."""
        a = spline_arguments(t, y, knot_spacing, break_tolerance, penalty, n_iter, sigma_upper, sigma_lower, dy, mask)
        n_c, n = a["y"].shape
        G = len(a["segments"]) - 1
        flat = numpy.empty_like(a["y"])
        trend = numpy.empty_like(a["y"]) if return_trend else None
        segment = numpy.zeros((n_c, G), dtype=SPLINE_SEGMENT_DTYPE)
        curve = numpy.zeros(n_c, dtype=SPLINE_CURVE_DTYPE)
        assert SPLINE_SEGMENT_DTYPE.itemsize == 8 * len(SPLINE_SEGMENT_FIELDS) and SPLINE_CURVE_DTYPE.itemsize == 8 * (3 + SPLINE_MAX_SPACINGS)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.tls_spline_detrend(
            self._h, _dp(a["t"]), _dp(a["y"]), None if a["dy"] is None else _dp(a["dy"]),
            None if a["mask"] is None else a["mask"].ctypes.data_as(u8p), n, n_c, _dp(a["spacings"]), len(a["spacings"]),
            a["break_tolerance"], a["penalty"], a["n_iter"], a["sigma_upper"], a["sigma_lower"], _dp(flat),
            None if trend is None else _dp(trend), segment.ctypes.data_as(ctypes.c_void_p), curve.ctypes.data_as(ctypes.c_void_p)))
        if a["single"]:
            flat, trend = flat[0], None if trend is None else trend[0]
        out = (flat,) + ((trend,) if return_trend else ())
        if return_fit:
            out += ({"segment": segment, "curve": curve, "segments": a["segments"], "spacings": a["spacings"]},)
        return out[0] if len(out) == 1 else out

    def clean_rows(self, t, y, window_length=None, break_tolerance=0.5, sigma_upper=4.0, sigma_lower=float("inf"), max_run=1,
                   n_iter=3, min_points=3, bad=None, return_flags=False, return_record=False):
        """The cleaning stage (tls_clean_rows; the statement: include/tls_amd.h, tests/clean_spec.py) of the curves y
        [n_curves, n] (or one row) over t, which may hold NaN, infinities and values <= 0: the repaired rows; then, with
        return_flags=True, the flags (uint8: 1 missing, 2 the caller's bad, 4 high, 8 low); then, with return_record=True, the
        records (CLEAN_DTYPE [n_curves]).  ValueError for what clean_arguments refuses."""
        a = clean_arguments(t, y, window_length, break_tolerance, sigma_upper, sigma_lower, max_run, n_iter, min_points, bad)
        n_c, n = a["y"].shape
        rows = numpy.empty_like(a["y"])
        flags = numpy.empty((n_c, n), dtype=numpy.uint8)
        record = numpy.zeros(n_c, dtype=CLEAN_DTYPE)
        assert CLEAN_DTYPE.itemsize == 8 * len(CLEAN_FIELDS)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.tls_clean_rows(
            self._h, _dp(a["t"]), _dp(a["y"]), None if a["bad"] is None else a["bad"].ctypes.data_as(u8p), n, n_c,
            0.0 if a["window_length"] is None else a["window_length"], a["break_tolerance"], a["sigma_upper"], a["sigma_lower"],
            a["max_run"], a["n_iter"], a["min_points"], _dp(rows), flags.ctypes.data_as(u8p),
            record.ctypes.data_as(ctypes.c_void_p)))
        if a["single"]:
            rows, flags, record = rows[0], flags[0], record[0]
        out = (rows,) + ((flags,) if return_flags else ()) + ((record,) if return_record else ())
        return out[0] if len(out) == 1 else out

    def debug_null_words(self, n, n_rows, seed, first_trial=0, block=None):
        """The raw Philox words [n_rows, W] tls_null_rows draws for these trials (tls_debug_null_words): white-noise
        layout when `block` is None, the bootstrap's otherwise."""
        n, n_rows = int(n), int(n_rows)
        words = 2 * n if block is None else -(-n // int(block)) if int(block) >= 1 else 1
        out = numpy.empty((n_rows, 4 * (-(-words // 4))), dtype=numpy.uint64)
        self._check(self._lib.tls_debug_null_words(self._h, n, n_rows, int(seed), int(first_trial), 0 if block is None else 1,
                                                   0 if block is None else int(block),
                                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def debug_cumsum(self, values, threads=512):
        """[0, cumsum(values)] computed by the kernel's exact parallel sequential-order scan."""
        v = _f8(values)
        out = numpy.empty(len(v) + 1, dtype=numpy.float64)
        self._check(self._lib.tls_debug_cumsum(self._h, _dp(v), len(v), _dp(out), int(threads)))
        return out

    def debug_post_search(self, y_batch, chi2, row, depth, median_kernel, with_fits=False):
        """Developer/test entry: tls_power_batch's post-search chain (spectra, pick, final T0 fit) on the prepared plan (prepare())
        with injected search results chi2 / row / depth [n_curves, n_periods] and flux y_batch [n_curves, n]; the summaries.
        with_fits: also (epochs, residuals) -- lists of every fit's trial epochs and residuals -- and handed_back [n_curves]
        (1: the rotation path handed the fit to the general kernel, 0: it did not, -1: it did not run)."""
        y_batch = numpy.ascontiguousarray(y_batch, dtype=numpy.float64)
        chi2 = numpy.ascontiguousarray(chi2, dtype=numpy.float64)
        row = numpy.ascontiguousarray(row, dtype=numpy.int64)
        depth = numpy.ascontiguousarray(depth, dtype=numpy.float64)
        if y_batch.ndim != 2 or chi2.ndim != 2 or chi2.shape != row.shape or chi2.shape != depth.shape \
                or len(chi2) != len(y_batch) or chi2.shape[1] != self._n_periods:
            raise ValueError("chi2, row, depth must have shape [n_curves, n_periods] of the prepared plan, y_batch [n_curves, n]")
        summary = numpy.zeros(len(chi2), dtype=POWER_SUMMARY_DTYPE)
        n_c = len(chi2)
        ep, res = numpy.empty(y_batch.shape), numpy.empty(y_batch.shape)
        n_ep, back = numpy.empty(n_c, dtype=numpy.int64), numpy.empty(n_c, dtype=numpy.int64)
        self._invalidate_results()
        self._check(self._lib.tls_debug_post_search(self._h, _dp(y_batch), n_c, _dp(chi2), _ip(row), _dp(depth),
                                                    int(median_kernel), summary.ctypes.data_as(ctypes.c_void_p),
                                                    *((_dp(ep), _dp(res), _ip(n_ep), _ip(back)) if with_fits else (None,) * 4)))
        if with_fits:
            return summary, [ep[c, :n_ep[c]] for c in range(n_c)], [res[c, :n_ep[c]] for c in range(n_c)], back
        return summary

    def device_bytes(self):
        """(total, t0_fit_scratch): bytes of device memory the context holds, in all and as the final T0 fit's HBM scratch."""
        total, scratch = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.tls_debug_device_bytes(self._h, ctypes.byref(total), ctypes.byref(scratch)))
        return int(total.value), int(scratch.value)

    def perm_table(self):
        """The held plan's table of folded orders (four-slot kernel): `bytes` (0 when the plan has none), `filled` once a
        launch of the plan has stored it (later launches read it and sort nothing), and `plan_reuses`, the prepare() calls the
        context has answered from a held plan (they keep the table)."""
        size, filled, reuses = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.tls_debug_perm_table(self._h, ctypes.byref(size), ctypes.byref(filled), ctypes.byref(reuses)))
        return {"bytes": int(size.value), "filled": bool(filled.value), "plan_reuses": int(reuses.value)}

    def lanes(self):
        """Search launches the context has sent to launch lane A (`a`) and lane B (`b`) so far, and whether the lanes are
        `on` (switch `lanes`): back-to-back execute() calls of a filled four-slot plan alternate between the two."""
        a, b, on = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.tls_debug_lanes(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(on)))
        return {"a": int(a.value), "b": int(b.value), "on": bool(on.value)}

    def launch_ms(self):
        """What kernel_timing charges each launch it holds, in ms: an overlapped launch is charged the shorter of its own
        event pair and the time from the end of the launch before it to its own end."""
        n = self._lib.tls_debug_launch_ms(self._h, None, 0)
        if n < 0:
            self._check(n)
        out = numpy.zeros(max(n, 1), dtype=numpy.float64)
        n = self._lib.tls_debug_launch_ms(self._h, _dp(out), len(out))
        if n < 0:
            self._check(n)
        return out[:n]

    def folded(self, n_periods, n):
        """Developer/test entry: the folded flux of every period of the prepared plan, (n_periods, n), as the
        kernel's sort left it."""
        self._invalidate_results()
        out = numpy.empty((int(n_periods), int(n)), dtype=numpy.float64)
        self._check(self._lib.tls_debug_folded(self._h, _dp(out), out.size))
        return out

    def prefix_sums(self, n_periods):
        """Developer/test entry: the prefix sum C[0..M] of the patched folded flux of every period, (n_periods, M + 1)."""
        self._invalidate_results()
        row = ctypes.c_int64(0)
        self._check(self._lib.tls_debug_prefix(self._h, None, 0, ctypes.byref(row)))
        out = numpy.empty((int(n_periods), int(row.value)), dtype=numpy.float64)
        self._check(self._lib.tls_debug_prefix(self._h, _dp(out), out.size, ctypes.byref(row)))
        return out

    def phase_cycles(self):
        """Developer instrumentation: per-phase shader-cycle sums of the last
        execute(phase_clock=True)."""
        arr = (ctypes.c_uint64 * 42)()
        self._check(self._lib.tls_debug_phase_cycles(self._h, arr, 42))
        names = ("fold_count", "scan", "scatter", "rank", "gather_patch", "cumsum", "batch_prefix",
                 "chi2", "e_convert", "predicate_strided", "cumsum_blocks", "cumsum_fallbacks",
                 "tile_staging", "predicate_dense", "cs_A", "cs_B1", "cs_B2", "cs_scan", "screen_split", "screen_resolve",
                 "tile_wait", "chi2_wait", "prune_e2", "prune_bounds", "prune_incumbent", "select_relist",
                 "slab_copy_in", "slab_copy_out", "part_fold", "part_scan", "part_lds", "part_store",
                 "stat_live_units", "stat_kept_units", "stat_singles", "stat_batches", "stat_pruned_periods",
                 "stat_exact_retries", "stat_screen_parked", "stat_screen_valued", "stat_register_scans",
                 "claim")   # (four-slot kernel: a period's last barrier to the next period's first phase)
        return dict(zip(names, [int(v) for v in arr]))

    def period_cycles(self):
        """Developer instrumentation: shader cycles per period of the prepared plan (one more search)."""
        self._invalidate_results()
        out = numpy.zeros(self._n_periods, dtype=numpy.uint64)
        self._check(self._lib.tls_debug_period_cycles(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                      len(out)))
        return out

    def batch_group_ms(self, with_wait=False):
        """Host wall time (ms) of every group of 32 light curves of the last power_batch / search_batch call; with_wait: also
        the part of each group's time spent in its one wait for the device (power_batch)."""
        n = self._lib.tls_debug_batch_group_ms(self._h, None, 0)
        out = numpy.zeros(2 * max(n, 0), dtype=numpy.float64)
        if n > 0:
            self._lib.tls_debug_batch_group_ms(self._h, _dp(out), 2 * n)
        return (out[:n], out[n:]) if with_wait else out[:n]

    def check_counts(self):
        """(checked_build, {check name: violations}) -- device-side bound checks of the debug build."""
        arr = (ctypes.c_uint64 * 17)()
        rc = self._lib.tls_debug_check_counts(self._h, arr, 17)
        if rc < 0:
            self._check(rc)
        names = ("lds_carve", "list_capacity", "dot_window", "predicate_read", "sort_window", "work_item",
                 "singles_capacity", "tile_stage", "screen_split", "detrend_slot",
                 "biweight_slot", "sysrem_index", "single_window", "times_window", "shape_index", "views_range",
                 "noise_window")
        return bool(rc), dict(zip(names, [int(v) for v in arr]))

    def poison_lds(self, word=0x7ff80000):
        """Test entry: every CU's LDS filled with `word` (default: fp64 NaNs) and every device buffer a call fills for itself
        smeared with 0xFF bytes (DESIGN.md section 7 lists them), on the context's stream."""
        self._check(self._lib.tls_debug_poison_lds(self._h, int(word)))

    def synchronize(self):
        self._check(self._lib.tls_synchronize(self._h))

    def execute_timed(self, reps=1):
        self._invalidate_results()
        ms = ctypes.c_double(0.0)
        self._check(self._lib.tls_execute_timed(self._h, int(reps), ctypes.byref(ms)))
        return ms.value

    def fetch(self, with_counters=False):
        n = self._n_periods
        chi2 = numpy.empty(n, dtype=numpy.float64)
        row = numpy.empty(n, dtype=numpy.int64)
        depth = numpy.empty(n, dtype=numpy.float64)
        c = Counters()
        self._check(self._lib.tls_fetch(self._h, _dp(chi2), _ip(row), _dp(depth), ctypes.byref(c)))
        # exactly this array, at this generation of the context, with these values is what the device still holds
        self._resident_chi2 = (weakref.ref(chi2), self._generation, self._fingerprint(chi2))
        if with_counters:
            return chi2, row, depth, c.as_dict()
        return chi2, row, depth

    def kernel_timing(self, reset=True):
        """(total ms, launches) of the search kernel since the last reset (HIP events)."""
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._check(self._lib.tls_kernel_timing(self._h, 1 if reset else 0, ctypes.byref(ms),
                                                ctypes.byref(n)))
        return ms.value, n.value

    def plan_info(self):
        c = Counters()
        lds, blocks, res = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.tls_plan_info(self._h, ctypes.byref(c), ctypes.byref(lds),
                                            ctypes.byref(blocks), ctypes.byref(res)))
        d = c.as_dict()
        d.update(lds_bytes=lds.value, n_blocks=blocks.value, resident=bool(res.value))
        return d

    def last_kernel(self):
        """Name of the search kernel the last execute launched (include/tls_amd.h, tls_last_kernel)."""
        return self._lib.tls_last_kernel(self._h).decode()

    # -- RCCL
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        rc = self._lib.tls_comm_unique_id(buf)
        if rc != 0:
            raise RuntimeError("tls_amd: ncclGetUniqueId failed: "
                               + self._lib.tls_last_error(None).decode())
        return buf.raw

    def comm_init(self, n_ranks, rank, unique_id):
        assert len(unique_id) == 128
        self._check(self._lib.tls_comm_init(self._h, int(n_ranks), int(rank), unique_id))

    def comm_destroy(self):
        self._check(self._lib.tls_comm_destroy(self._h))

    def comm_info(self):
        """(ranks, this rank, device) as RCCL reports them for the communicator; (0, -1, -1) without one."""
        n, r, d = ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_int(-1)
        self._check(self._lib.tls_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(d)))
        return n.value, r.value, d.value

    def comm_ranks(self):
        return self.comm_info()[0]

    def comm_allgather_results(self, count_per_rank, n_ranks):
        total = int(count_per_rank) * int(n_ranks)
        chi2 = numpy.empty(total, dtype=numpy.float64)
        row = numpy.empty(total, dtype=numpy.int64)
        depth = numpy.empty(total, dtype=numpy.float64)
        self._check(self._lib.tls_comm_allgather_results(self._h, int(count_per_rank), _dp(chi2),
                                                         _ip(row), _dp(depth)))
        return chi2, row, depth

    def comm_allgather_device(self, count_per_rank):
        """Enqueue pack + ncclAllGather behind the search; the batch stays device resident."""
        self._check(self._lib.tls_comm_allgather_device(self._h, int(count_per_rank)))

    def comm_stage_results(self, count_per_rank, slot, n_slots):
        """Survey mode: park the latest results as slot `slot` (device copies, no communication)."""
        self._check(self._lib.tls_comm_stage_results(self._h, int(count_per_rank), int(slot), int(n_slots)))

    def comm_allgather_staged(self, count_per_rank, n_slots):
        """ONE ncclAllGather of all staged slots, enqueued on the search stream."""
        self._check(self._lib.tls_comm_allgather_staged(self._h, int(count_per_rank), int(n_slots)))

    def comm_fetch_staged(self, count_per_rank, n_slots, slot, n_ranks):
        n = int(count_per_rank) * int(n_ranks)
        chi2 = numpy.empty(n, dtype=numpy.float64)
        row = numpy.empty(n, dtype=numpy.int64)
        depth = numpy.empty(n, dtype=numpy.float64)
        self._check(self._lib.tls_comm_fetch_staged(self._h, int(count_per_rank), int(n_slots), int(slot),
                                                    _dp(chi2), _ip(row), _dp(depth)))
        return chi2, row, depth

    def comm_fetch_gathered(self, count_per_rank, n_ranks):
        total = int(count_per_rank) * int(n_ranks)
        chi2 = numpy.empty(total, dtype=numpy.float64)
        row = numpy.empty(total, dtype=numpy.int64)
        depth = numpy.empty(total, dtype=numpy.float64)
        self._check(self._lib.tls_comm_fetch_gathered(self._h, int(count_per_rank), _dp(chi2), _ip(row),
                                                      _dp(depth)))
        return chi2, row, depth

    def comm_barrier(self):
        self._check(self._lib.tls_comm_barrier(self._h))

    def comm_max(self, value):
        v = ctypes.c_double(float(value))
        self._check(self._lib.tls_comm_max(self._h, ctypes.byref(v)))
        return v.value


def grid_cells(t, periods, table, params):
    """Trial cells each period enumerates (host-only planning call, needs no GPU)."""
    lib = load()
    t, periods = _f8(t), _f8(periods)
    arrays, tm, pr = Context._pack(table, params)
    out = numpy.zeros(len(periods), dtype=numpy.int64)
    rc = lib.tls_grid_cells(_dp(t), len(t), _dp(periods), len(periods), ctypes.byref(tm),
                            ctypes.byref(pr), _ip(out))
    if rc != 0:
        raise RuntimeError("tls_amd error %d: %s" % (rc, lib.tls_last_error(None).decode()))
    return out


def candidate_slabs(curve, n_fits, max_curves, max_fits):
    """(slab of every candidate, slot of its curve in that slab, row copies of every slab): how the per-candidate
    stages cut n_fits candidates into slabs (host-only, needs no GPU).  curve None: candidate f reads curve f."""
    lib = load()
    curve = None if curve is None else _i8(curve)
    slab, slot, runs = (numpy.zeros(max(n_fits, 0), dtype=numpy.int64) for _ in range(3))
    n_slabs = ctypes.c_int64(0)
    rc = lib.tls_debug_candidate_slabs(None if curve is None else _ip(curve), n_fits, max_curves, max_fits, _ip(slab),
                                       _ip(slot), _ip(runs), ctypes.byref(n_slabs))
    if rc != 0:
        raise RuntimeError("tls_amd error %d: %s" % (rc, lib.tls_last_error(None).decode()))
    return slab, slot, runs[:n_slabs.value].copy()


def period_costs(t, periods, table, params, sigma, with_slots=False, options=None):
    """(trial cells, expected template taps, modelled search time) of every period: what the shard
    boundaries are placed by (host-only planning call, needs no GPU).  options: the switches of the context
    that will search (Context.get_options()) -- the model follows the kernel variant and prefix-sum mode they
    select; None: the process's (its TLS_* environment, read once)."""
    lib = load()
    t, periods = _f8(t), _f8(periods)
    arrays, tm, pr = Context._pack(table, params)
    cells = numpy.zeros(len(periods), dtype=numpy.int64)
    taps = numpy.zeros(len(periods), dtype=numpy.float64)
    time = numpy.zeros(len(periods), dtype=numpy.float64)
    slots = ctypes.c_int64(0)
    opt = None if options is None else switches_text({k: v for k, v in options.items() if v is not None and float(v) >= 0}).encode()
    rc = lib.tls_period_costs(_dp(t), len(t), _dp(periods), len(periods), ctypes.byref(tm), ctypes.byref(pr),
                              float(sigma), _ip(cells), _dp(taps), _dp(time), ctypes.byref(slots), opt)
    if rc != 0:
        raise RuntimeError("tls_amd error %d: %s" % (rc, lib.tls_last_error(None).decode()))
    if with_slots:
        return cells, taps, time, int(slots.value)
    return cells, taps, time


def device_count():
    lib = load()
    n = lib.tls_device_count()
    if n < 0:
        raise RuntimeError("tls_amd: " + lib.tls_last_error(None).decode())
    return n
