"""The cases of tests/test_stage_memory.py (the device) and tests/test_stage_memory_host.py (the coverage): every survey stage
and every kernel of the post-search chain on the smallest EXISTING input on each side of every memory path the kernel has --
the LDS and the device scratch beyond it, one chunk and several, one tile and two, the small product kernel and the large.

No input is made here.  Every case takes the arrays of the stage's own GPU test or case module (whose premises -- ties, clear
picks, bounds -- the stage's host test checks), and is compared as that test compares: bit for bit where it says so, within
its stated bound elsewhere.  A case names

    stage    the stage it belongs to (the pairs of test_small_call_behind_a_large_one are formed within a stage)
    entry    the C entry it exercises
    method   the Context method that launches it
    run      a callable on a Context: the outputs, a tuple of arrays (prepare() included where the entry needs a plan)
    want     the statement's outputs from the stage's *_spec.py, evaluated on the CPU (None: see below);
             want_on_device: the statement itself runs a kernel (peak_fits_spec takes its T0 fit from tls_t0_fit), and is
             given a context of its own
    compare  compare(got, want): the stage's own comparison
    size     what the case's side of a constant is read from, without running it (see PAIRS)

Cases without a statement: the power_batch entries.  Their statement is power() through the same device and the CPU oracle
(tests/test_power_batch_chain.py, test_power_batch_statistics.py, test_power_batch_results.py); here they are held to
themselves under the three poison words and to a fresh context.

PAIRS lists, for every stage with two memory paths, (the _lib constant's value, the case below or at it, the case above it);
test_stage_memory_host.py checks that the sizes straddle."""
import collections
import functools
import glob
import os
import warnings

import numpy

from tls_amd import _lib, stats, survey, synthetic
from tls_amd.stats import calculate_fill_factor

Case = collections.namedtuple("Case", ("stage", "entry", "method", "run", "want", "compare", "size", "want_on_device"))
CASES = collections.OrderedDict()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def add(name, stage, entry, method, run, want=None, compare=None, size=None, want_on_device=False):
    assert name not in CASES, name
    CASES[name] = Case(stage, entry, method, run, want, compare, size, want_on_device)


def arrays(out):
    """The outputs of a call as a flat list of contiguous arrays (dicts in key order, None left out)."""
    if out is None:
        return []
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in arrays(out[k])]
    if isinstance(out, (tuple, list)):
        return [a for v in out for a in arrays(v)]
    return [numpy.ascontiguousarray(out)]


def quiet(fn, *args, **kw):
    with warnings.catch_warnings(), numpy.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args, **kw)


def fields_equal(got, want, names, what):
    """Every field bit for bit as the stages' tests hold it: assert_array_equal as floats, NaN equal to NaN."""
    for k in names:
        numpy.testing.assert_array_equal(numpy.asarray(got[k], dtype=float), numpy.asarray(want[k], dtype=float),
                                         err_msg=str((what, k)))


def columns_equal(got, want, names, what):
    """A structured array of the device against the statement's [n, fields] array."""
    for i, k in enumerate(names):
        numpy.testing.assert_array_equal(numpy.asarray(got[k], dtype=float), want[:, i], err_msg=str((what, k)))


# ---- pre-whitening: PREWHITEN_LDS_POINTS -----------------------------------------------------------------------------------------
def _prewhiten(name):
    import prewhiten_cases
    import test_prewhiten

    def case():
        return prewhiten_cases.cases()[name]

    def run(ctx):
        c = case()
        flat, trend, info = ctx.prewhiten(c.t, c.y, c.f, c.n_terms, c.harmonics, c.min_power, dy=c.dy, return_trend=True,
                                          debug=True)
        return flat, trend, info["terms"], info["n_iterations"], info["status"], info["steps"], info["sums"]

    def compare(got, want):
        c = case()
        flat, trend = got[0], got[1]
        info = dict(terms=got[2], n_iterations=got[3], status=got[4], steps=got[5], sums=got[6])
        for curve in range(len(c.y)):
            test_prewhiten.check_curve(c, curve, flat, trend, info, want[curve])

    add("prewhiten_" + name, "prewhiten", "tls_prewhiten", "prewhiten", run, lambda: prewhiten_cases.statement(name), compare,
        size=lambda: len(case().t))


for _name in ("lds_side", "global_side", "n256_c3_dy_h2"):
    _prewhiten(_name)


# ---- shape fit: SHAPE_LDS_MEMBERS (the n = 20000 case of test_shape_fit.py, the windows on either side) -------------------------
@functools.lru_cache(maxsize=None)
def _shape_inputs():
    import test_shape_fit as m
    t = m.series(20000)
    P, d = 8.0, 0.25
    y = m.dips(t, P, t[0] + 3.0, 0.25, seed=3)
    return t, numpy.atleast_2d(y), numpy.full((1, len(t)), 1e-3), [P], [t[0] + 3.0], [d]


def _shape(name, window):
    import shape_fit_spec as spec
    import test_shape_fit as m
    tables = (m.RATIOS, m.INGRESS, m.SHIFTS)

    def run(ctx):
        t, y, dy, period, T0, duration = _shape_inputs()
        return (ctx.shape_fit(t, y, dy, period, T0, duration, *tables, window=window),)

    @functools.lru_cache(maxsize=None)
    def want():
        t, y, dy, period, T0, duration = _shape_inputs()
        return spec.shape_fit_batch(t, y, dy, period, T0, duration, numpy.arange(1), *tables, window=window)

    add(name, "shape_fit", "tls_shape_fit", "shape_fit", run, want,
        lambda got, w: columns_equal(got[0], w, spec.FIELDS, name), size=lambda: int(want()[0, spec.FIELDS.index("n_points")]))


_shape("shape_fit_members_in_lds", 1.5625)
_shape("shape_fit_members_beyond_lds", 1.625)


# ---- centroid test: CENTROID_LDS_EPOCHS -------------------------------------------------------------------------------------------
def _centroid(name, make):
    import centroid_cases as cases
    import centroid_spec as spec
    case = functools.lru_cache(maxsize=None)(make)
    want = functools.lru_cache(maxsize=None)(lambda: cases.expected(case()))

    def run(ctx):
        c = case()
        return (ctx.centroid_test(c["t"], c["y"], c["cx"], c["cy"], c["period"], c["T0"], c["duration"], c["b"], curve=c["curve"],
                                  **c["options"]),)

    def compare(got, w):
        fields_equal(got[0], w, spec.FIELDS, name)
        case()["check"](got[0])

    add(name, "centroid_test", "tls_centroid_test", "centroid_test", run, want, compare,
        size=lambda: int(numpy.nanmax(want()["n_epochs"])))


def _centroid_small():
    import centroid_cases
    return centroid_cases.sizes()[0]


def _centroid_large():
    import centroid_cases
    return centroid_cases.many_epochs()


_centroid("centroid_epochs_in_lds", _centroid_small)
_centroid("centroid_epochs_beyond_lds", _centroid_large)


# ---- phase scan: PHASE_SCAN_CHUNK; max_bins 16 and the default (test_phase_scan.test_series_lengths) -------------------------------
def _phase_scan(name, n, **kw):
    import phase_scan_spec as spec
    import test_phase_scan as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        t = numpy.linspace(3.0, 3.0 + n / 48.0, n)
        y = numpy.array([m.noisy(t, n), m.noisy(t, n + 1, depth=4e-3)])
        q = numpy.array([40.5, 300.5, 1999.5, 4096.5])
        return t, y, numpy.full(8, 2.0), numpy.full(8, 3.3), numpy.tile(4.0 / q, 2), numpy.repeat([0, 1], 4)

    def run(ctx):
        t, y, period, T0, duration, curve = inputs()
        return (survey.phase_scan(t, y, period, T0, duration, curve=curve, context=ctx, **kw),)

    def want():
        t, y, period, T0, duration, curve = inputs()
        return [spec.expected(t, y[curve[f]], period[f], T0[f], duration[f], **kw) for f in range(len(period))]

    def compare(got, w):
        assert got[0].dtype.names == survey.phase_scan_fields()
        for f, rec in enumerate(w):
            for k in got[0].dtype.names:
                numpy.testing.assert_array_equal(numpy.asarray(got[0][k][f], dtype=float),
                                                 numpy.asarray(rec["status" if k == "scan_status" else k], dtype=float),
                                                 err_msg=str((name, f, k)))

    add(name, "phase_scan", "tls_phase_scan", "phase_scan", run, want, compare, size=lambda: n)


_phase_scan("phase_scan_one_chunk", 1920)
_phase_scan("phase_scan_two_chunks", _lib.PHASE_SCAN_CHUNK + 1)
_phase_scan("phase_scan_16_bins", 1920, max_bins=_lib.PHASE_SCAN_MIN_BINS)


# ---- single transits: SINGLE_TILE (test_single_transit.test_series_lengths_around_the_tile, the widest widths of the module) ------
def _single(name, n):
    import single_transit_spec as spec
    import test_single_transit as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        t = m.series(n)
        y = m.curves(n, 2, n)
        return t, y, numpy.full(y.shape, 1e-3), m.WIDTHS, m.shapes_of(m.WIDTHS), m.spans_of(t, m.WIDTHS)

    def run(ctx):
        return ctx.single_transits(*inputs(), with_arrays=True, k=6)

    def compare(got, w):
        fields_equal(got[0], w[0], spec.FIELDS, name)
        for a, b, what in zip(got[1:], w[1:], ("n_events", "ses", "row", "depth")):
            numpy.testing.assert_array_equal(numpy.asarray(a, dtype=float), numpy.asarray(b, dtype=float), err_msg=str((name, what)))

    add(name, "single_transits", "tls_single_transits", "single_transits", run, lambda: spec.expected(*inputs(), k=6), compare,
        size=lambda: n)


_single("single_transits_one_tile", _lib.SINGLE_TILE)
_single("single_transits_tile_and_one", _lib.SINGLE_TILE + 1)


# ---- transit times and event vetting: the (epoch, shift) units of a candidate against the LDS chunk -------------------------------
def chunk_epochs(reach):
    """The epochs of one LDS chunk of tls_transit_times / tls_event_vetting at this reach (tls_times.hip.h times_chunk_epochs)."""
    return max(1, (2 * _lib.TIMES_MAX_REACH + 1) // (2 * int(reach) + 1))


@functools.lru_cache(maxsize=None)
def _times_inputs():
    """test_transit_times.test_units_threads_and_chunks."""
    import test_transit_times as m
    n = 650
    t = m.series(n)
    rng = numpy.random.RandomState(8)
    dy = rng.uniform(5e-4, 2e-3, (2, n))
    P40, P3 = 16 * m.DT, 300 * m.DT
    y = numpy.array([m.dips(t, P40, t[5], 5, seed=9), m.dips(t, P3, t[20], 37, seed=10)])
    period = numpy.array([P40, P3, P3, P40, P40, P40])
    T0 = numpy.array([t[5], t[20], t[20], t[5], t[5], t[5]])
    return t, y, dy, period, T0, numpy.array([2, 4, 4, 1, 0, 3]), numpy.array([8, 1, 4096, 100, 300, 102]), numpy.array([0, 1, 1, 0, 0, 0])


def _times(name, f):
    import test_transit_times as m
    import transit_times_spec as spec

    def run(ctx):
        t, y, dy, period, T0, row, reach, curve = _times_inputs()
        return ctx.transit_times(t, y, dy, period[[f]], T0[[f]], row[[f]], reach[[f]], m.WIDTHS, m.shapes_of(m.WIDTHS),
                                 m.spans_of(m.WIDTHS), curve=curve[[f]], max_epochs=48)

    @functools.lru_cache(maxsize=None)
    def want():
        t, y, dy, period, T0, row, reach, curve = _times_inputs()
        return spec.expected(t, y, dy, curve[[f]], period[[f]], T0[[f]], row[[f]], reach[[f]], m.shapes_of(m.WIDTHS),
                             m.spans_of(m.WIDTHS), max_epochs=48)

    def compare(got, w):
        fields_equal(got[0], w[0], spec.EPHEMERIS_FIELDS, name)
        fields_equal(got[1], w[1], spec.TIME_FIELDS, name)

    add(name, "transit_times", "tls_transit_times", "transit_times", run, want, compare,
        size=lambda: (int(want()[0]["n_epochs"][0]), chunk_epochs(_times_inputs()[6][f])))


_times("transit_times_one_chunk", 0)
_times("transit_times_four_chunks", 4)


@functools.lru_cache(maxsize=None)
def _events_case():
    import event_vetting_cases as cases
    return next(c for c in cases.edge_cases() if c["label"] == "units")


def _events(name, f):
    import event_vetting_cases as cases
    import event_vetting_spec as spec
    which = numpy.array([f])

    def run(ctx):
        c = _events_case()
        return ctx.event_vetting(c["t"], c["y"], c["dy"], c["period"][which], c["T0"][which], c["row"][which], c["reach"][which],
                                 c["chase_reach"][which], c["guard"][which], c["chase_span"][which], c["widths"],
                                 cases.shapes_of(c["widths"]), c["span_max"], curve=c["curve"][which], **c["options"])

    want = functools.lru_cache(maxsize=None)(lambda: cases.expected(_events_case(), which=which))

    def compare(got, w):
        fields_equal(got[0], w[0], spec.SUMMARY_FIELDS, name)
        fields_equal(got[1], w[1], spec.EVENT_FIELDS, name)

    add(name, "event_vetting", "tls_event_vetting", "event_vetting", run, want, compare,
        size=lambda: (int(want()[0]["n_epochs"][0]), chunk_epochs(_events_case()["reach"][f])))


_events("event_vetting_one_chunk", 0)
_events("event_vetting_two_chunks", 2)


# ---- tls_find_peaks: PEAKS_LDS_PERIODS ----------------------------------------------------------------------------------------------
def _peaks(name, inputs, size):
    import peaks_spec
    inputs = functools.lru_cache(maxsize=None)(inputs)

    def run(ctx):
        power, periods, k, sep, ratios = inputs()
        return ctx.find_peaks(power, periods, k, sep, ratios)

    def want():
        power, periods, k, sep, ratios = inputs()
        return [peaks_spec.expected(row, periods, k, sep, ratios) for row in numpy.atleast_2d(power)]

    def compare(got, w):
        import test_peaks
        peaks, n_peaks = got
        for r, (rec, m) in enumerate(w):
            assert n_peaks[r] == m, (name, r)
            for field in rec.dtype.names:
                assert test_peaks.same_bits(peaks[r][field][:m], rec[field][:m]), (name, r, field)
            for field in ("period", "power", "chi2", "depth"):
                assert numpy.isnan(peaks[r][field][m:]).all(), (name, r, field)
            assert (peaks[r]["index"][m:] == -1).all() and (peaks[r]["row"] == -1).all(), (name, r)

    add(name, "find_peaks", "tls_find_peaks", "find_peaks", run, want, compare, size=size)


def _peaks_small():
    """test_peaks.test_crafted_rows_at_the_wave_and_workgroup_edges at n = 1025."""
    import peaks_spec
    import test_peaks as m
    return m.crafted_rows(1025, seed=1025), m.grid(1025), 3, 0.02, peaks_spec.HARMONICS


def _peaks_large():
    """test_peaks.test_one_row_past_the_lds_mask."""
    import peaks_spec
    import test_peaks as m
    n = _lib.PEAKS_LDS_PERIODS + 1
    power = m.smooth_spectrum(n, 13)
    power[-1] = power.max() + 1.0
    return power, 1.0 / numpy.linspace(1 / 0.6, 1 / 730.0, n), 8, 0.02, peaks_spec.HARMONICS


_peaks("find_peaks_mask_in_lds", _peaks_small, lambda: 1025)
_peaks("find_peaks_mask_in_device_memory", _peaks_large, lambda: _lib.PEAKS_LDS_PERIODS + 1)


# ---- Lomb-Scargle and nudft: GLS_SMALL_ROWS, F no multiple of GLS_FREQ_TILE, n no multiple of GLS_CHUNK, with and without dy -------
def _gls(name, R, with_dy):
    """test_gls.test_periodogram_equals_the_statement."""
    import gls_spec as spec
    import test_gls as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        t = m.series(330, gap_at=120, gap=70)
        y, dy = m.curves(t, R, seed=R, dy=with_dy)
        f = survey.variability_frequencies(t, oversampling=2, f_max=12.0)[::-1].copy()
        f[5] = f[17]
        return t, y, dy, f

    def run(ctx):
        t, y, dy, f = inputs()
        got = ctx.lomb_scargle(t, y, f, dy=dy, debug=True)
        return tuple(got[k] for k in ("mean", "variance", "rows", "weights", "sums", "power", "amplitude", "phase"))

    def want():
        t, y, dy, f = inputs()
        pro = [spec.prologue(y[r], None if dy is None else dy[r]) for r in range(R)]
        a = numpy.array([p[1] for p in pro])
        w = numpy.array([p[0] for p in pro])
        shared = w if dy is not None else w[:1]
        return dict(pro=pro, a=a, w=w, yc=spec.exact_sums(t, a, f), c=spec.exact_sums(t, shared, f), c2=spec.exact_sums(t, shared, 2.0 * f),
                    bound_a=spec.sum_bound(t, a, f), bound_w=spec.sum_bound(t, w, f), bound_w2=spec.sum_bound(t, w, 2.0 * f))

    def compare(got, w):
        t, y, dy, f = inputs()
        mean, variance, rows, weights, sums, power, amplitude, phase = got
        pro = w["pro"]
        m.same(mean, [p[2] for p in pro], (name, "mean"))
        m.same(variance, [p[3] for p in pro], (name, "variance"))
        m.same(rows, [p[1] for p in pro], (name, "rows"))
        m.same(weights, pro[0][0] if dy is None else [p[0] for p in pro], (name, "weights"))
        assert sums.shape == (R, len(f), 6)
        m.within(sums[:, :, 0:2], w["yc"], w["bound_a"], (name, "YC YS"))
        m.within(sums[:, :, 2:4], numpy.broadcast_to(w["c"], (R, len(f), 2)), w["bound_w"], (name, "C S"))
        m.within(sums[:, :, 4:6], numpy.broadcast_to(w["c2"], (R, len(f), 2)), w["bound_w2"], (name, "C2 S2"))
        p, amp, ph = spec.epilogue(*numpy.moveaxis(sums, 2, 0), variance[:, None])
        m.same(power, p, (name, "power"))
        m.same(amplitude, amp, (name, "amplitude"))
        m.phase_close(phase, ph, (name, "phase"))

    add(name, "lomb_scargle", "tls_lomb_scargle", "lomb_scargle", run, want, compare,
        size=lambda: dict(rows=R, n=len(inputs()[0]), F=len(inputs()[3])))


_gls("lomb_scargle_3_rows", 3, False)
_gls("lomb_scargle_3_rows_dy", 3, True)
_gls("lomb_scargle_40_rows", 40, False)
_gls("lomb_scargle_40_rows_dy", 40, True)


def _nudft(name, R, F, n):
    """test_gls.test_nudft_at_the_edges_of_the_tiles."""
    import gls_spec as spec
    import test_gls as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        rng = numpy.random.RandomState(R * 1000 + F + n)
        t = m.series(n, gap_at=n // 2, gap=40)
        rows = rng.normal(0, 1, (R, n))
        return rows, t, numpy.sort(rng.uniform(0.05, 30.0, F))

    def want():
        rows, t, f = inputs()
        return spec.exact_sums(t, rows, f), spec.sum_bound(t, rows, f)

    add(name, "nudft", "tls_nudft", "nudft", lambda ctx: (ctx.nudft(*inputs()),), want,
        lambda got, w: m.within(got[0], w[0], w[1], name), size=lambda: dict(rows=R, n=n, F=F))


_nudft("nudft_31_rows", 31, 63, 31)
_nudft("nudft_33_rows", 33, 65, 33)


# ---- sine test: with and without mask and dy -------------------------------------------------------------------------------------
class _Replay(object):
    """Stands where a stage's own check expects a Context: hands the outputs of a run already made to the one method the check
    calls, so that the check's comparison is applied to them as it stands."""

    def __init__(self, method, out):
        self._method, self._out = method, out

    def __getattr__(self, name):
        if name != self._method:
            raise AttributeError(name)
        return lambda *args, **kw: self._out


def _sine(name, inputs):
    import gls_spec as spec
    import test_gls as m
    inputs = functools.lru_cache(maxsize=None)(inputs)

    def run(ctx):
        t, y, dy, period, kw = inputs()
        return ctx.sine_test(t, y, period, dy=dy, debug=True, **kw)

    def want():
        """The statement of every candidate (test_gls.check_sine forms it again while it compares)."""
        t, y, dy, period, kw = inputs()
        T0, duration, curve = kw.get("T0"), kw.get("duration"), kw["curve"]
        return [spec.sine_test(t, y[c], period[i], None if dy is None else dy[c], None if T0 is None else T0[i],
                               None if T0 is None else duration[i], 1.5, (0.5, 1.0, 2.0)) for i, c in enumerate(curve)]

    def compare(got, w):
        t, y, dy, period, kw = inputs()
        m.check_sine(_Replay("sine_test", got), t, y, dy, period, label=name, **kw)

    add(name, "sine_test", "tls_sine_test", "sine_test", run, want, compare)


def _sine_plain():
    """test_gls.test_sine_test_without_a_mask at n = 257, no dy."""
    import test_gls as m
    t = m.series(257, gap_at=128, gap=20)
    y, dy = m.curves(t, 3, seed=257, dy=False)
    return t, y, dy, [1.1, 0.7, 3.0, 0.7, 2.2], dict(curve=[2, 0, 1, 0, 2])


def _sine_masked():
    """test_gls.test_sine_test_masks: masks and dy."""
    import test_gls as m
    t = m.series(300)
    y, dy = m.curves(t, 2, seed=41, dy=True)
    P = 1024.0
    T0 = [t[0]] * 3 + [t[7], numpy.nan, t[7], t[7], t[7]]
    d = [(296.5 / 64) / 0.75, (295.5 / 64) / 0.75, (290.5 / 64) / 0.75, 0.125, 0.125, numpy.nan, 0.0, 0.125]
    return t, y, dy, [P, P, P, 0.75, 0.75, 0.75, 0.75, numpy.inf], dict(T0=T0, duration=d, curve=[0, 0, 1, 1, 1, 0, 0, 0])


_sine("sine_test_no_mask_no_dy", _sine_plain)
_sine("sine_test_mask_and_dy", _sine_masked)


# ---- SysRem: SYSREM_ROW_CHUNK, K = 2 (test_sysrem.test_bit_equal_small at n = 257) ------------------------------------------------
def _sysrem(name, n_rows, with_dy):
    import sysrem_spec as spec
    import test_sysrem as m
    n = 257

    @functools.lru_cache(maxsize=None)
    def inputs():
        rng = numpy.random.default_rng(1000 * n + n_rows)
        y = m._rows(n_rows, n, rng)
        dy = m._errors(y, rng)
        return y, dy if with_dy else None

    def run(ctx):
        y, dy = inputs()
        flat, trend, (c, a, iters) = ctx.sysrem(y, 2, dy=dy, max_iter=30, tol=1e-6, return_trend=True, return_components=True)
        return flat, trend, c, a, iters

    def want():
        y, dy = inputs()
        return spec.fit(y, 2, dy=dy, max_iter=30, tol=1e-6)

    def compare(got, w):
        assert spec.trend_ok(w[1]) and got[4].tolist() == w[4].tolist(), name
        for a, b, what in zip(got[:4], w[:4], ("flat", "trend", "c", "a")):
            assert numpy.array_equal(m._bits(a), m._bits(b)), (name, what)

    add(name, "sysrem", "tls_sysrem", "sysrem", run, want, compare, size=lambda: n_rows)


_sysrem("sysrem_31_rows", 31, False)
_sysrem("sysrem_33_rows_dy", 33, True)


# ---- biweight and median filter: the smallest and the largest window of their tests on a row of 256 points ------------------------
def _biweight(name, largest):
    import biweight_spec as spec
    import test_biweight as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        rng = numpy.random.default_rng(256)
        rows = m._rows(256, rng)
        t = m._times(256, "regular", rng)
        return t, rows, (4.0 * (t[-1] - t[0]) + 1.0) if largest else 0.3 * m.CADENCE, 0.5

    def compare(got, w):
        assert numpy.array_equal(m._bits(got[1]), m._bits(w[1])) and numpy.array_equal(m._bits(got[0]), m._bits(w[0])), name

    add(name, "biweight_detrend", "tls_biweight_detrend", "biweight_detrend",
        lambda ctx: ctx.biweight_detrend(*inputs(), return_trend=True), lambda: spec.detrend(*inputs()), compare,
        size=lambda: int(numpy.max(numpy.subtract(*spec.windows(inputs()[0], inputs()[2], 0.5)[::-1]))))


_biweight("biweight_smallest_window", False)
_biweight("biweight_largest_window", True)


def _medfilt(name, largest):
    import test_detrend as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        rows = m._rows(256, numpy.random.default_rng(256))
        ks = [k for k in m.KERNELS if k <= 256]
        return rows, ks[-1] if largest else ks[0]

    def want():
        from scipy.signal import medfilt
        rows, k = inputs()
        trend = numpy.array([medfilt(r, k) for r in rows])
        return rows / trend, trend

    def compare(got, w):
        assert numpy.array_equal(m._bits(got[1]), m._bits(w[1])) and numpy.array_equal(m._bits(got[0]), m._bits(w[0])), name

    add(name, "medfilt_detrend", "tls_medfilt_detrend", "medfilt_detrend",
        lambda ctx: ctx.medfilt_detrend(*inputs(), return_trend=True), want, compare, size=lambda: inputs()[1])


_medfilt("medfilt_smallest_kernel", False)
_medfilt("medfilt_largest_kernel", True)


# ---- ephemeris match: MATCH_TILE ------------------------------------------------------------------------------------------------------
def _match(name, n):
    import ephemeris_match_spec as spec

    def compare(got, w):
        assert got[0].dtype.names == spec.FIELDS
        fields_equal(got[0], w, spec.FIELDS, name)

    add(name, "ephemeris_match", "tls_ephemeris_match", "ephemeris_match",
        lambda ctx: (survey.ephemeris_match(*spec.clustered(n, n), context=ctx),), lambda: spec.match(*spec.clustered(n, n)), compare,
        size=lambda: n)


_match("ephemeris_match_tile_less_one", _lib.MATCH_TILE - 1)
_match("ephemeris_match_tile_and_one", _lib.MATCH_TILE + 1)


# ---- inject and null rows: one small slab each (and the next size of their tests for the pairs) ------------------------------------
def _inject(name, inputs):
    import test_injection_recovery as m
    import test_injection_recovery_host as host
    inputs = functools.lru_cache(maxsize=None)(inputs)
    law, u = m.LAWS[0]

    def run(ctx):
        t, base, inj = inputs()
        return ctx.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(u, law, {})[1:])

    def want():
        t, base, inj = inputs()
        return host.host_rows(t, base, inj, u, law)

    def compare(got, w):
        t, base, inj = inputs()
        m._check_rows(name, t, base, inj, got[0], got[1], u, law)

    add(name, "inject_transits", "tls_inject_transits", "inject_transits", run, want, compare)


def _inject_branches():
    """test_injection_recovery.test_every_branch at p = 0.5."""
    import test_injection_recovery as m
    P, a, T0, p = 4.0, 3.0, 0.25, 0.5
    targets = numpy.array([0.0, p, abs(1.0 - p), 1.0 + p, max(p - 1.0, 0.0)])
    around = numpy.concatenate([targets * (1.0 + d) for d in (-1e-6, -1e-9, 1e-9, 1e-6)] + [numpy.linspace(0, 1 + p + 0.1, 97)])
    t = m._times_at(numpy.unique(numpy.concatenate([targets, numpy.abs(around)])), T0, P, a)
    return t, numpy.ones(len(t)), dict(T0=[T0], period=[P], rp_rs=[p], a=[a], inc=[90.0])


def _inject_gapped():
    """test_injection_recovery.test_device_model_against_host on the gapped series."""
    import test_injection_recovery_host as host
    t = numpy.linspace(3.0, 60.0, 2736)
    t = t[((t < 14.0) | (t > 21.5)) & ((t < 40.0) | (t > 41.2))]
    rng = numpy.random.RandomState(len(t))
    base = 1.0 + rng.normal(0.0, 1e-4, len(t))
    return t, base, host.random_injections(rng, t, 67)


_inject("inject_transits_branches", _inject_branches)
_inject("inject_transits_gapped_67", _inject_gapped)


def _null_white(name, n, sigma, first_trial, n_rows):
    import test_null_calibration_host as host

    def compare(got, w):
        numpy.testing.assert_allclose(got[0], w, rtol=0, atol=2.0 ** -51, err_msg=name)

    add(name, "null_rows_white", "tls_null_rows", "null_rows", lambda ctx: (ctx.null_rows(n, n_rows, 1, first_trial, sigma=sigma),),
        lambda: host.white_rows(n, n_rows, 1, first_trial, sigma), compare)


_null_white("null_rows_white_33", 33, 0.01, 2, 3)
_null_white("null_rows_white_4321", 4321, numpy.array([0.1, 0.05, 0.025, 0.0125]), 12345, 4)


def _null_bootstrap(name, n, block):
    import test_null_calibration_host as host

    @functools.lru_cache(maxsize=None)
    def source():
        rng = numpy.random.RandomState(5)
        small = 1.0 + 1e-3 * rng.standard_normal((3, 50))
        return small if n == 50 else 1.0 + 1e-3 * rng.standard_normal((3, n))

    def compare(got, w):
        assert numpy.array_equal(got[0].view(numpy.uint64), w.view(numpy.uint64)), name

    add(name, "null_rows_bootstrap", "tls_null_rows", "null_rows",
        lambda ctx: (ctx.null_rows(n, 4, 1, 12345, source=source(), block=block),),
        lambda: host.bootstrap_rows(n, 4, 1, 12345, source(), block), compare)


_null_bootstrap("null_rows_bootstrap_50", 50, 7)
_null_bootstrap("null_rows_bootstrap_4320", 4320, 48)


# ---- the post-search chain's own entries ---------------------------------------------------------------------------------------------
def _spectra(name, path):
    """test_gpu_parity.test_spectra_kernel_vs_reference_and_oracle on a golden file."""
    golden = functools.lru_cache(maxsize=None)(lambda: dict(numpy.load(path)))

    def run(ctx):
        g = golden()
        SR, praw, power, sde_raw, sde = ctx.spectra(int(g["oversampling_factor"]) * 30, g["chi2"])
        return SR, praw, power, numpy.array([sde_raw, sde])

    def compare(got, g):
        numpy.testing.assert_allclose(got[0], g["SR"], rtol=1e-13, err_msg=name)
        numpy.testing.assert_allclose(got[1], g["power_raw"], rtol=1e-10, atol=1e-11, err_msg=name)
        numpy.testing.assert_allclose(got[2], g["power"], rtol=1e-10, atol=1e-11, err_msg=name)
        numpy.testing.assert_allclose(got[3], [float(g["SDE_raw"]), float(g["SDE"])], rtol=1e-11)
        assert int(numpy.argmax(got[2])) == int(numpy.argmax(g["power"]))

    add(name, "spectra", "tls_spectra", "spectra", run, golden, compare, size=lambda: len(golden()["chi2"]))


_SPECTRA = sorted(glob.glob(os.path.join(GOLDEN, "spectra_*.npz")), key=lambda p: len(numpy.load(p)["chi2"]))
_spectra("spectra_shortest_golden", _SPECTRA[0])
_spectra("spectra_longest_golden", _SPECTRA[-1])


def _pink(name, n, width):
    """test_gpu_power's pink-noise sizes: the data are drawn in its order from its seed."""
    @functools.lru_cache(maxsize=None)
    def data():
        rng = numpy.random.RandomState(5)
        rows = {size: 1 + rng.normal(0, 3e-4, size) for size in (40, 700)}
        return rows[n]

    def compare(got, w):
        assert float(got[0]) == w, name

    add(name, "pink_noise", "tls_pink_noise", "pink_noise", lambda ctx: (numpy.array(ctx.pink_noise(data(), width)),),
        lambda: stats.pink_noise(data(), width), compare, size=lambda: n)


_pink("pink_noise_40_by_3", 40, 3)
_pink("pink_noise_700_by_128", 700, 128)


def _t0_fit(name, path):
    """test_gpu_parity.test_t0_fit_kernel_vs_oracle_and_reference_residuals on a golden file."""
    golden = functools.lru_cache(maxsize=None)(lambda: dict(numpy.load(path)))

    def run(ctx):
        g = golden()
        return (ctx.t0_fit_residuals(g["t"], g["y"], float(g["period"]), g["scaled_signal"], g["T0_array"], int(len(g["signal"]) / 2) + 1),)

    def compare(got, g):
        numpy.testing.assert_allclose(got[0], g["residuals"], rtol=1e-12, atol=0, err_msg=name)
        assert g["T0_array"][int(numpy.argmin(got[0]))] == float(g["T0"]), name

    add(name, "t0_fit", "tls_t0_fit", "t0_fit_residuals", run, golden, compare, size=lambda: len(golden()["T0_array"]))


_T0FIT = sorted(glob.glob(os.path.join(GOLDEN, "t0fit_*.npz")), key=lambda p: len(numpy.load(p)["T0_array"]))
_t0_fit("t0_fit_fewest_epochs_golden", _T0FIT[0])
_t0_fit("t0_fit_most_epochs_golden", _T0FIT[-1])


def _peak_fits(name, n):
    """test_peak_fits.test_t0_fit_shapes on the tiny plan: 15 points (the general kernel: below the rotation path's 16) and 17
    (the rotation path)."""
    import peak_fits_spec as spec
    import test_peak_fits as m

    @functools.lru_cache(maxsize=None)
    def inputs():
        rng = numpy.random.RandomState(n)
        inp = m.tiny_plan(n)
        y = 1 + rng.normal(0, 1e-3, (2, n))
        rec, power = m.records(inp, rng, 2, 2)
        return inp, y, rec, power, numpy.array([2, 2])

    def run(ctx):
        inp, y, rec, power, n_peaks = inputs()
        ctx.prepare(inp["t"], y[0], numpy.full(n, numpy.std(y[0])), inp["periods"], inp["table"], inp["params"])
        return m.debug_fits(ctx, inp, y, rec, n_peaks, power, with_fits=True)

    def want(ref):
        inp, y, rec, power, n_peaks = inputs()
        return [[quiet(spec.expected, ref, inp, y[c], rec[c, r], r, int(n_peaks[c]), power[c]) for r in range(2)] for c in range(2)]

    def compare(got, w):
        for c in range(2):
            for r in range(2):
                assert w[c][r]["status"] == spec.FITTED
                for k, v in w[c][r].items():
                    m.expect_equal(got[0][k][c, r], v, (name, c, r, k))

    add(name, "peak_fits", "tls_debug_peak_fits", "debug_peak_fits", run, want, compare, size=lambda: n, want_on_device=True)


_peak_fits("peak_fits_general_kernel_15", 15)
_peak_fits("peak_fits_rotation_path_17", 17)


@functools.lru_cache(maxsize=None)
def _stats_inputs():
    """test_power_batch_statistics.test_injected_picks_reach_every_branch: its series, its four picks and their powers."""
    import test_power_batch_statistics as m
    t = m.gapped_time()
    _, f = synthetic.light_curve(30.0, 24, 2e-4, per=4.321, rp=0.05, a=12)
    f = numpy.interp(t, numpy.linspace(3.0, 33.0, len(f)), f)
    inp = quiet(synthetic.search_inputs, t, f, period_min=1.5, period_max=9.0, oversampling_factor=2)
    n_p = len(inp["periods"])
    rng = numpy.random.RandomState(3)
    smooth = numpy.exp(-0.5 * ((numpy.arange(n_p) - n_p / 2) / 40.0) ** 2) + rng.uniform(0, 0.05, n_p)
    first_peak = smooth[::-1].copy()
    first_peak[0] = 10.0
    first_peak[-1] = 6.0
    last_peak = smooth.copy()
    last_peak[-1] = 10.0
    picks = [(4.321, 3.0 + 1.1, 3, smooth), (4.321, 3.0 - 1.3, 3, first_peak), (20.0, 19.5, 3, last_peak), (25.0, 16.0, 0, numpy.ones(n_p))]
    return inp, picks


def _transit_stats():
    import test_power_batch_statistics as m

    def run(ctx):
        inp, picks = _stats_inputs()
        t, y = inp["t"], inp["y"]
        ctx.prepare(t, y, inp["dy"], inp["periods"], inp["table"], inp["params"])
        root = numpy.array([float(k) ** 0.5 for k in range(len(t) + 1)])
        root_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(len(t) + 1)])
        powers = numpy.array([p[3] for p in picks])
        return ctx.debug_transit_stats(numpy.repeat(y[None, :], len(picks), axis=0), [p[0] for p in picks], [p[1] for p in picks],
                                       [p[2] for p in picks], 0.999, 0, [int(numpy.argmax(p)) for p in powers], powers,
                                       inp["table"].duration, calculate_fill_factor(t), root, 4000, root_count=root_count)

    def want():
        inp, picks = _stats_inputs()
        dur = inp["table"].duration
        return [m.host_stats(inp["t"], inp["y"], period, T0, dur[row], inp["periods"], power)[:2] for period, T0, row, power in picks]

    def compare(got, w):
        stats_, rows, n_ep = got
        for c, (rec, want_rows) in enumerate(w):
            for k, v in rec.items():
                m.expect_equal(stats_[k][c], v, "pick %d: %s" % (c, k))
            e = int(n_ep[c])
            assert e == rec["transit_count"]
            for i, v in enumerate(want_rows):
                m.expect_equal(rows[c, i, :e], v, "pick %d: %s" % (c, m.PER_TRANSIT[i]))
                assert numpy.all(numpy.isnan(rows[c, i, e:]))

    add("transit_stats_injected_picks", "transit_stats", "tls_debug_transit_stats", "debug_transit_stats", run, want, compare)


_transit_stats()


@functools.lru_cache(maxsize=None)
def _models_inputs():
    """test_power_batch_results.test_model_stage_edges_equal_the_host_sequence: its plan and its seven picks."""
    from tls_amd.stats import all_transit_times, calculate_stretch
    t, f = synthetic.light_curve(30.0, 24, 2e-4, per=4.321, rp=0.05, a=12)
    inp = quiet(synthetic.search_inputs, t, f, period_min=3.5, period_max=5.5, oversampling_factor=2)
    t, n = inp["t"], len(inp["t"])
    span, t0 = float(t[-1] - t[0]), float(t[0])
    maxw = int(numpy.max(inp["durations"]) * n)
    fill_half = 1 - ((1 - calculate_fill_factor(t)) * 0.5)
    P = 4.3
    stretch = calculate_stretch(t, P, [0.0] * len(all_transit_times(t0 + 1.0, t, P)))
    cases = []
    for occ in (0, 1):
        d = (occ + 0.5) / (fill_half * stretch * n)
        assert int((d * maxw * fill_half / (maxw / stretch)) * n) == occ
        cases.append((P, t0 + 1.0, d))
    cases += [(P, t0 + 1.0, 0.04), (span, t0 + 0.5, 0.03), (P, t0 - 1.3, 0.04), (P, t0 + span + 3 * P, 0.04), (0.11, t0 + 0.02, 0.01)]
    return inp, cases


def _transit_models():
    import test_power_batch_results as m
    depth = 0.9993

    def run(ctx):
        inp, cases = _models_inputs()
        ctx.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
        y = numpy.stack([inp["y"]] * len(cases))
        return quiet(m.run_injected, ctx, inp, y, numpy.array([c[0] for c in cases]), numpy.array([c[1] for c in cases]),
                     [c[2] for c in cases], depth)

    def want():
        inp, cases = _models_inputs()
        return [quiet(m.host_models, inp, inp["y"], inp["dy"], P, T, d, depth) for P, T, d in cases]

    def compare(got, w):
        stats_, rows, n_epochs, folded, model, lc, lc_len = got
        for c, (ph, fy, fdy, order, fm, lt, lm) in enumerate(w):
            numpy.testing.assert_array_equal(folded[c, 0], ph, str(c))
            numpy.testing.assert_array_equal(folded[c, 1], fy, str(c))
            numpy.testing.assert_array_equal(folded[c, 2], order, str(c))
            numpy.testing.assert_array_equal(model[c], fm, str(c))
            assert lc_len[c] == len(lt), c
            numpy.testing.assert_array_equal(lc[c, 0, :lc_len[c]], lt, str(c))
            numpy.testing.assert_array_equal(lc[c, 1, :lc_len[c]], lm, str(c))
            assert numpy.all(numpy.isnan(lc[c, :, lc_len[c]:])), c

    add("transit_models_injected_picks", "transit_models", "tls_debug_transit_models", "debug_transit_models", run, want, compare)


_transit_models()


@functools.lru_cache(maxsize=None)
def _chain_inputs():
    """test_power_batch_statistics.test_the_two_root_tables_are_checked: the gapped series, one row of noise, its plan."""
    import test_power_batch_statistics as m
    t = m.gapped_time()
    n = len(t)
    rng = numpy.random.RandomState(23)
    inp = quiet(synthetic.search_inputs, t, 1 + rng.normal(0, 4e-4, n), period_min=1.5, period_max=9.0, oversampling_factor=1)
    root = numpy.array([float(k) ** 0.5 for k in range(n + 1)])
    root_count = numpy.array([float(numpy.sum(k) ** 0.5) for k in range(n + 1)])
    chain = (inp["t"], numpy.ascontiguousarray(inp["y"][None, :]), inp["dy"][None, :], inp["periods"], inp["table"], inp["params"], 30)
    return inp, chain, calculate_fill_factor(t), root, root_count


def _power_batch_entries():
    def plain(ctx):
        inp, chain, fill, root, root_count = _chain_inputs()
        return ctx.power_batch(*chain, with_arrays=True, with_power=True, with_spectra=True)

    def with_stats(ctx):
        inp, chain, fill, root, root_count = _chain_inputs()
        return ctx.power_batch_stats(*chain, fill, root, 32, per_transit=True, with_arrays=True, with_spectra=True,
                                     root_count=root_count)

    def with_models(ctx):
        inp, chain, fill, root, root_count = _chain_inputs()
        lc_cap = 15 * len(inp["t"]) + 10
        return ctx.power_batch_stats(*chain, fill, root, 32, per_transit=True, models=survey._model_template(inp), lc_cap=lc_cap,
                                     root_count=root_count)

    add("power_batch_one_row", "power_batch", "tls_power_batch", "power_batch", plain)
    add("power_batch_stats_one_row", "power_batch_stats", "tls_power_batch_stats", "power_batch_stats", with_stats)
    add("power_batch_models_one_row", "power_batch_models", "tls_power_batch_models", "power_batch_stats", with_models)


_power_batch_entries()


def _peaks_pipeline():
    """test_peaks.test_one_context_across_two_grid_sizes' first batch: power_batch(peaks=4) on five rows, one of them flat; the
    peaks are the selection's statement on the device's own power, as test_peaks.check_pipeline holds them."""
    import peaks_spec
    import test_peaks as m

    @functools.lru_cache(maxsize=None)
    def flux():
        return m.curves(m.T960, 5, seed=1, flat=(4,))

    def run(ctx):
        summary, periods, chi2, row, depth, power, pk = quiet(survey.power_batch, m.T960, flux(), context=ctx, with_arrays=True,
                                                              peaks=4, period_max=6.0)
        return summary, periods, chi2, row, depth, power, pk["peaks"], pk["n_peaks"]

    def compare(got, w):
        summary, periods, chi2, row, depth, power, peaks, n_peaks = got
        for c in range(len(flux())):
            if summary["no_fit"][c]:
                assert n_peaks[c] == 0
                rec, k = peaks_spec.expected(power[c], periods, 4, min_power=numpy.inf)
            else:
                rec, k = peaks_spec.expected(power[c], periods, 4, 0.02, peaks_spec.HARMONICS, None, chi2[c], row[c], depth[c])
                assert k >= 1 and peaks[c]["index"][0] == summary["index_power"][c]
            assert n_peaks[c] == k, c
            for field in rec.dtype.names:
                assert m.same_bits(peaks[c][field], rec[field]), (c, field)

    add("power_batch_peaks_five_rows", "power_batch_peaks", "tls_power_batch_peaks", "power_batch", run, None, compare)


_peaks_pipeline()


# ---- the pairs: (stage, the constant, the case at or below it, the case above it, how a case's size is held against it) -----------
def _count(size, constant):
    return size <= constant, size > constant


def _epochs_in_chunk(size, constant):
    """size = (the candidate's epochs, the epochs of a chunk at its reach): one chunk, or several."""
    return size[0] <= size[1], size[0] > size[1]


def _rows_of(size, constant):
    return size["rows"] <= constant, size["rows"] > constant


PAIRS = (
    ("prewhiten", _lib.PREWHITEN_LDS_POINTS, "prewhiten_lds_side", "prewhiten_global_side", _count),
    ("shape_fit", _lib.SHAPE_LDS_MEMBERS, "shape_fit_members_in_lds", "shape_fit_members_beyond_lds", _count),
    ("centroid_test", _lib.CENTROID_LDS_EPOCHS, "centroid_epochs_in_lds", "centroid_epochs_beyond_lds", _count),
    ("phase_scan", _lib.PHASE_SCAN_CHUNK, "phase_scan_one_chunk", "phase_scan_two_chunks", _count),
    ("single_transits", _lib.SINGLE_TILE, "single_transits_one_tile", "single_transits_tile_and_one", _count),
    ("transit_times", None, "transit_times_one_chunk", "transit_times_four_chunks", _epochs_in_chunk),
    ("event_vetting", None, "event_vetting_one_chunk", "event_vetting_two_chunks", _epochs_in_chunk),
    ("find_peaks", _lib.PEAKS_LDS_PERIODS, "find_peaks_mask_in_lds", "find_peaks_mask_in_device_memory", _count),
    ("lomb_scargle", _lib.GLS_SMALL_ROWS, "lomb_scargle_3_rows", "lomb_scargle_40_rows_dy", _rows_of),
    ("lomb_scargle", _lib.GLS_SMALL_ROWS, "lomb_scargle_3_rows_dy", "lomb_scargle_40_rows", _rows_of),
    ("nudft", _lib.GLS_SMALL_ROWS, "nudft_31_rows", "nudft_33_rows", _rows_of),
    ("sysrem", _lib.SYSREM_ROW_CHUNK, "sysrem_31_rows", "sysrem_33_rows_dy", _count),
    ("ephemeris_match", _lib.MATCH_TILE, "ephemeris_match_tile_less_one", "ephemeris_match_tile_and_one", _count),
)

# ---- the smaller call behind the larger one, stage by stage: (the larger case, the smaller case) ------------------------------------
BEHIND = collections.OrderedDict((
    ("prewhiten", ("prewhiten_global_side", "prewhiten_n256_c3_dy_h2")),
    ("prewhiten_lds", ("prewhiten_lds_side", "prewhiten_n256_c3_dy_h2")),
    ("shape_fit", ("shape_fit_members_beyond_lds", "shape_fit_members_in_lds")),
    ("centroid_test", ("centroid_epochs_beyond_lds", "centroid_epochs_in_lds")),
    ("phase_scan", ("phase_scan_two_chunks", "phase_scan_one_chunk")),
    ("phase_scan_bins", ("phase_scan_one_chunk", "phase_scan_16_bins")),
    ("single_transits", ("single_transits_tile_and_one", "single_transits_one_tile")),
    ("transit_times", ("transit_times_four_chunks", "transit_times_one_chunk")),
    ("event_vetting", ("event_vetting_two_chunks", "event_vetting_one_chunk")),
    ("find_peaks", ("find_peaks_mask_in_device_memory", "find_peaks_mask_in_lds")),
    ("lomb_scargle", ("lomb_scargle_40_rows_dy", "lomb_scargle_3_rows")),
    ("nudft", ("nudft_33_rows", "nudft_31_rows")),
    ("sine_test", ("sine_test_mask_and_dy", "sine_test_no_mask_no_dy")),
    ("sysrem", ("sysrem_33_rows_dy", "sysrem_31_rows")),
    ("biweight_detrend", ("biweight_largest_window", "biweight_smallest_window")),
    ("medfilt_detrend", ("medfilt_largest_kernel", "medfilt_smallest_kernel")),
    ("ephemeris_match", ("ephemeris_match_tile_and_one", "ephemeris_match_tile_less_one")),
    ("inject_transits", ("inject_transits_gapped_67", "inject_transits_branches")),
    ("null_rows_white", ("null_rows_white_4321", "null_rows_white_33")),
    ("null_rows_bootstrap", ("null_rows_bootstrap_4320", "null_rows_bootstrap_50")),
    ("spectra", ("spectra_longest_golden", "spectra_shortest_golden")),
    ("pink_noise", ("pink_noise_700_by_128", "pink_noise_40_by_3")),
    ("t0_fit", ("t0_fit_most_epochs_golden", "t0_fit_fewest_epochs_golden")),
    ("peak_fits", ("peak_fits_rotation_path_17", "peak_fits_general_kernel_15")),
    ("power_batch", ("power_batch_peaks_five_rows", "power_batch_one_row")),
    ("power_batch_stats", ("power_batch_models_one_row", "power_batch_stats_one_row")),
    ("transit_stats", ("transit_models_injected_picks", "transit_stats_injected_picks")),
))
