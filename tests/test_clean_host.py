"""The cleaning stage without a GPU: the statement (tests/clean_spec.py) in its two forms and its identities, what it does on
the project's usual curve with flares, missing points and single low samples (the figures DESIGN.md "Cleaning" quotes), the
argument checks, the Clean step of the survey calls, and align_rows."""
import math
import os
import re

import numpy
import pytest

import clean_cases as cases
import clean_spec as spec
from tls_amd import _lib, helpers, survey, synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


# ---- the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.PLAIN)
def test_plain_python_equals_numpy(name):
    t, y, bad, kw = cases.CASES[name]
    plain = spec.clean(t, y, bad, plain=True, **kw)
    for a, b in zip(plain, cases.expected(name)):
        assert cases.same(a, b), name


def test_the_cases_reach_what_they_are_for():
    """Every case's record says that its path was taken."""
    rec = lambda name: cases.expected(name)[2]   # noqa: E731
    flags = lambda name: cases.expected(name)[1]   # noqa: E731
    assert rec("window_of_one")["rounds"].tolist() == [0.0, 0.0] and numpy.isnan(rec("window_of_one")["sigma"]).all()
    assert rec("segment_missing")["status"].tolist() == [1.0, 0.0] and rec("segment_missing")["longest_run"][0] == 20.0
    assert rec("row_missing")["status"].tolist() == [2.0, 0.0] and numpy.all(cases.expected("row_missing")[0][0] == 1.0)
    assert rec("constant")["sigma"].tolist() == [0.0] and rec("constant")["rounds"].tolist() == [1.0] and not flags("constant").any()
    assert rec("constant_slide")["sigma"].tolist() == [0.0] and flags("constant_slide").sum() == 1
    few, all_ = cases.expected("few_members"), spec.clean(*cases.CASES["few_members"][:3], **dict(cases.CASES["few_members"][3], min_points=3))
    assert numpy.all(few[1][:, 2] == 0) and numpy.all(all_[1][:, 2] == 4)      # (short of 20 members: no residual, never flagged)
    for it in (0, 1, 16):
        r = rec("one_a_round_%d" % it)
        assert r["rounds"][0] == r["n_high"][0] == r["n_filled"][0] == it, it
    assert numpy.flatnonzero(flags("one_a_round_16")[0]).tolist() == list(range(24, 40))
    # the guard: two of three valid points would go; the round is not applied, but it is counted and leaves its sigma
    g = cases.expected("guard")
    assert not g[1].any() and g[2]["rounds"].tolist() == [1.0, 1.0] and numpy.all(g[2]["sigma"] > 0)
    assert cases.same(g[0], cases.CASES["guard"][1])
    gb = cases.expected("guard_after_bad")
    assert gb[1].tolist() == [[0, 0, 0, 2, 1]] and gb[2]["rounds"][0] == 1.0
    # runs: [row 0] 58, 59 | 60 across a boundary; [row 1] 30, (31 missing), 32 and 90 alone; [row 2] 20..23, high 24, 25, 26
    low = lambda run: [numpy.flatnonzero(f & 8).tolist() for f in flags("runs_max%d" % run)]   # noqa: E731
    assert low(1) == [[60], [90], []]
    assert low(2) == [[58, 59, 60], [30, 32, 90], [25, 26]]
    assert low(3) == low(2)
    assert numpy.flatnonzero(flags("runs_max1")[2] & 4).tolist() == [24]
    for run in (1, 2, 3):
        assert cases.same(flags("runs_slide_max%d" % run), flags("runs_max%d" % run))
    # duplicated stamps: between two valid points of one stamp the left one's value; else the interpolation of the header
    t, y, _, _ = cases.CASES["duplicate_stamps"]
    out = cases.expected("duplicate_stamps")[0]
    assert out[0, 11] == y[0, 10] + (y[0, 12] - y[0, 10]) * ((t[11] - t[10]) / (t[12] - t[10])) and out[0, 39] == y[0, 38]
    assert out[0, 4] == y[0, 3] + (y[0, 6] - y[0, 3]) * ((t[4] - t[3]) / (t[6] - t[3])) and out[1, 0] == y[1, 3]
    same_stamp = spec.clean([1.0, 1.0, 1.0, 2.0], [1.5, numpy.nan, 2.5, 3.0], sigma_upper=INF)[0]
    assert same_stamp.tolist() == [1.5, 1.5, 2.5, 3.0]          # t_b == t_a: y_a


def test_identities():
    t = cases.series(300, gap_at=200)
    y = cases.dirty_rows(300, 3, seed=31)
    rows, flags, record = spec.clean(t, y, sigma_upper=INF, sigma_lower=INF)
    for k in range(3):
        kept_t, kept_y = helpers.cleaned_array(t + 1.0, y[k])      # (t + 1: cleaned_array drops t <= 0 as well)
        assert numpy.array_equal(kept_t, (t + 1.0)[flags[k] == 0]) and cases.same(kept_y, y[k][flags[k] == 0])
        assert set(numpy.unique(flags[k]).tolist()) == {0, 1}
        assert cases.same(rows[k][flags[k] == 0], y[k][flags[k] == 0])
    assert record["rounds"].tolist() == [0.0] * 3 and numpy.array_equal(record["n_missing"], (flags == 1).sum(axis=1))
    # a finite row with nothing flagged comes back bit for bit
    quiet = 1.0 + 1e-3 * numpy.sin(numpy.arange(300.0))[None, :] * numpy.array([[1.0], [1e-300], [1e300]])
    quiet[1:] = numpy.abs(quiet[1:]) + 1e-310
    for kw in (dict(), dict(window_length=0.5, sigma_lower=4.0), dict(n_iter=0), dict(sigma_upper=INF, sigma_lower=INF)):
        rows, flags, record = spec.clean(t, quiet[:1], **kw)
        assert cases.same(rows, quiet[:1]) and not flags.any() and record["n_filled"][0] == 0 and record["status"][0] == 0
    # bad of zeros gives the bits of no bad
    for name in ("bad", "bad_slide"):
        t, y, bad, kw = cases.CASES[name]
        for a, b in zip(spec.clean(t, y, numpy.zeros(y.shape, dtype=bad.dtype), **kw), spec.clean(t, y, None, **kw)):
            assert cases.same(a, b)
        assert numpy.array_equal((cases.expected(name)[1] & 2) != 0, bad != 0)


# ---- measured on the statement, seeds 0 to 4 --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_flat_rows(seed):
    c = cases.survey_curve(seed)
    rows, flags, record = spec.clean(c["t"], c["y"], window_length=None, sigma_upper=4.0, sigma_lower=5.0, max_run=1, n_iter=5)
    clipped = (flags & 12) != 0
    print("seed %d: sigma / noise %.3f, rounds %d, %d of %d flare samples, %d low, %d in transit"
          % (seed, record["sigma"] / cases.NOISE, record["rounds"], (clipped & c["flare"]).sum(), c["flare"].sum(),
             record["n_low"], (clipped & c["in_transit"]).sum()))
    assert numpy.array_equal((flags & 1) != 0, c["nan"])
    assert numpy.all((flags[c["low"]] & 8) != 0)
    assert not (((flags & 4) != 0) & ~c["flare"]).any()
    assert abs(record["sigma"] / cases.NOISE - 1.0) <= 0.10
    assert record["rounds"] <= 3
    assert not (clipped & c["in_transit"]).any()
    assert numpy.all(numpy.isfinite(rows) & (rows > 0.0)) and cases.same(rows[flags == 0], c["y"][flags == 0])


@pytest.mark.parametrize("seed", range(5))
def test_raw_rows_of_the_rotator(seed):
    """A sliding clip on an undetrended fast rotator eats the shoulders of its transits: the counts DESIGN.md quotes."""
    c = cases.survey_curve(seed, rotator=True)
    tr = c["in_transit"]
    shoulder = (numpy.convolve(tr.astype(float), numpy.ones(25), mode="same") > 0) & ~tr      # within 0.25 d of a transit
    for window in (0.3, 0.5):
        rows, flags, record = spec.clean(c["t"], c["y"], window_length=window, sigma_upper=4.0)
        clipped = (flags & 12) != 0
        print("seed %d, %.1f d: sigma / noise %.3f, %d of %d flare samples, %d in transit, %d on the shoulders, %d elsewhere"
              % (seed, window, record["sigma"] / cases.NOISE, (clipped & c["flare"]).sum(), c["flare"].sum(), (clipped & tr).sum(),
                 (clipped & shoulder & ~c["flare"]).sum(), (clipped & ~shoulder & ~tr & ~c["flare"]).sum()))
        if window == 0.3:
            assert (clipped & c["flare"]).sum() >= 37
            assert not (clipped & tr).any()


def _sde(oracle_lib, t, y):
    """(period, SDE_raw) of the oracle's search of one row: SR = min(chi2) / chi2, SDE = (max - mean) / std of SR."""
    inp = synthetic.search_inputs(t, y, period_min=5.0, period_max=10.0, oversampling_factor=2)
    p = inp["params"]
    chi2 = oracle_lib.search(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], p["transit_depth_min"], p["R_star_min"],
                             p["R_star_max"], p["M_star_min"], p["M_star_max"], p["T0_fit_margin"])[0]
    sr = chi2.min() / chi2
    return float(inp["periods"][int(numpy.argmax(sr))]), float((sr.max() - sr.mean()) / sr.std())


def test_end_to_end_on_the_cpu(oracle_lib):
    """The period found on the repaired row against the one found with the flagged points deleted (the oracle's search)."""
    c = cases.survey_curve(0)
    rows, flags, record = spec.clean(c["t"], c["y"], window_length=None, sigma_upper=4.0, sigma_lower=5.0, max_run=1, n_iter=5)
    keep = flags == 0
    repaired = _sde(oracle_lib, c["t"], rows)
    deleted = _sde(oracle_lib, c["t"][keep], c["y"][keep])
    print("repaired: period %.4f, SDE %.2f; flagged points deleted: period %.4f, SDE %.2f; ratio %.3f"
          % (repaired + deleted + (repaired[1] / deleted[1],)))
    assert abs(repaired[0] / 7.0 - 1.0) < 0.01 and abs(deleted[0] / 7.0 - 1.0) < 0.01
    assert abs(repaired[0] / deleted[0] - 1.0) < 0.005


# ---- the interface and the source -------------------------------------------------------------------------------------------
def test_the_fields_and_the_constants():
    assert survey.clean_fields() == _lib.CLEAN_FIELDS == spec.FIELDS
    assert _lib.CLEAN_DTYPE == spec.RECORD_DTYPE and _lib.CLEAN_DTYPE.itemsize == 80
    assert (_lib.CLEAN_MAX_ITER, _lib.CLEAN_LDS_POINTS) == (spec.MAX_ITER, _lib.NOISE_LDS_POINTS) == (16, 8192)
    header = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    for line in ("#define TLS_CLEAN_MAX_ITER 16", "#define TLS_CLEAN_LDS_POINTS 8192", "#define TLS_AMD_ABI_VERSION 8",
                 "int tls_clean_rows(tls_ctx *ctx, const double *t, const double *y, const uint8_t *bad, int64_t n, int64_t n_rows,"):
        assert line in header, line
    assert "tls_clean_rows" in _lib.SYMBOLS


def test_where_the_method_and_the_buffer_stand():
    import ast
    tree = ast.parse(open(os.path.join(REPO, "tls_amd", "_lib.py")).read())
    context = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Context")
    names = [n.name for n in context.body if isinstance(n, ast.FunctionDef)]
    assert names.index("clean_rows") > names.index("spline_detrend") > names.index("ephemeris_match")
    source = open(os.path.join(REPO, "tls_amd", "csrc", "tls_amd.hip")).read()
    assert re.search(r'DevBuf<double> d_clean\{pool, "d_clean", kScratch\};', source)
    body = source[source.index("int tls_clean_rows(tls_ctx* ctx"):source.index("// ---- spline detrending (tls_spline.hip.h")]
    assert body.count("L.bind(") == 1 and "L.bind(ctx->d_clean)" in body and "hipMalloc" not in body
    assert '#include "tls_clean.hip.h"' in open(os.path.join(REPO, "tls_amd", "csrc", "tls_kernels.hip.h")).read()
    kernels = open(os.path.join(REPO, "tls_amd", "csrc", "tls_clean.hip.h")).read()
    assert kernels.count("#pragma clang fp contract(off)") == 3 and "__syncthreads" not in kernels and "atomicAdd(&a.counts" in kernels
    assert "detrend_stage_sort(" in kernels and "noise_median(" in kernels            # shared, not copied
    assert "bitonic" not in kernels and "hist[" not in kernels


_N = 12
_T = numpy.arange(_N) / 48.0
_Y = numpy.linspace(1.0, 1.1, 2 * _N).reshape(2, _N)

REFUSALS = [
    ("t_descending", dict(t=_T[::-1]), "cleaning: t must be finite and non-decreasing"),
    ("t_shape", dict(t=_T[None, :]), "cleaning: t must have shape \\[n\\] with n in \\[1, 1e8\\]"),
    ("flux_shape", dict(flux_batch=numpy.ones((2, _N + 1))), "cleaning: flux must be \\[n\\] or \\[n_curves, n\\] over the time stamps t \\[n\\]"),
    ("flux_text", dict(flux_batch=[["a"] * _N]), "cleaning: the light curves must hold numbers"),
    ("window_zero", dict(window_length=0.0), "cleaning: window_length must be None or finite and > 0, got 0.0"),
    ("window_inf", dict(window_length=INF), "cleaning: window_length must be None or finite and > 0"),
    ("window_bool", dict(window_length=True), "cleaning: window_length must be None or finite and > 0"),
    ("break_zero", dict(break_tolerance=0.0), "cleaning: break_tolerance must be a number > 0, got 0.0"),
    ("break_nan", dict(break_tolerance=math.nan), "cleaning: break_tolerance must be a number > 0"),
    ("sigma_upper_zero", dict(sigma_upper=0.0), "cleaning: sigma_upper must be a number > 0, got 0.0"),
    ("sigma_lower_nan", dict(sigma_lower=math.nan), "cleaning: sigma_lower must be a number > 0, got nan"),
    ("max_run_zero", dict(max_run=0), "cleaning: max_run must be an integer"),
    ("max_run_float", dict(max_run=1.5), "cleaning: max_run must be an integer"),
    ("n_iter_high", dict(n_iter=17), "cleaning: n_iter must be an integer in \\[0, 16\\], got 17"),
    ("n_iter_negative", dict(n_iter=-1), "cleaning: n_iter must be an integer in \\[0, 16\\], got -1"),
    ("min_points_zero", dict(min_points=0), "cleaning: min_points must be an integer"),
    ("bad_dtype", dict(bad=numpy.zeros((2, _N))), "bad must be a uint8 or bool array, got dtype float64"),
    ("bad_shape", dict(bad=numpy.zeros((2, _N - 1), dtype=bool)), "bad must have shape \\(2, 12\\)"),
]


@pytest.mark.parametrize("name,kwargs,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, kwargs, message):
    kwargs = dict(kwargs)
    t, flux = kwargs.pop("t", _T), kwargs.pop("flux_batch", _Y)
    with pytest.raises(ValueError, match=message):
        survey.clean_batch(t, flux, **kwargs)
    with pytest.raises(ValueError, match=message):
        _lib.clean_arguments(t, flux, **kwargs)


def test_what_the_checks_accept():
    y = _Y.copy()
    y[0, :4] = [numpy.nan, INF, -1.0, 0.0]
    a = _lib.clean_arguments(_T, y[0], None, INF, INF, INF, 2 ** 40, 0, 1)
    assert a["single"] and a["y"].shape == (1, _N) and a["window_length"] is None and a["bad"] is None and a["max_run"] == 2 ** 40
    a = _lib.clean_arguments(_T, y, 0.25, bad=numpy.zeros((2, _N), dtype=bool))
    assert not a["single"] and a["bad"].dtype == numpy.uint8 and a["window_length"] == 0.25
    t = numpy.arange(5000) / 48.0
    with pytest.raises(ValueError, match="cleaning: a window holds 5000 points, more than BIWEIGHT_MAX_WINDOW = 4095"):
        _lib.clean_arguments(t, numpy.ones(5000), 1000.0)


class _Recorder(object):
    """A context that records what a survey call hands its stage methods."""

    def __init__(self):
        self.calls = []

    def clean_rows(self, t, y, *args, **kw):
        self.calls.append(("clean_rows", args, kw))
        rows = numpy.where(numpy.isfinite(y) & (numpy.asarray(y) > 0), y, 1.0)
        if kw.get("return_record"):
            return rows, numpy.zeros(numpy.shape(y), dtype=numpy.uint8), numpy.zeros(len(y), dtype=_lib.CLEAN_DTYPE)
        return rows

    def biweight_detrend(self, t, y, window_length, break_tolerance, return_trend=False):
        assert numpy.all(numpy.isfinite(y))
        self.calls.append(("biweight_detrend", (window_length, break_tolerance), {}))
        return numpy.asarray(y) * 1.0

    def biweight_detrend_masked(self, t, y, mask, *args, **kw):
        self.calls.append(("biweight_detrend_masked", (mask,) + args, kw))
        return numpy.asarray(y) * 1.0, numpy.ones_like(y), numpy.zeros(numpy.shape(y), dtype=numpy.uint8)

    def medfilt_detrend(self, y, k, return_trend=False):
        self.calls.append(("medfilt_detrend", (k,), {}))
        return numpy.asarray(y) * 1.0


def test_the_step_on_the_survey_calls():
    step = survey.Clean()
    assert step == (None, 4.0, INF, 1, 3, 3, 0.5)
    assert step._fields == ("window_length", "sigma_upper", "sigma_lower", "max_run", "n_iter", "min_points", "break_tolerance")
    assert survey.Clean(None, 4.0).sigma_upper == 4.0 and survey.Clean(sigma_upper=INF).window_length is None
    assert survey._detrend_steps(step) == (step,) and survey._detrend_steps((step, 5)) == (step, 5)
    with pytest.raises(AttributeError):
        step.n_iter = 2
    y = _Y.copy()
    y[0, 3], y[1, 7] = numpy.nan, -2.0
    # _detrended: clean_batch with the step's fields; the repaired rows go on; a mask goes to the steps behind it only
    ctx = _Recorder()
    mask = numpy.zeros((2, _N), dtype=numpy.uint8)
    mask[1, 3] = 1
    rows = survey._detrended(_T, y, (survey.Clean(0.2, 3.0, 5.0, 2, 4, 6, 0.7), survey.Biweight(0.2)), ctx, None, None, detrend_mask=mask)
    assert rows.shape == y.shape and [c[0] for c in ctx.calls] == ["clean_rows", "biweight_detrend_masked"]
    assert ctx.calls[0][1][:7] == (0.2, 0.7, 3.0, 5.0, 2, 4, 6) and ctx.calls[0][1][7] is None
    assert numpy.array_equal(ctx.calls[1][1][0], mask)
    ctx = _Recorder()
    survey._detrended(_T, y, (step, survey.Biweight(0.2), 3, survey.Clean(None, 4.0)), ctx, None, None)
    assert [c[0] for c in ctx.calls] == ["clean_rows", "biweight_detrend", "medfilt_detrend", "clean_rows"]
    # _detrend_rows (injection_recovery, null_sde)
    ctx = _Recorder()
    survey._detrend_rows(ctx, _T, y, (survey.Clean(0.2, n_iter=1), survey.Biweight(0.2)))
    assert ctx.calls[0][0] == "clean_rows" and ctx.calls[0][2] == dict(window_length=0.2, break_tolerance=0.5, sigma_upper=4.0,
                                                                       sigma_lower=INF, max_run=1, n_iter=1, min_points=3)
    assert ctx.calls[1][0] == "biweight_detrend"
    # the step is accepted by the calls that form masks themselves, and checked before any device work everywhere
    bad = survey.Clean(n_iter=99)
    message = "cleaning: n_iter must be an integer in \\[0, 16\\], got 99"
    for call in (lambda: survey.power_batch(_T, y, detrend=bad), lambda: survey.search_batch(_T, y, detrend=(bad, 3)),
                 lambda: survey.power_results(_T, y, detrend=bad), lambda: survey.lomb_scargle(_T, y, detrend=bad),
                 lambda: survey.single_transits(_T, y, detrend=bad),
                 lambda: survey.power_batch_protected(_T, y, (bad, survey.Biweight(0.2)), 7.0),
                 lambda: survey.power_batch_multi(_T, y, 7.0, detrend=(bad, survey.Biweight(0.2)), protect_factor=1.5),
                 lambda: survey.null_sde(_T, 4, detrend=bad, sigma=1e-3),
                 lambda: survey.injection_recovery(_T, y[0], {"T0": [0.1], "period": [0.1], "rp_rs": [0.05], "a": [10.0], "inc": [90.0]},
                                                   detrend=(bad, survey.Biweight(0.5)))):
        with pytest.raises(ValueError, match=message):
            call()
    # the messages of the steps before stay
    with pytest.raises(ValueError, match="a step of detrend must be a kernel size, a Biweight or a SysRem"):
        survey._detrend_steps((step, None))
    with pytest.raises(ValueError, match="detrend_mask: the median filter \\(detrend=3\\) is defined by its sample count"):
        survey._detrended(_T, _Y, (step, 3), _Recorder(), None, None, detrend_mask=mask)


def test_nan_is_refused_without_the_step():
    """Non-finite flux passes only behind a Clean at the head of detrend; everywhere else today's messages stand."""
    _T = 1.0 + numpy.arange(480) / 48.0
    y = 1.0 + 1e-3 * numpy.sin(numpy.arange(960.0)).reshape(2, 480)
    y[1, 3] = numpy.nan
    ctx = _Recorder()
    for call, message in (
            (lambda: survey.power_batch(_T, y, context=ctx), "light curve 1 has a NaN, infinite or non-positive flux"),
            (lambda: survey.search_batch(_T, y, context=ctx), "light curve 1 has a NaN, infinite or non-positive flux"),
            (lambda: survey.biweight_batch(_T, y, 0.2, context=ctx), "flux has a NaN, infinite or non-positive value"),
            (lambda: survey.detrend_batch(y, 3, context=ctx), "NaN|non-finite|finite"),
            (lambda: survey.spline_batch(_T, y, 0.1, context=ctx), "spline detrending: flux has a NaN, infinite or non-positive value"),
            (lambda: survey.lomb_scargle(_T, y, context=ctx), "NaN|finite"),
            (lambda: survey.power_batch(_T, y, detrend=(survey.Biweight(0.2), survey.Clean()), context=ctx),
             "flux has a NaN, infinite or non-positive value"),
            (lambda: survey.power_batch(_T, y, detrend=(3, survey.Clean()), context=ctx), "NaN|non-finite|finite"),
            (lambda: survey.lomb_scargle(_T, y, detrend=(survey.Biweight(0.2), survey.Clean()), context=ctx), "NaN|finite"),
            (lambda: survey.injection_recovery(_T, y[1], {"T0": [0.1], "period": [0.1], "rp_rs": [0.05], "a": [10.0], "inc": [90.0]},
                                               detrend=(survey.Biweight(0.5), survey.Clean()), context=ctx),
             "flux has a NaN, infinite or non-positive value")):
        with pytest.raises(ValueError, match=message):
            call()
    assert ctx.calls == []


# ---- align_rows -------------------------------------------------------------------------------------------------------------
def test_align_rows():
    t = numpy.arange(10.0) * 0.5                     # the grid: 0, 0.5, ..., 4.5; tolerance 0.25 by default
    times = [numpy.array([0.01, 0.25, 0.5, 0.74, 3.9, 20.0]),      # 0.25 ties between 0 and 0.5: the lower index; 20.0 is dropped
             numpy.array([]),                                      # an empty star
             numpy.array([1.0, 1.0, 1.1, 4.4])]                    # three samples on one stamp
    fluxes = [numpy.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), numpy.array([]), numpy.array([1.0, 2.0, 6.0, numpy.nan])]
    rows, dropped, mean, largest = survey.align_rows(times, fluxes, t)
    assert rows.shape == (3, 10) and dropped.tolist() == [1, 0, 0] and dropped.dtype == numpy.int64
    want = numpy.full((3, 10), numpy.nan)
    want[0, [0, 1, 8]] = [(1.0 + 2.0) / 2.0, (3.0 + 4.0) / 2.0, 5.0]
    want[2, 2] = ((1.0 + 2.0) + 6.0) / 3.0
    assert cases.same(rows[:, :9], want[:, :9]) and numpy.isnan(rows[2, 9])     # (a NaN sample stays one: clean_batch flags it)
    offsets = numpy.array([0.01, 0.25, 0.0, 0.74 - 0.5, 3.9 - 4.0])
    assert mean[0] == offsets.mean() and largest[0] == 0.25 and numpy.isnan(mean[1]) and numpy.isnan(largest[1])
    assert abs(mean[2] - (0.0 + 0.0 + 0.1 - 0.1) / 4.0) < 1e-15 and abs(largest[2] - 0.1) < 1e-15
    # a tolerance of its own; a sample beyond it is dropped, one on it is kept
    rows, dropped, _, _ = survey.align_rows([numpy.array([0.1, 0.6, 1.05])], [numpy.array([1.0, 2.0, 3.0])], t, tolerance=0.1)
    assert dropped.tolist() == [0] and rows[0, :3].tolist() == [1.0, 2.0, 3.0]
    rows, dropped, _, _ = survey.align_rows([numpy.array([0.1, 0.6, 1.05])], [numpy.array([1.0, 2.0, 3.0])], t, tolerance=0.06)
    assert dropped.tolist() == [2] and numpy.isnan(rows[0, :2]).all() and rows[0, 2] == 3.0
    for args, message in ((([[0.0]], [[1.0]], t[::-1]), "align_rows: t must be finite and non-decreasing"),
                          (([[0.0]], [[1.0]], [0.0, 0.0, 1.0]), "align_rows: the grid t must ascend strictly"),
                          (([[1.0, 0.0]], [[1.0, 1.0]], t), "align_rows: star 0: the time stamps must be finite and sorted"),
                          (([[0.0, 1.0]], [[1.0]], t), "align_rows: star 0: time stamps and flux must be 1-d and of one length"),
                          (([[0.0]], [[1.0], [2.0]], t), "align_rows: times and fluxes must have one entry a star each"),
                          (([[0.0]], [[1.0]], t, -1.0), "align_rows: tolerance must be finite and >= 0")):
        with pytest.raises(ValueError, match=message):
            survey.align_rows(*args)
    # the stated way: align, clean, search -- the rows align_rows makes are what clean_arguments takes
    a = _lib.clean_arguments(t, survey.align_rows(times, fluxes, t)[0])
    assert a["y"].shape == (3, 10)
