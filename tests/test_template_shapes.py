"""Every search family, the chain behind it and the survey stages that take a template, on tables that are NOT the default
planet's (template_shapes.py): the two presets, a limb-brightened grazing transit, eccentric orbits -- asymmetric rows, and
rows SHORTER than their width --, and three synthetic tables (flat, skew, cusp3).

(a) Every shape against the long-double STATEMENT of the search (search_spec.py, which values a short row as the reference
    does) as test_input_scales.py reads the default table: chi2 within RTOL_TIGHT, rows wherever the statement's gap exceeds
    1e-8, the argmin period, depth, chi2 == n, RTOL_CONTRACT against the oracle, the counting launch bit for bit and both
    work counters -- the four uniform-weight variants at 1500 and 2900 points, per-point weights at 1500 and 2891, exact
    prefix-sum mode.  A table with a short row takes the plain classic kernel whatever variant is forced (include/tls_amd.h):
    asserted, not skipped.
(b) The pruning variant and the fp32 screen, forced, on tables whose rows the pruning bound holds for only in part (cusp3) or
    not at all (the short shapes): the plain kernel's bits at three noise levels, parity with the oracle, never chosen
    without forcing, and the same bits after the LDS was poisoned.
(c) The family edges of plan_edges.py (4350 to 8907 points, 2892 and 5930 weighted) with 40 periods, strided rows among
    them, against the oracle with all three counters, on both sort paths of the slab.
(d) The chain: power() against power() fed by the oracle, the final T0 fit's two kernels on an asymmetric and on a short row,
    survey.power_results and power_batch(models=True) against power() per curve, the peak fits' rank-0 invariant.
(e) One compact case per survey stage that builds a template from power()'s keywords, each equal to its spec bit for bit.

Measured on an MI355X (153 tests, 7 s; largest |chi2 - statement| / statement over a case's 14 periods, 1500 / 2900 (2891)
points; the oracle's distance on the same periods beside it):

                 uniform weights, all four variants       per-point weights: uniform(0.7, 1.4)   both, R = 100        oracle
    shape        device (the same bits)   oracle          device                                 device
    grazing      9.9e-13 / 1.8e-12        1.1e-14 / 1.4e-14   2.6e-12 / 1.6e-12                  1.7e-10 / 1.5e-11    6.0e-13 / 3.3e-13
    box          7.4e-13 / 2.6e-12        6.3e-15 / 6.0e-15   2.0e-12 / 1.6e-12                  2.2e-10 / 8.3e-11    7.2e-13 / 1.0e-13
    grazing_ld   1.4e-12 / 1.6e-12        1.6e-14 / 7.3e-15   2.8e-12 / 1.8e-12                  1.7e-10 / 4.7e-11    3.6e-13 / 5.1e-13
    ecc_full     8.3e-13 / 2.2e-12        1.7e-14 / 8.4e-15   2.6e-12 / 1.5e-12                  2.1e-10 / 5.8e-11    1.0e-12 / 3.4e-13
    ecc_short    2.5e-12 / 2.5e-12        1.2e-14 / 6.3e-15   2.0e-12 / 1.9e-12                  1.0e-10 / 2.4e-11    5.0e-13 / 2.8e-13
    grazing_ecc  2.6e-12 / 1.9e-12        1.3e-14 / 1.2e-14   2.2e-12 / 1.9e-12                  1.1e-10 / 2.4e-11    5.5e-13 / 2.4e-13
    flat         7.3e-17 / 1.0e-16        2.6e-15 / 4.7e-15   1.7e-12 / 1.7e-12                  1.2e-10 / 4.3e-10    4.4e-15 / 4.6e-15
    skew         3.2e-12 / 2.7e-12        1.2e-14 / 1.3e-14   5.4e-12 / 2.4e-12                  2.6e-10 / 9.4e-11    8.6e-13 / 4.2e-13
    cusp3        2.9e-12 / 2.0e-12        1.7e-14 / 1.6e-14   4.8e-12 / 2.6e-12                  1.4e-10 / 5.2e-11    5.2e-13 / 2.9e-13

    exact_prefix = 1 (dy none; both, R = 100):   skew 1.1e-16; 4.2e-16    ecc_short 1.2e-16; 4.2e-16    cusp3 3.4e-16; 1.2e-15

The two short shapes ran the plain classic kernel under every forced variant (asserted), the others the variant that was
forced; with a few points a hundred times more precise the device's distance is fast mode's depth scale, as on the default
table (test_input_scales.py), and exact mode sits at 1e-16 on a short row as on a full one.  Rows, depths,
the argmin and both work counters agreed in every case.  The family edges of (c) sit 2.8e-13 to 8.7e-12 from the oracle.  The
T0 fit's rotation path is 4e-16 from the general kernel on both rows and 3e-15 from the oracle; the reversed row would be 1e-2
to 9e-2 off.
"""
import functools
import warnings

import numpy
import pytest

import plan_edges as pe
import search_spec
import template_shapes as T
import test_input_scales as scales
from conftest import oracle_search
from test_gpu_parity import RTOL_CONTRACT, RTOL_TIGHT, assert_parity

pytestmark = pytest.mark.gpu

N_PERIODS = 14
N_PERIODS_EDGE = 40
WEIGHTED_MAX = scales.WEIGHTED_MAX
VARIANTS = scales.VARIANTS
SERIES = ("k2", "gapped")
MEASURED = {}                       # case -> (device off the statement, oracle off the statement)


def _args(inp):
    return (inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])


def _kernel_for(inp, forced):
    """The kernel the library documents for a forced variant: a table with a short row takes the plain classic kernel."""
    return "resident" if pe.short_rows(inp) else forced


@functools.lru_cache(maxsize=None)
def _oracle(oracle_lib, shape, series, dy_name, n):
    inp = T.case(shape, series, dy_name, N_PERIODS, n)
    return oracle_search(oracle_lib, inp, periods=inp["selected"])


def _against_statement(gpu, oracle_lib, shape, series, dy_name, n, forced, mode=""):
    """One search of a case against the statement and the oracle (test_input_scales._against_statement's assertions)."""
    what = (shape, series, dy_name, forced) + ((mode,) if mode else ())
    inp = T.case(shape, series, dy_name, N_PERIODS, n)
    kernel = _kernel_for(inp, forced)
    n_points = len(inp["t"])
    spec = T.statement(shape, series, dy_name, N_PERIODS, n)
    want = _oracle(oracle_lib, shape, series, dy_name, n)
    chi2, row, depth = gpu.search(*_args(inp))[:3]
    assert gpu.last_kernel() == kernel, (what, gpu.last_kernel())
    dist, oracle_dist = search_spec.distance(chi2, spec["chi2"]), search_spec.distance(want[0], spec["chi2"])
    MEASURED[what] = (dist, oracle_dist)
    print("%-12s %-7s %-10s %-18s device off the statement %.2e   oracle %.2e   device off the oracle %.2e"
          % (shape, series, dy_name, " ".join(what[3:]), dist, oracle_dist, float(numpy.max(numpy.abs(chi2 - want[0]) / want[0]))))
    assert numpy.isfinite(chi2).all() and numpy.isfinite(spec["chi2"]).all(), what
    assert dist <= RTOL_TIGHT, (what, dist)
    T.S.rows_agree(row, spec, what)
    assert int(numpy.argmin(chi2)) == spec["argmin"] or spec["period_gap"] <= 1e-8, what
    numpy.testing.assert_allclose(depth, spec["depth"], rtol=0, atol=max(1e-12, 3e-16 * n_points), err_msg=str(what))
    numpy.testing.assert_array_equal(chi2 == n_points, spec["chi2"] == n_points, err_msg=str(what))
    numpy.testing.assert_allclose(chi2, want[0], rtol=RTOL_CONTRACT, atol=0, err_msg=str(what))
    # a counting launch (the pruning and the screen variants have none: theirs is the plain kernel's) returns the same bits
    counted = gpu.search(*_args(inp), count_work=True)
    assert gpu.last_kernel() == kernel.split("+")[0], (what, gpu.last_kernel())
    for a, b in zip(counted[:3], (chi2, row, depth)):
        assert a.tobytes() == b.tobytes(), what
    assert counted[3]["evaluated_cells"] == int(want[3][1]) == int(spec["evaluated_cells"].sum()), what
    assert counted[3]["inner_steps"] == int(want[3][2]) == int(spec["inner_steps"].sum()), what


# ---- (a) against the statement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", sorted(VARIANTS))
@pytest.mark.parametrize("series", SERIES)
@pytest.mark.parametrize("shape", T.SHAPES)
def test_uniform_weights_against_the_statement(gpu, oracle_lib, shape, series, kernel):
    """The four-slot kernel and the classic kernel's plain, fp32-screen and pruning variants: 1500 and 2900 points."""
    gpu.set_options(**VARIANTS[kernel])
    _against_statement(gpu, oracle_lib, shape, series, "none", None, kernel)


@pytest.mark.parametrize("series", SERIES)
@pytest.mark.parametrize("shape", T.SHAPES)
def test_per_point_weights_against_the_statement(gpu, oracle_lib, shape, series):
    """The classic kernel two a CU (A and B both sliding dot products): 1500 and 2891 points."""
    n = None if series == "k2" else WEIGHTED_MAX
    gpu.set_options(prune=0, screen32=0)
    for dy_name in ("uniform", "both_R100"):
        inp = T.case(shape, series, dy_name, N_PERIODS, n)
        assert pe.expected_plan(*pe.shape(inp), uniform=False, short_rows=pe.short_rows(inp)) == ("resident", 2)
        _against_statement(gpu, oracle_lib, shape, series, dy_name, n, "resident")


@pytest.mark.parametrize("series", SERIES)
@pytest.mark.parametrize("shape", ["skew", "ecc_short", "cusp3"])
def test_exact_prefix_mode_against_the_statement(gpu, oracle_lib, shape, series):
    """The classic kernel with the reference's own prefix sum throughout (switch exact_prefix)."""
    gpu.set_options(exact_prefix=1, prune=0, screen32=0)
    for dy_name in ("none", "both_R100"):
        _against_statement(gpu, oracle_lib, shape, series, dy_name, None if series == "k2" or dy_name == "none" else WEIGHTED_MAX,
                           "resident", mode="exact prefix")


# ---- (b) the pruning variant and the fp32 screen on mixed tables ---------------------------------------------------------------

def _bits_equal(a, b, what):
    for x, y in zip(a[:3], b[:3]):
        numpy.testing.assert_array_equal(x, y, err_msg=str(what))


@pytest.mark.parametrize("sigma", [50e-6, 500e-6, 3000e-6])
@pytest.mark.parametrize("shape", ["cusp3", "ecc_short", "grazing_ecc"])
def test_forced_pruning_and_screen_return_the_plain_kernels_bits(gpu, oracle_lib, shape, sigma):
    """As test_pruning_kernel_is_exact and test_fp32_screen_kernel_is_exact compare the variants, on a table with rows the
    pruning bound does not hold for (cusp3: a forced launch evaluates them always, beside screened and bounded rows) and on
    tables of short rows (which the library keeps in the plain kernel)."""
    inp = T.noisy_case(shape, sigma)
    what = (shape, sigma)
    prunable = T.k_mono(inp["table"]) >= 0
    assert (shape == "cusp3") == (prunable.any() and not prunable.all() and not pe.short_rows(inp))
    gpu.set_options(prune=0, screen32=0)
    plain = gpu.search(*_args(inp))
    assert gpu.last_kernel() == "resident", what
    want = oracle_search(oracle_lib, inp, periods=inp["selected"])
    assert_parity(plain, want, len(inp["t"]))
    for no_screen in (0, 1):
        gpu.set_options(prune=1, prune_min_live=0, no_screen=no_screen, screen32=0)
        pruned = gpu.search(*_args(inp))
        assert gpu.last_kernel() == _kernel_for(inp, "resident+prune"), (what, gpu.last_kernel())
        _bits_equal(plain, pruned, what + ("prune", no_screen))
    gpu.set_options(prune=0, screen32=1, no_screen=None)
    screened = gpu.search(*_args(inp))
    assert gpu.last_kernel() == _kernel_for(inp, "resident+screen32"), (what, gpu.last_kernel())
    _bits_equal(plain, screened, what + ("screen32",))
    counted = gpu.search(*_args(inp), count_work=True)
    _bits_equal(plain, counted, what + ("counted",))
    assert counted[3]["evaluated_cells"] == int(want[3][1]) and counted[3]["inner_steps"] == int(want[3][2]), what
    # without forcing, a table with a row the bound does not hold for never takes the pruning variant
    gpu.set_options(prune=None, screen32=None, no_screen=None, prune_min_live=None)
    free = gpu.search(*_args(inp))
    assert gpu.last_kernel() != "resident+prune", (what, gpu.last_kernel())
    if pe.short_rows(inp):
        assert gpu.last_kernel() == "resident", (what, gpu.last_kernel())
    _bits_equal(plain, free, what + ("free",))


@pytest.mark.parametrize("shape", ["cusp3", "ecc_short", "grazing_ecc"])
def test_mixed_tables_do_not_depend_on_what_the_lds_held_before(gpu, shape):
    inp = T.noisy_case(shape, 500e-6)
    for options in (dict(prune=0, screen32=0), dict(prune=1, prune_min_live=0, no_screen=0, screen32=0),
                    dict(prune=1, prune_min_live=0, no_screen=1, screen32=0), dict(prune=0, screen32=1)):
        gpu.set_options(**options)
        before = gpu.search(*_args(inp))
        gpu.poison_lds(0x7ff80000)
        after = gpu.search(*_args(inp))
        _bits_equal(before, after, (shape, sorted(options.items()), gpu.last_kernel()))


# ---- (c) the family edges ---------------------------------------------------------------------------------------------------

def test_the_edge_lengths_are_test_input_scales():
    assert [(n, w) for n, w, _, _ in scales._edge_lengths()] == [(4350, False), (5121, False), (8890, False), (8906, False),
                                                                 (8907, False), (2892, True), (5930, True)]


def _edge_case(gpu, oracle_lib, shape, index, margin=None):
    n, weighted, kernel, slots = scales._edge_lengths()[index]
    inp = T.case(shape, "gapped", "down_R1000" if weighted else "none", N_PERIODS_EDGE, n, margin)
    default = T.case("default", "gapped", "down_R1000" if weighted else "none", N_PERIODS_EDGE, n, margin)
    numpy.testing.assert_array_equal(inp["table"].width, default["table"].width)
    plan = pe.expected_plan(*pe.shape(inp), uniform=not weighted, short_rows=pe.short_rows(inp))
    if margin is None and not pe.short_rows(inp):
        assert plan == (kernel, slots), (shape, n, plan)
    elif margin is None:               # a short row: the classic kernel in place of the four-slot one, the slab as it was
        assert plan[0] == (kernel if kernel.startswith(("slab", "resident")) else "resident"), (shape, n, plan)
    if plan[0] == "resident":
        gpu.set_options(prune=0, screen32=0)               # (the plain variant, whatever the noise level suggests)
    scales._parity(gpu, oracle_lib, inp, plan[0], (shape, n, margin))
    if plan[0].startswith("slab"):
        gpu.set_options(sort2=0)                           # the general bucket sort in place of the two-level one
        scales._parity(gpu, oracle_lib, inp, plan[0], (shape, n, margin, "sort2", 0))


@pytest.mark.parametrize("index", range(7))
@pytest.mark.parametrize("shape", ["grazing", "skew", "ecc_short", "cusp3"])
def test_family_edges_against_the_oracle(gpu, oracle_lib, shape, index):
    _edge_case(gpu, oracle_lib, shape, index)


@pytest.mark.parametrize("index", [2, 4])
@pytest.mark.parametrize("shape", ["skew", "ecc_short"])
def test_family_edges_with_strided_rows(gpu, oracle_lib, shape, index):
    """T0_fit_margin = 0.1 at 8890 and 8907 points: windows up to a tenth of their width apart."""
    n = scales._edge_lengths()[index][0]
    inp = T.case(shape, "gapped", "none", N_PERIODS_EDGE, n, 0.1)
    width = numpy.asarray(inp["table"].width)
    assert max(search_spec.stride(int(d), 0.1) for d in width) >= 50
    _edge_case(gpu, oracle_lib, shape, index, margin=0.1)


# ---- (d) the chain ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["grazing", "box", "ecc_short", "grazing_ecc"])
def test_power_equals_power_with_the_oracles_search(monkeypatch, oracle_lib, shape):
    """test_gpu_power.test_power_gpu_equals_power_with_oracle_search's pattern and tolerances under a shape's keywords, key
    for key: 1440 points, with uniform weights and with a dy."""
    import pins
    import tls_amd
    from tls_amd import transit_model
    rng = numpy.random.RandomState(3)
    n = 1440
    t = numpy.linspace(2.0, 32.0, n)
    y = transit_model.light_curve(t, 2.5, 3.3, 0.05, 12, 89.8, 0, 90, [0.4, 0.3], "quadratic") + rng.normal(0, 3e-4, n)
    kwargs = dict(period_min=1.0, period_max=10.0, oversampling_factor=2, T0_fit_margin=0.01, verbose=False,
                  show_progress_bar=False, **T.KEYWORD_SHAPES[shape])
    for dy in (None, rng.uniform(0.8, 1.3, n) * 3e-4):
        with warnings.catch_warnings(), monkeypatch.context() as m:
            warnings.simplefilter("ignore")
            got = tls_amd.transitleastsquares(t, y, dy, verbose=False).power(**kwargs)

            def oracle_search_periods(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                      M_star_min, M_star_max, T0_fit_margin, **_unused):
                assert bool((numpy.asarray(table.length) < numpy.asarray(table.width)).all()) == (shape in T.SHORT_SHAPES)
                return oracle_lib.search(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                         M_star_min, M_star_max, T0_fit_margin)[:3]

            m.setattr(tls_amd.search, "spectra", lambda chi2_, osf_, **kw: oracle_lib.spectra(chi2_, int(osf_ * 30)))
            m.setattr(tls_amd.search, "search_periods", oracle_search_periods)
            m.setattr(tls_amd.search, "t0_fit_residuals",
                      lambda t_, y_, p_, s_, e_, r_, **kw: oracle_lib.t0_residuals(t_, y_, p_, s_, e_, r_))
            want = tls_amd.transitleastsquares(t, y, dy, verbose=False).power(**kwargs)
        assert list(got.keys()) == list(want.keys())
        assert abs(got.period - 3.3) < 0.02 and got.SDE > 10
        for key in pins.SCALARS:
            numpy.testing.assert_allclose(float(got[key]), float(want[key]), rtol=1e-9, atol=1e-12, err_msg=key)
        for key in pins.ARRAYS:
            atol = 2e-9 if key in ("power", "power_raw", "SR") else 1e-11     # (as the pattern: SR's spread is 1e-3)
            numpy.testing.assert_allclose(numpy.asarray(got[key], dtype=float), numpy.asarray(want[key], dtype=float),
                                          rtol=1e-9, atol=atol, err_msg=key)
        assert int(numpy.argmin(got.chi2)) == int(numpy.argmin(want.chi2))


@pytest.mark.parametrize("shape", ["skew", "ecc_short"])
def test_t0_fit_on_an_asymmetric_and_on_a_short_row(gpu, oracle_lib, shape):
    """The final T0 fit of k2_90d with a row of the shape's table (ecc_short: one sample shorter than its width): the rotation
    path and the general kernel agree as test_t0_fit_rotation_path_equals_the_general_kernel holds them (1e-13, the same
    first-minimum epoch), and both equal the oracle's residuals to 1e-12.  Read backwards the row gives other residuals."""
    t, f, kw = T.synthetic.config("k2_90d")
    inp = T._shaped(shape, t, f, None, kw)
    r = len(inp["rows"]) // 3
    row = numpy.asarray(inp["rows"][r])
    assert (len(row) < inp["overview"]["width_in_samples"][r]) == (shape in T.SHORT_SHAPES)
    signal = 1 - (1 - row) * 0.002
    period = 10.12452
    roll = int(len(signal) / 2) + 1
    points = min(len(t), int(len(t) / (0.01 * len(signal))))
    epochs = numpy.linspace(inp["t"].min(), inp["t"].min() + period, points)
    gpu.set_options(t0_rot=None)
    got = gpu.t0_fit_residuals(inp["t"], inp["y"], period, signal, epochs, roll)
    gpu.set_options(t0_rot=0)
    general = gpu.t0_fit_residuals(inp["t"], inp["y"], period, signal, epochs, roll)
    gpu.set_options(t0_rot=None)
    ref = oracle_lib.t0_residuals(inp["t"], inp["y"], period, signal, epochs, roll)
    back = oracle_lib.t0_residuals(inp["t"], inp["y"], period, signal[::-1].copy(), epochs, roll)
    print("T0 fit on a %s row of %d samples: rotation path %s the general kernel's bits, %.1e apart; %.1e off the oracle; "
          "the reversed row %.1e off" % (shape, len(signal), "has" if got.tobytes() == general.tobytes() else "has not",
                                        float(numpy.max(numpy.abs(got - general) / general)),
                                        float(numpy.max(numpy.abs(got - ref) / ref)), float(numpy.max(numpy.abs(back - ref) / ref))))
    assert float(numpy.max(numpy.abs(back - ref) / ref)) > 1e-6           # (what makes the two comparisons below see a reversal)
    for res, name in ((got, "rotation"), (general, "general")):
        numpy.testing.assert_allclose(res, ref, rtol=1e-12, atol=0, err_msg=name)
        assert int(numpy.argmin(res)) == int(numpy.argmin(ref)), name
    numpy.testing.assert_allclose(got, general, rtol=1e-13, atol=0)
    assert epochs[int(numpy.argmin(got))].tobytes() == epochs[int(numpy.argmin(general))].tobytes()


@pytest.mark.parametrize("shape", ["grazing", "ecc_short"])
def test_survey_results_equal_power_per_curve(gpu, shape):
    """survey.power_results (power_batch(models=True) behind it: the model template of the shape) on 3 curves, one of them
    without a fit: all 41 keys equal power()'s of the curve on its own; and power_batch(peaks=3, peak_fits=True) keeps its
    rank-0 invariant -- the first peak is the pick wherever the two indices agree."""
    import test_power_batch_results as results
    from tls_amd import _lib, survey
    t = results.gapped_time()
    fluxes = results.batch(t, 6, 11)[0][[0, 1, 5]]
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02, **T.KEYWORD_SHAPES[shape])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_results(t, fluxes, None, context=gpu, **kw)
        assert len(got) == 3 and numpy.isnan(got[2].period) and not numpy.isnan(got[0].period)
        for s in range(3):
            results.assert_results_equal(got[s], results.power_of(t, fluxes[s], None, gpu, kw), "%s curve %d" % (shape, s))
        summary, periods, chi2, row, depth, power, pk = survey.power_batch(
            t, fluxes, None, context=gpu, statistics=True, peaks=3, peak_fits=True, with_arrays=True, **kw)
    for s in range(3):
        numpy.testing.assert_array_equal(chi2[s], got[s].chi2, err_msg="curve %d" % s)
    peaks = pk["peaks"]
    same = numpy.flatnonzero((summary["index_best"] == summary["index_power"]) & (summary["no_fit"] == 0))
    assert summary["no_fit"].tolist() == [0, 0, 1] and len(same) >= 1
    for c in same:
        assert peaks["index"][c, 0] == summary["index_power"][c] and peaks["status"][c, 0] == 0
        for k in ("T0", "rp_rs") + _lib.TRANSIT_STATS_FIELDS:
            numpy.testing.assert_array_equal(float(peaks[k][c, 0]), float(summary[k][c]), err_msg=str((c, k)))


# ---- (e) the survey stages that build a template from power()'s keywords ------------------------------------------------------
# One compact case a stage through survey.<stage>(..., **template keywords), compared as the stage's own module compares
# its survey call with its spec (every field bit for bit): a grazing transit on an eccentric orbit.

STAGE_KW = dict(transit_template="grazing", ecc=0.6, w=20)


def _stage_rows(t, flux, dy):
    from tls_amd import survey
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, dy, dict(STAGE_KW, oversampling_factor=1))
    assert inp["shape"]["ecc"] == 0.6 and inp["shape"]["w"] == 20
    return inp, y_rows, dy_rows


def test_single_transits_with_template_keywords(gpu):
    import test_single_transit as m
    from tls_amd import survey
    n = 1000
    t = m.series(n, 400, 40)
    flux = m.curves(n, 3, 10)
    dy = numpy.random.RandomState(11).uniform(0.5, 2.0, flux.shape) * 1e-3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.single_transits(t, flux, dy, context=gpu, with_arrays=True, **STAGE_KW)
        default = survey.single_transits(t, flux, dy, context=gpu, with_arrays=True)
    inp, y_rows, dy_rows = _stage_rows(t, flux, dy)
    widths = survey.single_transit_widths(t)
    want = m.spec.expected(t, y_rows, dy_rows, widths, m.spec.shapes_of(widths, **inp["shape"]), m.spans_of(t, widths))
    for f in m.spec.FIELDS:
        m.expect_equal(got[0][f], want[0][f], f)
    for a, b in zip(got[1:], want[1:]):
        m.expect_equal(a, b, "planes")
    assert (got[1] >= 1).all() and not numpy.array_equal(got[2], default[2], equal_nan=True)


def test_transit_times_with_template_keywords(gpu):
    import test_transit_times as m
    from tls_amd import survey
    flux = numpy.array([m.curve_of(s) for s in range(2)])
    dy = numpy.random.RandomState(3).uniform(3e-4, 6e-4, flux.shape)
    period, T0, duration = [1.9, 3.1, 1.9], [3.4, 4.0, 3.9], [0.09, 0.11, 0.02]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eph, times = survey.transit_times(m.T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, search=2.0, min_ses=0.0,
                                          context=gpu, **STAGE_KW)
        default = survey.transit_times(m.T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, search=2.0, min_ses=0.0,
                                       context=gpu)
    inp, y_rows, dy_rows = _stage_rows(m.T, flux, dy)
    widths, span_max, row, reach = survey.transit_time_rows(m.T, period, duration, 2.0)
    want = m.spec.expected(m.T, y_rows, dy_rows, [0, 1, 1], period, T0, row, reach, m.spec.shapes_of(widths, **inp["shape"]),
                           span_max, 0.0, 0.0, times.shape[1])
    m.equal_records(eph, want[0], m.spec.EPHEMERIS_FIELDS, "template keywords")
    m.equal_records(times, want[1], m.spec.TIME_FIELDS, "template keywords")
    assert (eph["n_timed"] >= 2).all() and times.tobytes() != default[1].tobytes()


def test_event_vetting_with_template_keywords(gpu):
    import test_event_vetting as m
    from tls_amd import survey
    flux = numpy.array([m.curve_of(s) for s in range(2)])
    dy = numpy.random.RandomState(3).uniform(3e-4, 6e-4, flux.shape)
    period, T0, duration = [1.9, 3.1, 1.9], [3.4, 4.0, 3.9], [0.09, 0.11, 0.02]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, events = survey.event_vetting(m.T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, search=2.0,
                                           chase_window=0.25, guard=1.0, context=gpu, **STAGE_KW)
        default = survey.event_vetting(m.T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, search=2.0,
                                       chase_window=0.25, guard=1.0, context=gpu)
    inp, y_rows, dy_rows = _stage_rows(m.T, flux, dy)
    widths, span_max, row, reach, chase_reach, guard, chase_span = survey.event_vetting_rows(m.T, period, duration, 2.0, 0.25, 1.0)
    want = m.spec.expected(m.T, y_rows, dy_rows, [0, 1, 1], period, T0, row, reach, chase_reach, guard, chase_span,
                           m.spec.shapes_of(widths, **inp["shape"]), span_max, max_epochs=events.shape[1])
    m.equal_records(out, want[0], m.spec.SUMMARY_FIELDS, "template keywords")
    m.equal_records(events, want[1], m.spec.EVENT_FIELDS, "template keywords")
    assert (out["n_epochs"] >= 2).all() and events.tobytes() != default[1].tobytes()


def test_centroid_test_with_template_keywords(gpu):
    import test_centroid as m
    from tls_amd import survey
    rows = [m.curve_of(s) for s in range(3)]
    flux, cx, cy = (numpy.array([r[i] for r in rows]) for i in range(3))
    period, T0, duration = [1.9, 3.1, 1.9], [3.4, 4.0, 3.9], [0.09, 0.11, 0.02]
    options = dict(window=2.0, min_in=2, min_out=4, max_epochs=7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = survey.centroid_test(m.T, flux, cx, cy, period, T0, duration, curve=[2, 1, 1], context=gpu, **options, **STAGE_KW)
        default = survey.centroid_test(m.T, flux, cx, cy, period, T0, duration, curve=[2, 1, 1], context=gpu, **options)
    inp, y_rows, _ = _stage_rows(m.T, flux, None)
    raw = m.spec.centroid_batch(m.T, y_rows, cx, cy, period, T0, duration, [2, 1, 1], survey._centroid_shape(inp), **options)
    for i, k in enumerate(m.spec.FIELDS):
        m.expect_equal(out["cen_" + k], raw[:, i], k)
    assert (out["cen_status"][:2] == 0).all() and out["cen_depth"][0] != default["cen_depth"][0]

