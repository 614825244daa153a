"""Every search family, the chain behind it and the survey stages at the input scales of survey data (input_scales.py):
time stamps at JD offsets 0, 1325 and 2457000 -- where a double resolves 4.7e-10 d --, and dy of wide range.

(a) At up to 3000 points every family is read against the long-double STATEMENT of the search (search_spec.py), not only
    against the CPU oracle: chi2 within RTOL_TIGHT of the statement (the device has no running sum: it sits closer to the
    definition than the reference's arithmetic does), rows and the argmin period wherever the statement's gap exceeds 1e-8,
    depth within assert_parity's bound, chi2 within RTOL_CONTRACT of the oracle, and the oracle's evaluated cells and template
    samples -- the cell set is exact at any offset and any dy.
(b) At the smallest lengths that select each remaining family (plan_edges.py), against the oracle by assert_parity, with the
    fold and the prefix sum bit for bit against numpy on every sort path at offset 2457000.
(c) The chain: power(), power_batch with statistics and peak fits, and the final T0 fit's rotation path.
(d) One compact case per survey stage at offset 2457000, each equal to its spec bit for bit.

Measured on an MI355X (71 tests, 9 s; largest |chi2 - statement| / statement over a case's 14 periods and over the three
offsets, which do not show; the oracle's distance on the same periods beside it):

    dy                                    device, 1500 / 2900 (2891) points    oracle                device, exact_prefix = 1
    uniform weights, all four variants    9.3e-13 / 2.2e-12 (the same bits)    1.4e-14 / 1.9e-14     1.2e-16 / 8.8e-17
    uniform(0.7, 1.4), 15 points x R      6.7e-12 / 1.5e-12                    1.7e-14 / 1.8e-14
    5 points / R or both, R = 10          2.6e-11 / 1.5e-12                    1.2e-13 / 1.5e-14
    5 points / R or both, R = 1e2, 1e3    2.3e-10 / 2.1e-10                    8.5e-13 / 1.1e-12     5.2e-16 / 4.5e-16
    both, R = 1e4                         0 (nothing fitted) / 2.1e-10         0 / 1.1e-12

With a few points far more precise than the rest the device sits 2e-10 from the statement, two orders farther than the
oracle: that is fast mode's depth scale (taken from the exact running sum, not from the reference's rounded cumsum), which
moves chi2 in first order once the unweighted window mean is far from the weighted optimum -- in exact mode the same kernel
is 5e-16 from the statement.  Rows, depths, the argmin and both work counters agreed in every case; the
family edges of (b) sit 3e-14 to 3.9e-12 from the oracle; the rotation path of the T0 fit is taken at both offsets, 4e-16
from the general kernel's residuals, the same epoch."""
import functools
import warnings

import numpy
import pytest

import input_scales as S
import plan_edges as pe
import search_spec
from conftest import oracle_search
from test_gpu_parity import RTOL_CONTRACT, RTOL_TIGHT, assert_parity, _folded_reference

pytestmark = pytest.mark.gpu

N_PERIODS = 14                      # (a): 12 to 16 periods a case
N_PERIODS_EDGE = 40                 # (b)
WEIGHTED_MAX = 2891                 # the last length the classic kernel holds two a CU with per-point weights (plan_edges)
JD = 2457000.0

# the switches that force each variant of the uniform-weight families (test_slim_dense_predicate.FORCE_SLIM)
VARIANTS = {
    "slim": dict(slim=1, prune=0, screen32=0),
    "resident": dict(slim=0, prune=0, screen32=0),
    "resident+screen32": dict(slim=0, prune=0, screen32=1),
    "resident+prune": dict(slim=0, prune=1, screen32=0, prune_min_live=0),
}
MEASURED = {}                       # case -> (device off the statement, oracle off the statement)


def _args(inp):
    return (inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])


@functools.lru_cache(maxsize=None)
def _oracle(oracle_lib, series, offset, dy_name, n_periods, n):
    inp = S.case(series, offset, dy_name, n_periods, n)
    return oracle_search(oracle_lib, inp, periods=inp["selected"])


def _against_statement(gpu, oracle_lib, series, offset, dy_name, n, kernel, mode=""):
    """One search of a case against the statement and the oracle (the module docstring's list)."""
    what = (series, offset, dy_name, kernel) + ((mode,) if mode else ())
    inp = S.case(series, offset, dy_name, N_PERIODS, n)
    n_points = len(inp["t"])
    spec = S.statement(series, offset, dy_name, N_PERIODS, n)
    want = _oracle(oracle_lib, series, offset, dy_name, N_PERIODS, n)
    chi2, row, depth = gpu.search(*_args(inp))[:3]
    assert gpu.last_kernel() == kernel, (what, gpu.last_kernel())
    dist, oracle_dist = search_spec.distance(chi2, spec["chi2"]), search_spec.distance(want[0], spec["chi2"])
    MEASURED[what] = (dist, oracle_dist)
    print("%-7s offset %-8g %-18s %-18s device off the statement %.2e   oracle %.2e   device off the oracle %.2e"
          % (series, offset, dy_name, " ".join(what[3:]), dist, oracle_dist, float(numpy.max(numpy.abs(chi2 - want[0]) / want[0]))))
    assert numpy.isfinite(chi2).all() and numpy.isfinite(spec["chi2"]).all(), what
    assert dist <= RTOL_TIGHT, (what, dist)
    S.rows_agree(row, spec, what)
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
@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("series", ["k2", "gapped"])
def test_uniform_weights_against_the_statement(gpu, oracle_lib, series, offset, kernel):
    """The four-slot kernel and the classic kernel's plain, fp32-screen and pruning variants: 1500 and 2900 points."""
    gpu.set_options(**VARIANTS[kernel])
    _against_statement(gpu, oracle_lib, series, offset, "none", None, kernel)


@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("series", ["k2", "gapped"])
def test_per_point_weights_against_the_statement(gpu, oracle_lib, series, offset):
    """The classic kernel two a CU (A and B both sliding dot products): every dy case, 1500 and 2891 points."""
    n = None if series == "k2" else WEIGHTED_MAX
    gpu.set_options(prune=0, screen32=0)                   # (the plain variant, whatever the noise level suggests)
    for dy_name, kind, _ in S.DY_CASES:
        if kind is None:
            continue
        inp = S.case(series, offset, dy_name, N_PERIODS, n)
        assert pe.expected_plan(*pe.shape(inp), uniform=False) == ("resident", 2)
        _against_statement(gpu, oracle_lib, series, offset, dy_name, n, "resident")


@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("series", ["k2", "gapped"])
def test_exact_prefix_mode_against_the_statement(gpu, oracle_lib, series, offset):
    """The classic kernel with the reference's own prefix sum throughout (switch exact_prefix): the depth scale of a cell
    is then the statement's to the bit, and what is left of the distance is the rounding of the sums."""
    gpu.set_options(exact_prefix=1, prune=0, screen32=0)
    for dy_name in ("none", "precise_R1000", "both_R1000"):
        _against_statement(gpu, oracle_lib, series, offset, dy_name, None if series == "k2" or dy_name == "none" else WEIGHTED_MAX,
                           "resident", mode="exact prefix")


def test_the_no_fit_case_fits_nothing_and_the_others_fit():
    """(no GPU work: what the cases above searched) the R = 1e4 case of the k2 prefix is the no-fit path, in the others cells
    win."""
    for offset in S.OFFSETS:
        assert (S.statement("k2", offset, "both_R10000_nofit", N_PERIODS)["chi2"] == 1500).all()
        for dy_name in ("none", "both_R1000", "precise_R1000", "down_R1000"):
            assert (S.statement("k2", offset, dy_name, N_PERIODS)["chi2"] < 1500).all(), (offset, dy_name)


# ---- (b) against the oracle, at the family edges ----------------------------------------------------------------------------

def _edge(name):
    return [e for e in pe.PLAN_EDGES if e.name == name][0].model_edge()


@functools.lru_cache(maxsize=None)
def _edge_lengths():
    """[(n, weighted, kernel, periods a CU holds)]: the smallest lengths that select each family beyond (a)'s."""
    return ((_edge("quarter") + 1, False, "slim", 3), (_edge("registers") + 1, False, "slim512", 2),
            (_edge("half") + 1, False, "resident", 1), (_edge("resident") + 1, False, "slab+split", 1),
            (_edge("resident") + 2, False, "slab", 1),
            (_edge("two-per-cu-weighted") + 1, True, "resident", 1), (_edge("resident-weighted") + 1, True, "slab", 1))


def test_the_edge_lengths_are_where_the_issue_puts_them():
    assert [(n, w) for n, w, _, _ in _edge_lengths()] == [(4350, False), (5121, False), (8890, False), (8906, False),
                                                          (8907, False), (2892, True), (5930, True)]


def _check_fold_and_prefix(gpu, inp, what):
    """tls_debug_folded against the mergesort order and tls_debug_prefix against numpy.cumsum, bit for bit."""
    periods, n = inp["selected"], len(inp["t"])
    gpu.prepare(*_args(inp))
    got = gpu.folded(len(periods), n)
    C = gpu.prefix_sums(len(periods))
    W = C.shape[1] - 1 - n
    assert W == pe.shape(inp)[1] - n
    for k, period in enumerate(periods):
        f = _folded_reference(inp["t"], inp["y"], period)
        numpy.testing.assert_array_equal(got[k], f, err_msg="fold, %s period %r" % (what, period))
        numpy.testing.assert_array_equal(C[k], numpy.cumsum(numpy.insert(numpy.append(f, f[:W]), 0, 0)),
                                         err_msg="prefix sum, %s period %r" % (what, period))


def _parity(gpu, oracle_lib, inp, kernel, what):
    counted = gpu.search(*_args(inp), count_work=True)
    assert gpu.last_kernel() == kernel, (what, gpu.last_kernel())
    want = oracle_search(oracle_lib, inp, periods=inp["selected"])
    assert_parity(counted, want, len(inp["t"]))
    assert counted[3]["grid_cells"] == int(want[3][0]), what
    assert counted[3]["evaluated_cells"] == int(want[3][1]), what
    assert counted[3]["inner_steps"] == int(want[3][2]), what
    print("%s %s: device off the oracle %.2e" % (what, kernel, float(numpy.max(numpy.abs(counted[0] - want[0]) / want[0]))))


@pytest.mark.parametrize("offset", [1325.0, JD])
@pytest.mark.parametrize("index", range(7))
def test_family_edges_against_the_oracle(gpu, oracle_lib, index, offset):
    n, weighted, kernel, slots = _edge_lengths()[index]
    inp = S.case("gapped", offset, "down_R1000" if weighted else "none", N_PERIODS_EDGE, n)
    assert pe.expected_plan(*pe.shape(inp), uniform=not weighted) == (kernel, slots)
    if kernel == "resident":
        gpu.set_options(prune=0, screen32=0)               # (the plain variant, whatever the noise level suggests)
    _parity(gpu, oracle_lib, inp, kernel, (n, offset))
    if offset == JD and kernel != "slim":
        # (the two debug entries run the classic or the slab kernel's sort: the four-slot kernel's own is pinned by (a))
        sorts = (None, 0) if kernel.startswith("slab") else (None,)     # the two-level slab sort and the general bucket sort
        for sort2 in sorts:
            gpu.set_options(sort2=sort2)
            _check_fold_and_prefix(gpu, inp, (n, kernel, "sort2", sort2))
            if sort2 is not None:
                _parity(gpu, oracle_lib, inp, kernel, (n, offset, "sort2", sort2))


def _shuffled_with_duplicates(n, weighted):
    """A gapped series at JD 2457000, shuffled, with runs of equal time stamps and stamps one resolution step apart."""
    inp = S.case("gapped", JD, "down_R1000" if weighted else "none", N_PERIODS_EDGE, n)
    rng = numpy.random.RandomState(n)
    order = rng.permutation(n)
    t, y = inp["t"][order].copy(), inp["y"][order]
    dy = S.make_dy(n, "down", 1e3)[order] if weighted else None
    t[100:110] = t[100]
    t[n // 2] = t[77]
    t[300:306] = t[300] + numpy.arange(6)[::-1] * numpy.spacing(JD)      # neighbours of the double grid, stored descending
    out = S.synthetic.search_inputs(t, y, dy)
    out["selected"] = S.pick_periods(out["periods"], N_PERIODS_EDGE)
    return out


@pytest.mark.parametrize("n,weighted,kernel", [(2900, False, "slim"), (2891, True, "resident"), (8890, False, "resident"),
                                               (8906, False, "slab+split"), (5930, True, "slab")])
def test_duplicated_and_shuffled_time_stamps_at_jd(gpu, oracle_lib, n, weighted, kernel):
    inp = _shuffled_with_duplicates(n, weighted)
    assert len(numpy.unique(inp["t"])) < n and (numpy.diff(inp["t"]) < 0).any()
    if kernel == "resident":
        gpu.set_options(prune=0, screen32=0)
    _parity(gpu, oracle_lib, inp, kernel, ("shuffled", n))
    if kernel != "slim":
        for sort2 in ((None, 0) if kernel.startswith("slab") else (None,)):
            gpu.set_options(sort2=sort2)
            _check_fold_and_prefix(gpu, inp, ("shuffled", n, "sort2", sort2))


# ---- (c) the chain ----------------------------------------------------------------------------------------------------------

def test_power_at_jd_equals_power_with_the_oracles_search(monkeypatch, oracle_lib):
    """test_gpu_power.test_power_gpu_equals_power_with_oracle_search's pattern at offset 2457000, key for key: with
    uniform weights and with the "both, R = 1e3" dy."""
    import pins
    import tls_amd
    from tls_amd import transit_model
    rng = numpy.random.RandomState(3)
    n = 1440
    t = JD + numpy.linspace(2.0, 32.0, n)
    y = transit_model.light_curve(t, JD + 2.5, 3.3, 0.05, 12, 89.8, 0, 90, [0.4, 0.3], "quadratic") + rng.normal(0, 3e-4, n)
    kwargs = dict(period_min=1.0, period_max=10.0, oversampling_factor=2, T0_fit_margin=0.01, verbose=False,
                  show_progress_bar=False)
    for dy in (None, S.make_dy(n, "both", 1e3) * (3e-4 / S.SIGMA)):
        with warnings.catch_warnings(), monkeypatch.context() as m:
            warnings.simplefilter("ignore")
            got = tls_amd.transitleastsquares(t, y, dy, verbose=False).power(**kwargs)

            def oracle_search_periods(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                      M_star_min, M_star_max, T0_fit_margin, **_unused):
                return oracle_lib.search(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                         M_star_min, M_star_max, T0_fit_margin)[:3]

            m.setattr(tls_amd.search, "spectra", lambda chi2_, osf_, **kw: oracle_lib.spectra(chi2_, int(osf_ * 30)))
            m.setattr(tls_amd.search, "search_periods", oracle_search_periods)
            m.setattr(tls_amd.search, "t0_fit_residuals",
                      lambda t_, y_, p_, s_, e_, r_, **kw: oracle_lib.t0_residuals(t_, y_, p_, s_, e_, r_))
            want = tls_amd.transitleastsquares(t, y, dy, verbose=False).power(**kwargs)
        assert list(got.keys()) == list(want.keys())
        if dy is None:                 # (five points of a thousand times the weight carry the other search: no planet there)
            assert abs(got.period - 3.3) < 0.02 and got.SDE > 10
        for key in pins.SCALARS:
            numpy.testing.assert_allclose(float(got[key]), float(want[key]), rtol=1e-9, atol=1e-12, err_msg=key)
        for key in pins.ARRAYS:
            atol = 2e-9 if key in ("power", "power_raw", "SR") else 1e-11     # (as the pattern: SR's spread is 1e-3)
            numpy.testing.assert_allclose(numpy.asarray(got[key], dtype=float), numpy.asarray(want[key], dtype=float),
                                          rtol=1e-9, atol=atol, err_msg=key)
        assert int(numpy.argmin(got.chi2)) == int(numpy.argmin(want.chi2))


def test_t0_fit_at_jd_returns_the_general_kernels_fit(gpu, oracle_lib):
    """The final T0 fit of the rotation tests' first input (config 2, its full epoch count), which takes the rotation path at
    offset 0, and an unevenly sampled one: at offset 2457000 -- time stamps on a grid of 4.7e-10 d, where the path's gap
    bound 6e-15 (Q + 2) reckons with well-separated computed phases and may hand a fit back to the general kernel -- the fit is
    the general kernel's whichever path it took: the same first-minimum epoch, so T0 bit for bit, every residual within the
    distance of a sum taken in another order (1e-13, as test_t0_fit_rotation_path_equals_the_general_kernel holds it; a fit
    handed back has the general kernel's bits throughout -- printed: both inputs kept the rotation path at both offsets), and
    the oracle's residuals to 1e-12."""
    t, f, kw = S.synthetic.config("k2_90d")
    inp = S.synthetic.search_inputs(t, f, **kw)
    signal = 1 - (1 - inp["rows"][len(inp["rows"]) // 3]) * 0.002
    period = 10.12452
    roll = int(len(signal) / 2) + 1
    points = min(len(t), int(len(t) / (0.01 * len(signal))))
    uneven = numpy.sort(5.0 + numpy.random.RandomState(11).uniform(0, 40.0, 3000))
    cases = [("k2_90d", inp["t"], inp["y"], period, signal, points),
             ("uneven", uneven, 1 + numpy.random.RandomState(12).normal(0, 3e-4, 3000), 2.7183,
              numpy.linspace(0.9990, 0.9996, 41), 3000)]
    for name, t0, y, P, sig, n_epochs in cases:
        for offset in (0.0, JD):
            tt = t0 + offset
            epochs = numpy.linspace(tt.min(), tt.min() + P, n_epochs)
            r = int(len(sig) / 2) + 1
            gpu.set_options(t0_rot=None)
            got = gpu.t0_fit_residuals(tt, y, P, sig, epochs, r)
            gpu.set_options(t0_rot=0)
            want = gpu.t0_fit_residuals(tt, y, P, sig, epochs, r)
            gpu.set_options(t0_rot=None)
            print("T0 fit %s at offset %g: %d epochs, residuals %s the general kernel's, largest distance %.1e"
                  % (name, offset, n_epochs, "bit-equal to" if got.tobytes() == want.tobytes() else "not the bits of",
                     float(numpy.max(numpy.abs(got - want) / want))))
            assert int(numpy.argmin(got)) == int(numpy.argmin(want)), (name, offset)
            assert epochs[int(numpy.argmin(got))].tobytes() == epochs[int(numpy.argmin(want))].tobytes()
            numpy.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg="%s %g" % (name, offset))
            ref = oracle_lib.t0_residuals(tt, y, P, sig, epochs, r)
            numpy.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg="%s %g" % (name, offset))
            assert int(numpy.argmin(got)) == int(numpy.argmin(ref)), (name, offset)


def _survey_batch(n_curves, seed=11):
    """Curves over shared time stamps at JD 2457000 (30 d, 720 points, a data gap), each with its own planet; one flat."""
    from tls_amd import transit_model
    rel = numpy.linspace(3.0, 33.0, 720)
    rel = rel[(rel < 14.0) | (rel > 18.5)]
    t = JD + rel
    rng = numpy.random.RandomState(seed)
    fluxes = []
    for s in range(n_curves):
        per = float(rng.uniform(1.6, 6.0))
        f = transit_model.light_curve(t, JD + 3.2 + rng.uniform(0, 1), per, float(rng.uniform(0.03, 0.08)), 12, 89.8, 0, 90,
                                      [0.4, 0.3], "quadratic") + rng.normal(0, 4e-4, len(t))
        if s == 5:
            f = numpy.ones(len(t))
            f[::7] += 1e-7
        fluxes.append(f)
    return t, numpy.array(fluxes)


@pytest.mark.parametrize("weights", [False, True])
def test_power_batch_at_jd_equals_power_per_curve(oracle_lib, weights):
    """power_batch(statistics=True, peaks=3, peak_fits=True) on 33 curves (a launch group and one) at offset 2457000: T0,
    period and every statistics field equal power()'s of the curve on its own, NaN for NaN; the first peak is the pick where
    its two indices agree; and the peak fits of curves in both groups equal tests/peak_fits_spec.py."""
    import peak_fits_spec
    import tls_amd
    from test_power_batch_statistics import RESULT_OF
    from tls_amd import _lib, survey
    ctx = _lib.Context(0)
    try:
        t, fluxes = _survey_batch(33)
        dy_batch = numpy.array([S.make_dy(len(t), "both", 1e3, seed=s) for s in range(33)]) if weights else None
        kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            summary, periods, chi2, row, depth, power, pk = survey.power_batch(
                t, fluxes, dy_batch, context=ctx, statistics=True, peaks=3, peak_fits=True, with_arrays=True, **kw)
            assert len(summary) == 33 and summary["no_fit"][5] == 1 and summary["no_fit"].sum() <= 3
            for s in range(33):
                one = tls_amd.transitleastsquares(t, fluxes[s], None if dy_batch is None else dy_batch[s], verbose=False).power(
                    context=ctx, verbose=False, show_progress_bar=False, **kw)
                rec = summary[s]
                numpy.testing.assert_array_equal(chi2[s], one.chi2, err_msg="curve %d" % s)
                for got, want, name in ((rec["T0"], one.T0, "T0"), (rec["period"], one.period, "period")):
                    numpy.testing.assert_array_equal(float(got), float(want), err_msg="curve %d: %s" % (s, name))
                for field, (key, i) in RESULT_OF.items():
                    want = one[key] if i is None else one[key][i]
                    numpy.testing.assert_array_equal(float(rec[field]), float(want), err_msg="curve %d: %s" % (s, field))
            inp, y_rows, _ = survey._batch_inputs(t, fluxes, dy_batch, dict(kw))
        peaks, n_peaks = pk["peaks"], pk["n_peaks"]
        same = numpy.flatnonzero((summary["index_best"] == summary["index_power"]) & (summary["no_fit"] == 0))
        assert len(same) >= 8
        for c in same:
            assert peaks["index"][c, 0] == summary["index_power"][c] and peaks["status"][c, 0] == 0
            for k in ("T0", "rp_rs") + _lib.TRANSIT_STATS_FIELDS:
                numpy.testing.assert_array_equal(float(peaks[k][c, 0]), float(summary[k][c]), err_msg=str((c, k)))
        fitted = 0
        for c in (0, 5, 31, 32):
            for r in range(3):
                want = peak_fits_spec.expected(ctx, inp, y_rows[c], peaks[c, r], r, int(n_peaks[c]), power[c])
                for k, v in want.items():
                    numpy.testing.assert_array_equal(float(peaks[k][c, r]), float(v), err_msg=str((c, r, k)))
                fitted += want["status"] == peak_fits_spec.FITTED
        assert fitted >= 6
    finally:
        ctx.close()


# ---- (d) the survey stages ---------------------------------------------------------------------------------------------------
# One compact case a stage at offset 2457000 through the comparison its own module makes with its spec (every field bit for
# bit; the six GLS sums inside the spec's a-priori bound), on time stamps that are NOT exact in binary -- the per-stage
# modules keep to multiples of 1/64 d so that every time difference is exact -- with a gap, and the "both, R = 1e3" dy where
# the call takes one.

def _stage_times(n=1920, days=40.0):
    rel = numpy.linspace(3.0, 3.0 + days, n)
    return JD + rel[(rel < 9.0) | (rel > 10.7)]


def _stage_dy(t, n_curves, sigma=1e-3):
    return numpy.array([S.make_dy(len(t), "both", 1e3, seed=40 + c) for c in range(n_curves)]) * (sigma / S.SIGMA)


def _span_max(t, widths, gap_tolerance=0.5):
    dt = float(numpy.median(numpy.diff(t)))
    return [(int(L) - 1) * dt * (1 + gap_tolerance) for L in widths]


def test_phase_scan_at_jd(gpu):
    import test_phase_scan as m
    t = _stage_times()
    period, T0 = numpy.array([2.0, 3.1, 1.7]), JD + numpy.array([3.3, 4.0, 3.9])
    y = numpy.array([m.noisy(t, s, P=period[s], T0=T0[s]) for s in range(3)])
    got = m.check(gpu, t, y, period, T0, numpy.array([0.1, 0.12, 0.05]), label="phase scan at JD")
    assert (got["scan_status"] == 0).all() and (got["primary_depth"] > 5e-4).all() and (got["n_windows"] >= 8).all()


def test_transit_times_at_jd(gpu):
    import test_transit_times as m
    t = _stage_times()
    widths = [3, 5, 8, 37]
    period, T0 = numpy.array([2.3, 3.1, 4.7]), JD + numpy.array([3.4, 4.0, 5.1])
    rows = numpy.array([1, 2, 3])
    y = numpy.array([m.dips(t, period[s], T0[s], widths[rows[s]], seed=s) for s in range(3)])
    eph, times = m.check(gpu, t, y, _stage_dy(t, 3), period, T0, rows, numpy.array([2, 3, 6]), widths=widths,
                         span_max=_span_max(t, widths), min_ses=0.0, label="transit times at JD")
    assert (eph["n_epochs"] >= 4).all() and (eph["n_timed"] >= 2).all()


def test_shape_fit_at_jd(gpu):
    import test_shape_fit as m
    t = _stage_times()
    period, T0, T14 = numpy.array([2.3, 3.1, 4.7]), JD + numpy.array([3.4, 4.0, 5.1]), numpy.array([0.2, 0.3, 0.25])
    y = numpy.array([m.dips(t, period[s], T0[s], T14[s], seed=s) for s in range(3)])
    got = m.check(gpu, t, y, _stage_dy(t, 3), period, T0, T14, label="shape fit at JD")
    assert (got["status"] == 0).all()


def test_folded_views_at_jd(gpu):
    import test_folded_views as m
    import test_shape_fit as shapes
    t = _stage_times()
    period, T0, T14 = numpy.array([2.3, 3.1, 4.7]), JD + numpy.array([3.4, 4.0, 5.1]), numpy.array([0.2, 0.3, 0.25])
    y = numpy.array([shapes.dips(t, period[s], T0[s], T14[s], seed=s) for s in range(3)])
    records, views = m.check(gpu, t, y, period, T0, T14, phi=numpy.array([0.5, 0.37, numpy.nan]), label="views at JD",
                             n_global=201, n_local=61)
    assert (records["status"] == 0).all()


def test_single_transits_at_jd(gpu):
    import test_single_transit as m
    t = _stage_times()
    widths = [3, 4, 5, 8, 37, 64, 65]
    y = m.curves(len(t), 3, seed=7)
    got = m.check(gpu, t, y, _stage_dy(t, 3), widths, label="single transits at JD")
    assert (got[1] >= 1).all()


def test_biweight_at_jd(gpu):
    import test_biweight as m
    t = _stage_times(1920, 40.0)
    rng = numpy.random.RandomState(8)
    m._check(gpu, t, m._rows(len(t), rng)[:5], 0.5)
    m._check(gpu, t, m._rows(len(t), rng)[:2], 1.3, break_tolerance=0.3)


@pytest.mark.parametrize("with_dy", [False, True])
def test_lomb_scargle_and_sine_test_at_jd(gpu, with_dy):
    import test_gls as m
    from tls_amd import survey
    t = _stage_times()
    y, _ = m.curves(t, 3, seed=3)
    dy = _stage_dy(t, 3, 3e-4) if with_dy else None
    f = survey.variability_frequencies(t, oversampling=1, f_max=6.0)
    got = m.check_periodogram(gpu, t, y, dy, f, ("periodogram at JD", with_dy))
    assert numpy.isfinite(got["power"]).all()
    sine, _ = m.check_sine(gpu, t, y, dy, numpy.array([1.1, 0.7, 3.0, 2.2]), T0=JD + numpy.array([3.3, 3.5, 4.0, 3.1]),
                           duration=numpy.array([0.1, 0.08, 0.2, 0.15]), curve=numpy.array([2, 0, 1, 0]),
                           label=("sine test at JD", with_dy))
    assert (sine["status"] == 0).all() and (sine["n_used"] < len(t)).all()


def test_sysrem_with_wide_range_dy(gpu):
    import test_sysrem as m
    rng = numpy.random.RandomState(9)
    y = m._rows(5, 900, rng)
    dy = m._errors(y, rng)
    for c in range(len(y)):                                   # five points a row R times more precise, fifteen de-weighted
        idx = rng.choice(y.shape[1], S.N_PRECISE + S.N_DOWN, replace=False)
        dy[c, idx[:S.N_PRECISE]] /= 1e3
        dy[c, idx[S.N_PRECISE:]] *= 1e3
    m._check(gpu, y, 2, dy=dy)


def test_inject_transits_at_jd(gpu):
    import test_injection_recovery as m
    from tls_amd import survey
    t = _stage_times(1920, 40.0)
    rng = numpy.random.RandomState(len(t))
    base = 1.0 + rng.normal(0.0, 1e-4, len(t))
    for law, u in m.LAWS:
        inj = m.random_injections(rng, t, 5)
        rows, count = gpu.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(u, law, {})[1:])
        assert rows.shape == (5, len(t)) and count.sum() > 0
        m._check_rows("jd", t, base, inj, rows, count, u, law)
