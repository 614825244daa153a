"""Survey-mode power()'s post-search chain on the device (tls_power_batch after the search: spectra, pick, trial epochs and
scaled template, batched final T0 fit, first minimum) against a plain host reference of main.py:198-273 and
stats.py:105-204, curve by curve, at the sizes, group shapes and edges where the chain branches: series in the LDS and in
HBM, fits the rotation path hands back, spectra with and without detrending, T0_fit_margin at its ends, launch groups of
1 to 97 curves, no-fit curves at group edges, one context reused across sizes, and injected search results
(tls_debug_post_search) for the ties and rows no light curve produces on demand.

The reference is fed the chi2 / row / depth the device returned (with_arrays): search parity is tested elsewhere."""
import warnings

import numpy
import pytest

from tls_amd import _lib, synthetic, transit_model
from tls_amd.helpers import running_median

pytestmark = pytest.mark.gpu

# the rotation path of the T0 fit sums a fit's residuals in another order than the reference: a trial epoch whose residual
# is this close to the minimum may be the one picked instead (a near-tie)
T0_TIE_RTOL = 1e-12


def reference_chain(oracle_lib, t, y, periods, chi2, row, depth, rows, margin, median_kernel, with_t0=True):
    """main.py:198-273 with stats.py:105-204 on one curve's search results: dict of the summary fields (+ the T0 fit's
    trial epochs and residuals when with_t0)."""
    kernel = int(median_kernel)
    if kernel % 2 == 0:
        kernel += 1
    with numpy.errstate(invalid="ignore", divide="ignore"):
        SR = numpy.min(chi2) / chi2
        sde_raw = (1 - numpy.mean(SR)) / numpy.std(SR)
        praw = SR - numpy.mean(SR)
        praw = praw * (sde_raw / numpy.max(praw))
        if len(chi2) > 2 * kernel:
            power = praw - running_median(praw, kernel)
            power = power - numpy.mean(power)
            sde = numpy.max(power / numpy.std(power))
            power = power * (sde / numpy.max(power))
        else:
            power, sde = praw, sde_raw
    out = dict(index_best=int(numpy.argmin(chi2)), index_power=int(numpy.argmax(power)), chi2_min=float(numpy.min(chi2)),
               no_fit=int(numpy.max(chi2) == numpy.min(chi2)))
    out["best_row"] = int(row[out["index_best"]])
    if out["no_fit"]:
        out.update(SDE=0.0, SDE_raw=0.0, period=numpy.nan, depth=1.0, T0=0.0, epochs=None)
        return out
    o_SR, o_praw, o_power, o_sde_raw, o_sde = oracle_lib.spectra(chi2, kernel)
    numpy.testing.assert_allclose([sde_raw, sde], [o_sde_raw, o_sde], rtol=1e-9)
    assert int(numpy.argmax(o_power)) == out["index_power"]
    out.update(SDE=float(sde), SDE_raw=float(sde_raw), period=float(periods[out["index_power"]]),
               depth=float(depth[out["index_power"]]), epochs=None)
    if with_t0:
        T0, epochs, res = oracle_lib.final_t0_fit(rows[out["best_row"]], out["depth"], t, y, out["period"], margin)
        out.update(T0=T0, epochs=epochs, residuals=res)
    return out


class Tally(object):
    """Near-ties of T0 seen in the module (reported at the end, asserted rare)."""
    fits = 0
    ties = 0


def check_curve(rec, ref, where, epochs=None, residuals=None):
    for k in ("index_best", "index_power", "best_row", "no_fit"):
        assert int(rec[k]) == ref[k], (where, k, rec[k], ref[k])
    assert rec["chi2_min"] == ref["chi2_min"], where
    if ref["no_fit"]:
        assert rec["SDE"] == 0 and rec["SDE_raw"] == 0 and numpy.isnan(rec["period"]) and rec["depth"] == 1 and rec["T0"] == 0, where
        return
    assert rec["period"] == ref["period"] and rec["depth"] == ref["depth"], where
    numpy.testing.assert_allclose([rec["SDE"], rec["SDE_raw"]], [ref["SDE"], ref["SDE_raw"]], rtol=1e-11, err_msg=str(where))
    if ref["epochs"] is None:
        return
    if epochs is not None:
        # the trial grid bit for bit (numpy.linspace: arange * step + start, the end point set to stop), the residuals to
        # the summation-order bound
        assert epochs.tobytes() == ref["epochs"].tobytes(), (where, len(epochs), len(ref["epochs"]))
        numpy.testing.assert_allclose(residuals, ref["residuals"], rtol=T0_TIE_RTOL, atol=0, err_msg=str(where))
    Tally.fits += 1
    if rec["T0"] == ref["T0"]:
        return
    # a near-tie: the oracle's residual at the device's epoch is within T0_TIE_RTOL of its minimum
    j = numpy.flatnonzero(ref["epochs"] == rec["T0"])
    assert len(j), (where, "T0 is not a trial epoch", rec["T0"], ref["T0"])
    res = ref["residuals"]
    assert res[j[0]] <= numpy.min(res) * (1 + T0_TIE_RTOL), (where, rec["T0"], ref["T0"], res[j[0]], numpy.min(res))
    Tally.ties += 1


def check_batch(oracle_lib, summary, t, y_batch, periods, chi2, row, depth, rows, margin, median_kernel, t0_curves=None,
                label="", fits=None):
    """Every curve of the batch against the reference; the oracle's T0 fit on `t0_curves` (None: all).  fits: the device's
    (epochs, residuals) of every curve (tls_debug_post_search), compared where the oracle's fit ran."""
    refs = []
    for c in range(len(summary)):
        with_t0 = t0_curves is None or c in t0_curves
        ref = reference_chain(oracle_lib, t, y_batch[c], periods, chi2[c], row[c], depth[c], rows, margin, median_kernel,
                              with_t0=with_t0)
        check_curve(summary[c], ref, (label, c), *((fits[0][c], fits[1][c]) if fits else ()))
        refs.append(ref)
    return refs


def shared_curves(t, n_curves, seed, weights=False, flat=(), per_range=(2.0, 7.0), noise=4e-4, periods=None):
    """Light curves on the shared time stamps t: one planet each (period from per_range, or from `periods`), white
    noise; the curves in `flat` have nothing that passes transit_depth_min (a no-fit curve)."""
    rng = numpy.random.RandomState(seed)
    fluxes, dys = [], []
    for s in range(n_curves):
        per = float(rng.uniform(*per_range)) if periods is None else float(periods[s])
        f = transit_model.light_curve(t, t[0] + 0.2 + rng.uniform(0, 1), per, float(rng.uniform(0.03, 0.08)), 12, 89.8, 0,
                                      90, [0.4, 0.3], "quadratic") + rng.normal(0, noise, len(t))
        if s in flat:
            f = numpy.ones(len(t))
            f[::7] += 1e-7
        fluxes.append(f)
        d = rng.uniform(0.8, 1.3, len(t))
        dys.append(d / numpy.mean(d))             # (normalised, as validate.py hands dy to the search)
    return numpy.array(fluxes), (numpy.array(dys) if weights else numpy.tile(numpy.std(fluxes, axis=1)[:, None], len(t)))


def plan(t, flux, dy=None, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return synthetic.search_inputs(t, flux, dy, **kw)


def run_and_check(ctx, oracle_lib, inp, y_batch, dy_batch, median_kernel, periods=None, params=None, t0_curves=None,
                  label=""):
    periods = inp["periods"] if periods is None else periods
    params = inp["params"] if params is None else params
    summary, chi2, row, depth, _ = ctx.power_batch(inp["t"], y_batch, dy_batch, periods, inp["table"], params, median_kernel,
                                                   with_arrays=True)
    # the same chain once more on the arrays it was just fed (the plan is still prepared), every fit's trial grid and
    # residuals returned: the summaries are the same bit for bit
    again, epochs, residuals, handed_back = ctx.debug_post_search(y_batch, chi2, row, depth, median_kernel, with_fits=True)
    assert again.tobytes() == summary.tobytes(), label
    refs = check_batch(oracle_lib, summary, inp["t"], y_batch, periods, chi2, row, depth, inp["rows"],
                       params["T0_fit_margin"], median_kernel, t0_curves=t0_curves, label=label, fits=(epochs, residuals))
    for c, ref in enumerate(refs):
        ref["handed_back"] = int(handed_back[c])
    return summary, refs


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _report_ties():
    yield
    print("\nT0 near-ties: %d of %d fits compared with the oracle" % (Tally.ties, Tally.fits))
    assert Tally.ties * 50 <= Tally.fits, (Tally.ties, Tally.fits)


@pytest.mark.parametrize("n_curves", [1, 31, 32, 33, 97])
@pytest.mark.parametrize("weights", [False, True])
def test_group_shapes(ctx, oracle_lib, n_curves, weights):
    """Launch groups of 32: one curve (the drop-in power()), a partial group, whole groups, the third group reusing the
    first's pinned staging slot; every curve compared, no-fit curves at the first and last position of a group."""
    t = numpy.linspace(3.0, 33.0, 720)
    flat = {c for c in (0, 31, 32, 96) if c < n_curves and n_curves > 1}
    y, dy = shared_curves(t, n_curves, seed=n_curves, weights=weights, flat=flat)
    inp = plan(t, y[min(set(range(n_curves)) - flat)], None, period_min=1.5, period_max=9.0, oversampling_factor=2,
               T0_fit_margin=0.02)
    summary, refs = run_and_check(ctx, oracle_lib, inp, y, dy, 60, label="group %d" % n_curves)
    assert sum(r["no_fit"] for r in refs) == len(flat)


def test_a_whole_group_of_no_fit_curves(ctx, oracle_lib):
    t = numpy.linspace(3.0, 33.0, 720)
    y, dy = shared_curves(t, 70, seed=5, flat=set(range(32, 64)) | {69})
    inp = plan(t, y[0], period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    summary, refs = run_and_check(ctx, oracle_lib, inp, y, dy, 60, label="no-fit group")
    assert [r["no_fit"] for r in refs] == [int(c in range(32, 64) or c == 69) for c in range(70)]


@pytest.mark.parametrize("n", [10223, 10224])
def test_both_sides_of_the_lds_boundary(ctx, oracle_lib, n):
    """N = 10 223 is the largest series the T0 fit keeps in the LDS (272 + 16 N bytes <= 160 KB); 10 224 runs on the HBM
    slabs, the batched fit indexing them by workgroup.  Two groups, uniform and per-point weights."""
    t = numpy.linspace(3.0, 33.0, n)
    y, dy = shared_curves(t, 34, seed=n, per_range=(3.0, 6.0), flat={33}, weights=True)
    for weights in (False, True):
        inp = plan(t, y[0], dy[0] if weights else None, period_min=2.5, period_max=7.0, oversampling_factor=1,
                   T0_fit_margin=0.05)
        w = dy if weights else numpy.tile(numpy.std(y, axis=1)[:, None], n)
        summary, refs = run_and_check(ctx, oracle_lib, inp, y, w, 30, t0_curves={1, 32}, label=(n, weights))
        # (distinct, evenly spaced time stamps: the rotation path keeps every fit -- the batched base sort, one workgroup a
        # fit, each on a slab of its own where the series is in HBM, left nothing to redo)
        assert [r["handed_back"] for r in refs] == [0] * len(refs)


def test_tess_size_batch_and_bounded_t0_fit_scratch(ctx, oracle_lib):
    """40 curves at TESS size (N = 19 440) on time stamps with duplicates: every fit is handed back by the rotation path
    and runs the general kernel on HBM slabs.  The T0 fit's scratch no longer grows with the number of fits: at most one
    slab of 3N doubles per workgroup (2 per CU) plus one per fit of the base sort."""
    t, f, kw = synthetic.config("tess_27d")
    n = len(t)
    t = t.copy()
    t[1::2] = t[0::2][: n // 2]           # pairs of equal time stamps
    y, dy = shared_curves(t, 40, seed=7, per_range=(2.0, 5.0), noise=2e-4)
    inp = plan(t, y[0], period_min=2.0, period_max=5.0, oversampling_factor=1, T0_fit_margin=0.1)
    summary, refs = run_and_check(ctx, oracle_lib, inp, y, dy, 30, t0_curves={0, 33}, label="tess duplicates")
    assert [r["handed_back"] for r in refs] == [1] * len(refs)
    n_cu = 256   # MI355X
    assert ctx.device_bytes()[1] <= (2 * n_cu + 32) * 3 * n * 8, ctx.device_bytes()


def test_commensurate_period_for_some_curves_of_a_group(ctx, oracle_lib):
    """30-min cadence; curves 1, 2 and 5 carry a planet of period 78/48 d, which the period list holds exactly: their fits'
    phases fall onto the cadence (a gap the folds' rounding could close), the rotation path hands those fits back to the
    general kernel.  Both the LDS-resident and the HBM series; a margin that keeps the oracle's fit to a few thousand
    epochs."""
    for days in (100.0, 400.0):           # N = 4 800 and 19 200
        t = 3.0 + numpy.arange(int(days * 48)) / 48.0
        pers = [3.3, 78 / 48.0, 78 / 48.0, 4.1, 2.7, 78 / 48.0, 3.7, 2.2]
        y, dy = shared_curves(t, len(pers), seed=int(days), periods=pers, noise=2e-4)
        inp = plan(t, y[0], period_min=1.5, period_max=4.5, oversampling_factor=1, T0_fit_margin=0.1)
        periods = numpy.sort(numpy.append(inp["periods"][::8], 78 / 48.0))
        params = dict(inp["params"], T0_fit_margin=2.0)
        summary, refs = run_and_check(ctx, oracle_lib, inp, y, dy, 30, periods=periods, params=params,
                                      t0_curves={0, 1, 5} if days < 200 else {1}, label=("commensurate", days))
        assert all(summary[c]["period"] == 78 / 48.0 for c in (1, 2, 5)), summary["period"]
        assert [r["handed_back"] for r in refs] == [int(c in (1, 2, 5)) for c in range(len(pers))]


@pytest.mark.parametrize("osf,extra", [(0.5, 0), (0.5, 1), (2, 0), (2, 1), (5, 0), (5, 1)])
def test_spectra_branches(ctx, oracle_lib, osf, extra):
    """n_periods = 2k (no detrending) and 2k + 1 (the running median) for the kernels of oversampling_factor 0.5 (15: odd
    without the +1), 2 (60 -> 61) and 5 (150 -> 151)."""
    t = numpy.linspace(3.0, 33.0, 720)
    y, dy = shared_curves(t, 5, seed=int(osf * 10) + extra, flat={4})
    inp = plan(t, y[0], period_min=1.5, period_max=9.0, oversampling_factor=osf, T0_fit_margin=0.02)
    kernel = int(osf * 30)
    k = kernel + 1 if kernel % 2 == 0 else kernel
    periods = numpy.linspace(1.5, 9.0, 2 * k + extra)
    run_and_check(ctx, oracle_lib, inp, y, dy, kernel, periods=periods, label=("spectra", osf, extra))


@pytest.mark.parametrize("margin", [0, 0.001, 0.1])
def test_t0_fit_margin_of_power(ctx, oracle_lib, margin):
    """T0_fit_margin as power() takes it (validate clamps to [0, 0.1]): 0 is N trial epochs a fit."""
    t = numpy.linspace(3.0, 33.0, 720)
    y, dy = shared_curves(t, 6, seed=17, weights=True)
    inp = plan(t, y[0], dy[0], period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=margin)
    assert inp["params"]["T0_fit_margin"] == margin
    run_and_check(ctx, oracle_lib, inp, y, dy, 60, label=("margin", margin))


def test_t0_fit_of_one_and_of_no_epoch(ctx, oracle_lib):
    """Through the C ABI a margin may exceed 0.1: chosen so that points = int(N / (margin * dur)) is exactly 1 (the
    trial grid is [min t]) and exactly 0 (no trial epoch: T0 = 0)."""
    t = numpy.linspace(3.0, 33.0, 720)
    y, dy = shared_curves(t, 3, seed=23)
    inp = plan(t, y[0], period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    summary, _ = run_and_check(ctx, oracle_lib, inp, y, dy, 60, label="margin probe")
    dur = len(inp["rows"][summary[0]["best_row"]])
    for points, margin in ((1, len(t) / (1.5 * dur)), (0, 2.0 * len(t) / dur)):
        params = dict(inp["params"], T0_fit_margin=margin)
        summary, refs = run_and_check(ctx, oracle_lib, inp, y, dy, 60, params=params, label=("points", points))
        assert len(refs[0]["epochs"]) == points
        assert summary[0]["T0"] == (t.min() if points == 1 else 0.0)


def test_kepler_size_group(ctx, oracle_lib):
    """N = 70 128 (BASELINE config 3's time stamps) with a few dozen periods: HBM slabs, the largest series."""
    t, f, kw = synthetic.config("kepler_4yr")
    y, dy = shared_curves(t, 3, seed=3, per_range=(9.8, 10.4), noise=5e-5)
    inp = plan(t, y[0], period_min=9.9, period_max=10.3, oversampling_factor=1, T0_fit_margin=0.1)
    periods = inp["periods"][:: max(1, len(inp["periods"]) // 40)]
    summary, chi2, row, depth, _ = ctx.power_batch(inp["t"], y, dy, periods, inp["table"], inp["params"], 30,
                                                   with_arrays=True)
    # (the oracle's T0 fit sorts N points per trial epoch: a margin that keeps a few hundred epochs)
    dur = len(inp["rows"][summary[0]["best_row"]])
    params = dict(inp["params"], T0_fit_margin=len(t) / (300.0 * dur))
    run_and_check(ctx, oracle_lib, inp, y, dy, 30, periods=periods, params=params, t0_curves={0}, label="kepler")


def test_one_context_across_sizes_equals_fresh_contexts(ctx, oracle_lib):
    """720, then 19 440, then 720 again on one context (plan, slots and DevBufs carried over, grown and reused): bit-equal
    to a fresh context each time."""
    cases = []
    for days, cadence in ((30.0, 24), (27.0, 720), (30.0, 24)):
        n = int(days * cadence)
        t = numpy.linspace(3.0, 3.0 + days, n)
        y, dy = shared_curves(t, 3, seed=n, per_range=(2.0, 5.0), noise=2e-4)
        inp = plan(t, y[0], period_min=2.0, period_max=5.0, oversampling_factor=1, T0_fit_margin=0.05)
        cases.append((inp, y, dy))
    reused = [ctx.power_batch(inp["t"], y, dy, inp["periods"], inp["table"], inp["params"], 30)[0] for inp, y, dy in cases]
    for (inp, y, dy), got in zip(cases, reused):
        fresh = _lib.Context(0)
        want = fresh.power_batch(inp["t"], y, dy, inp["periods"], inp["table"], inp["params"], 30)[0]
        fresh.close()
        assert got.tobytes() == want.tobytes()


def reported_rows(table):
    first = {}
    for r, w in enumerate(table.width):
        first.setdefault(int(w), r)
    return sorted(first.values())


def test_injected_search_results(ctx, oracle_lib):
    """tls_debug_post_search runs the chain tls_power_batch runs on chi2 / row / depth the test writes: exact ties at the
    chi2 minimum and at the power maximum, constant chi2 in some curves, the power peak away from the chi2 minimum
    (period and depth from one index, the template from the other), rows of every duration."""
    t = numpy.linspace(3.0, 33.0, 720)
    y, dy = shared_curves(t, 8, seed=31)
    inp = plan(t, y[0], period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    ctx.prepare(inp["t"], y[0], dy[0], inp["periods"], inp["table"], inp["params"])
    n_p = len(inp["periods"])
    good = reported_rows(inp["table"])
    rng = numpy.random.RandomState(2)
    chi2 = 700 + rng.uniform(0, 1, (8, n_p))
    row = numpy.array([rng.choice(good, n_p) for _ in range(8)], dtype=numpy.int64)
    depth = 1 - rng.uniform(1e-4, 3e-3, (8, n_p))
    chi2[0, [40, 90]] = 600.0                    # exact tie at the minimum (and, undetrended, at the power peak)
    chi2[1, :] = 650.0                           # constant: no fit
    i0, i1 = n_p // 3, 2 * n_p // 3              # a broad dip holds the minimum, a sharp one the power peak
    chi2[2] = 700 + 0.01 * rng.uniform(0, 1, n_p)
    chi2[2, i0 - 150:i0 + 150] -= 40 * numpy.hanning(300)
    chi2[2, i1] = chi2[2, i0] + 2.0
    chi2[3] = chi2[0]                            # the tie again, rows of the widest and narrowest duration
    row[3, 40], row[3, 90] = good[-1], good[0]
    chi2[4, ::2] = 640.0                         # many equal minima
    chi2[5] = chi2[2][::-1]
    for kernel, undetrended in ((60, False), (n_p, True)):
        summary = ctx.debug_post_search(y, chi2, row, depth, kernel)
        refs = check_batch(oracle_lib, summary, inp["t"], y, inp["periods"], chi2, row, depth, inp["rows"],
                           inp["params"]["T0_fit_margin"], kernel, label=("injected", kernel))
        assert refs[1]["no_fit"] and refs[0]["index_best"] == 40 and refs[4]["index_best"] == 0
        assert summary[3]["best_row"] == good[-1]
        if undetrended:
            assert refs[0]["index_power"] == 40
        else:
            assert refs[2]["index_power"] != refs[2]["index_best"] and refs[5]["index_power"] != refs[5]["index_best"]
    # on the arrays of a real search this entry gives what tls_power_batch gave
    s2, c2, r2, d2, _ = ctx.power_batch(inp["t"], y, dy, inp["periods"], inp["table"], inp["params"], 60, with_arrays=True)
    ctx.prepare(inp["t"], y[0], dy[0], inp["periods"], inp["table"], inp["params"])
    assert ctx.debug_post_search(y, c2, r2, d2, 60).tobytes() == s2.tobytes()


def test_injected_row_that_starts_no_duration_is_an_error(ctx):
    t = numpy.linspace(3.0, 33.0, 720)
    y, dy = shared_curves(t, 2, seed=37)
    inp = plan(t, y[0], period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    table = inp["table"]
    good = reported_rows(table)
    bad = [r for r in range(len(table.width)) if r not in good] + [-1, len(table.width)]
    ctx.prepare(inp["t"], y[0], dy[0], inp["periods"], table, inp["params"])
    n_p = len(inp["periods"])
    chi2 = 700 + numpy.random.RandomState(1).uniform(0, 1, (2, n_p))
    depth = numpy.full((2, n_p), 0.999)
    for b in bad:
        row = numpy.full((2, n_p), good[0], dtype=numpy.int64)
        row[1, int(numpy.argmin(chi2[1]))] = b
        with pytest.raises(RuntimeError, match="not the first row"):
            ctx.debug_post_search(y, chi2, row, depth, 60)
    # (a row away from the minimum is never read)
    row = numpy.full((2, n_p), good[0], dtype=numpy.int64)
    row[1, int(numpy.argmax(chi2[1]))] = bad[0]
    ctx.debug_post_search(y, chi2, row, depth, 60)
