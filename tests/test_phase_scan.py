"""The phase scan on the device (survey.phase_scan / tls_phase_scan; power_batch(peaks=K, peak_fits=True, phase_scan=True) /
tls_power_batch_phase_scan) against tests/phase_scan_spec.py bit for bit: the standalone entry at the edges of the statement
(bin counts, bin edges, the clamp, empty bins, ties, bad candidates) and of the kernel (its LDS chunk, its 256 bins a step),
and the pipeline at the slab and group edges of the peak-fit stage, with every other result untouched."""
import ctypes
import warnings

import numpy
import pytest

import phase_scan_spec as spec
from tls_amd import _lib, survey, transit_model
from tls_amd.stats import calculate_fill_factor

pytestmark = pytest.mark.gpu

# the light curves and keywords of tests/test_peak_fits.py
T = numpy.linspace(3.0, 43.0, 1920)          # 40 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))          # period [d], a / R_star
CHUNK = _lib.PHASE_SCAN_CHUNK


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def curve(s):
    rng = numpy.random.RandomState(1000 + s)
    f = numpy.ones(len(T))
    for per, a in PLANETS:
        tp = T[0] + rng.uniform(0.1, 0.9) * per
        f += transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3], "quadratic") - 1
    return f + rng.normal(0, 4e-4, len(T))


def batch(n_curves):
    return numpy.array([curve(s) for s in range(n_curves)])


@pytest.fixture(scope="module")
def shared():
    """The plan every batch of this module gets and the flux rows as the device sees them."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, _ = survey._batch_inputs(T, batch(33), None, dict(KW))
    return dict(inp=inp, y=y_rows)


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check(ctx, t, y, period, T0, duration, curve=None, label="", **kw):
    """survey.phase_scan of the candidates equals the statement, field by field; the device's records."""
    got = survey.phase_scan(t, y, period, T0, duration, curve=curve, context=ctx, **kw)
    rows = numpy.atleast_2d(y)
    period, T0, duration = (numpy.atleast_1d(numpy.asarray(a, dtype=float)) for a in (period, T0, duration))
    which = numpy.arange(len(period)) if curve is None else numpy.asarray(curve)
    assert got.shape == period.shape and got.dtype.names == survey.phase_scan_fields()
    for f in range(len(period)):
        want = spec.expected(t, rows[which[f]], period[f], T0[f], duration[f], **kw)
        for k in got.dtype.names:
            expect_equal(got[k][f], want["status" if k == "scan_status" else k], (label, f, k))
    return got


def noisy(t, seed, P=2.0, T0=3.3, depth=2e-3):
    """Noise and a box of `depth` at phase 0, another of half the depth at phase 0.4."""
    rng = numpy.random.RandomState(seed)
    phase = ((t - T0) / P) % 1.0
    y = 1 + rng.normal(0, 3e-4, len(t))
    y[(phase < 0.01) | (phase > 0.99)] -= depth
    y[abs(phase - 0.4) < 0.01] -= 0.5 * depth
    return y


def test_bin_counts(ctx):
    """B = 15 (nothing to scan), 16 (q exact and not), 255, 256 and 257 (the window pass takes 256 windows a step), 4096, and
    requests beyond the cap, the default's and a caller's; min_count 1 where three points a window are rare."""
    y = noisy(T, 1)
    P = 2.0
    q = numpy.array([15.5, 16.0, 16.5, 255.5, 256.5, 257.5, 511.5, 513.5, 4095.5, 4096.5, 10000.3])
    got = check(ctx, T, y, numpy.full(len(q), P), numpy.full(len(q), 3.3), 2.0 * P / q, curve=numpy.zeros(len(q), dtype=int),
                label="bins")
    expect_equal(got["scan_status"], [1] + [0] * 10, "status")
    expect_equal(got["n_bins"][1:], [16, 16, 255, 256, 257, 511, 513, 4095, 4096, 4096], "n_bins")
    assert (got["n_windows"][3:8] >= 8).all() and numpy.isfinite(got["scan_std"][3:8]).all()      # (16 bins: 11 windows, at most 8 left)
    got = check(ctx, T, y, numpy.full(len(q), P), numpy.full(len(q), 3.3), 2.0 * P / q, curve=numpy.zeros(len(q), dtype=int),
                label="bins, min_count 1", min_count=1)
    assert (got["n_windows"][3:] >= 8).all() and numpy.isfinite(got["scan_std"][3:]).all()
    got = check(ctx, T, y, numpy.full(4, P), numpy.full(4, 3.3), 2.0 * P / numpy.array([99.5, 100.5, 257.5, 4000.0]),
                curve=[0, 0, 0, 0], label="cap 100", max_bins=100)
    expect_equal(got["n_bins"], [99, 100, 100, 100], "cap")
    got = check(ctx, T, y, [P] * 3, [3.3] * 3, 2.0 * P / numpy.array([15.9, 16.2, 300.0]), curve=[0, 0, 0], max_bins=16)
    expect_equal(got["n_bins"], [numpy.nan, 16, 16], "cap 16")


def test_bin_edges_hit_exactly(ctx):
    """P = 2, T0 = 0.5, t = k / 64, d = 0.125: 32 bins, every phase * B an integer or an exact quarter; and the same time
    stamps all below T0 (negative x, floor below zero)."""
    t = numpy.arange(1280) / 64.0
    y = noisy(t, 2, T0=0.5)
    got = check(ctx, t, y, [2.0, 2.0, 2.0], [0.5, 50.0, 20.0 - 1 / 128], [0.125] * 3, curve=[0, 0, 0], label="edges")
    expect_equal(got["n_bins"], [32, 32, 32], "B")
    assert (spec.bins(t, 2.0, 0.5, 32) * 4 == ((t - 0.5) / 2.0 % 1.0) * 128).sum() == 320     # (a quarter of the points on an edge)
    assert (got["primary_count"] == 80).all()


def test_the_clamp(ctx):
    """x = -5e-21: phi = x - floor(x) rounds to 1.0, and the point belongs to the last bin."""
    t = numpy.concatenate([[-1e-20], numpy.arange(1, 1280) / 64.0])
    assert (t[0] - 0.0) / 2.0 == -5e-21 and (t[0] / 2.0) - numpy.floor(t[0] / 2.0) == 1.0
    y = noisy(t, 3, T0=0.0)
    y[0] = 0.5                                   # (the clamped point weighs on its bin)
    got = check(ctx, t, y, [2.0], [0.0], [0.125], label="clamp")
    assert spec.bins(t, 2.0, 0.0, 32)[0] == 31 and got["primary_count"][0] == 80
    without = check(ctx, t[1:], y[1:], [2.0], [0.0], [0.125], label="clamp, without the point")
    assert without["primary_count"][0] == 79 and without["primary_depth"][0] != got["primary_depth"][0]


def test_gaps_and_empty_bins(ctx):
    """Phases without a point: empty bins, windows below min_count (NaN depths inside the scan), an empty primary window;
    and a curve of twenty points, where no window is valid at all."""
    phase = ((T - 3.3) / 2.0) % 1.0
    keep = ~((phase > 0.30) & (phase < 0.36)) & ~((phase > 0.70) & (phase < 0.705))
    t, y = T[keep], noisy(T, 4)[keep]
    got = check(ctx, t, y, [2.0] * 3, [3.3] * 3, [0.04, 0.01, 0.004], curve=[0, 0, 0], label="gaps")
    for f, d in enumerate((0.04, 0.01, 0.004)):
        rec, delta = spec.scan(t, y, 2.0, 3.3, d, with_delta=True)
        inside = numpy.array(delta[2:int(rec["n_bins"]) - 3])
        assert numpy.isnan(inside).any() and got["n_windows"][f] >= 8, d
    no_primary = keep & ~((phase < 0.02) | (phase > 0.98))
    got = check(ctx, T[no_primary], noisy(T, 4)[no_primary], [2.0], [3.3], [0.04], label="no primary")
    assert got["primary_count"][0] == 0 and numpy.isnan(got["primary_depth"][0]) and numpy.isnan(got["primary_significance"][0])
    assert got["secondary_significance"][0] > 5
    got = check(ctx, T[::96], noisy(T, 5)[::96], [3.1, 3.1], [4.0, 4.0], [0.12, 0.5], curve=[0, 0], label="twenty points")
    expect_equal(got["scan_status"], [0, 1], "status")
    assert got["n_bins"][0] == 51 and got["n_windows"][0] == 0
    for k in ("primary_depth", "secondary_depth", "secondary_phase", "secondary_count", "bump_depth", "bump_phase", "scan_mean", "scan_std"):
        assert numpy.isnan(got[k][0]), k
    # ... and fewer than eight windows away from the deepest: extremes, but no scatter
    got = check(ctx, T, noisy(T, 6), [2.0], [3.3], [0.25], label="sixteen bins", min_count=1)
    assert got["n_bins"][0] == 16 and got["n_windows"][0] < 8 and numpy.isfinite(got["secondary_depth"][0])
    assert numpy.isnan(got["scan_std"][0]) and numpy.isnan(got["secondary_significance"][0])


def test_constant_flux_ties(ctx):
    """Every window's depth is exactly zero: the first window is both extremes, and the scatter is zero."""
    for B_d in (0.04, 2.0 * 2.0 / 600.5):
        got = check(ctx, T, numpy.ones(len(T)), [2.0], [3.3], [B_d], label=("constant", B_d), min_count=1)
        B = got["n_bins"][0]
        assert got["secondary_depth"][0] == 0 == got["bump_depth"][0] == got["primary_depth"][0]
        assert got["secondary_phase"][0] == 3 / B == got["bump_phase"][0]
        assert got["scan_std"][0] == 0 == got["scan_mean"][0] and got["n_windows"][0] == B - 5 - 3
        assert numpy.isnan(got["secondary_significance"][0])
    # two windows as deep as each other, to the bit: the first is reported
    t = (numpy.arange(64 * 40) + 0.5) / 64 / 20           # P = 1: 64 bins, 40 points in each
    y = numpy.ones(len(t))
    b = spec.bins(t, 1.0, 0.0, 64)
    y[(b == 40) | (b == 20)] = 0.75
    y[(b == 50) | (b == 11)] = 1.25
    got = check(ctx, t, y, [1.0], [0.0], [2.0 / 64.5], label="equal windows")
    assert got["secondary_phase"][0] == 20 / 64 and got["bump_phase"][0] == 11 / 64 and got["secondary_count"][0] == 80


def test_several_fits_per_curve_in_any_order(ctx):
    rng = numpy.random.RandomState(7)
    rows = numpy.array([noisy(T, 10 + s, P=2.0 + 0.3 * s) for s in range(3)])
    which = numpy.array([2, 0, 1, 1, 0, 2, 1, 0, 0])
    period = 2.0 + 0.3 * which + rng.uniform(-0.01, 0.01, len(which))
    T0 = rng.uniform(3.0, 5.0, len(which))
    T0[:3] = 3.3
    period[:3] = 2.0 + 0.3 * which[:3]
    duration = rng.uniform(0.02, 0.2, len(which))
    got = check(ctx, T, rows, period, T0, duration, curve=which, label="scrambled")
    assert (got["primary_significance"][:3] > 10).all() and (got["secondary_significance"][:3] > 5).all()
    assert (abs(got["secondary_phase"][:3] - 0.4) < 0.05).all()          # (a bin is at most 1/20 wide)
    # one fit a curve, in order, without `curve`; one row without a batch dimension
    check(ctx, T, rows, period[[1, 2, 0]], T0[[1, 2, 0]], duration[[1, 2, 0]], label="in order")
    one = survey.phase_scan(T, rows[1], period[2], T0[2], duration[2], context=ctx)
    assert one.shape == (1,) and one[0].tobytes() == got[2].tobytes()


def test_bad_candidates(ctx):
    inf, nan = numpy.inf, numpy.nan
    bad = [(0.0, 3.3, 0.1), (-2.0, 3.3, 0.1), (nan, 3.3, 0.1), (inf, 3.3, 0.1), (-inf, 3.3, 0.1), (2.0, nan, 0.1),
           (2.0, inf, 0.1), (2.0, -inf, 0.1), (2.0, 3.3, 0.0), (2.0, 3.3, -0.1), (2.0, 3.3, nan), (2.0, 3.3, inf), (2.0, 3.3, 0.2501),
           (2.0, 3.3, 0.1)]
    period, T0, duration = (numpy.array(c) for c in zip(*bad))
    got = check(ctx, T, noisy(T, 8), period, T0, duration, curve=numpy.zeros(len(bad), dtype=int), label="bad")
    expect_equal(got["scan_status"], [1] * 13 + [0], "status")
    for k in got.dtype.names[1:]:
        assert numpy.isnan(got[k][:13]).all() and numpy.isfinite(got[k][13]), k
    # a flux that is not finite reaches the sums as it is: in the primary window it costs the primary depth, in the
    # baseline every depth
    b = spec.bins(T, 2.0, 3.3, 1000)
    y = noisy(T, 8)
    y[numpy.flatnonzero(b == 0)[0]] = nan
    got = check(ctx, T, y, [2.0], [3.3], [0.004], label="NaN in the primary")
    assert got["n_bins"][0] == 1000 and numpy.isnan(got["primary_depth"][0]) and got["n_windows"][0] >= 8
    assert 2 <= b[100] <= 997 and 2 <= b[700] <= 997
    y = noisy(T, 8)
    y[100] = nan
    got = check(ctx, T, y, [2.0], [3.3], [0.004], label="NaN in the baseline")
    assert got["scan_status"][0] == 0 and got["n_windows"][0] == 0 and numpy.isnan(got["secondary_depth"][0])
    y[100], y[700] = 1.0, inf
    check(ctx, T, y, [2.0], [3.3], [0.004], label="inf in the baseline")


@pytest.mark.parametrize("n", [1920, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 907])
def test_series_lengths(ctx, n):
    """One chunk of the kernel's LDS staging, its last point and the next, and three chunks with a tail that is no multiple of
    four; bins of every size class at each."""
    t = numpy.linspace(3.0, 3.0 + n / 48.0, n)
    y = numpy.array([noisy(t, n), noisy(t, n + 1, depth=4e-3)])
    q = numpy.array([40.5, 300.5, 1999.5, 4096.5])
    got = check(ctx, t, y, numpy.full(8, 2.0), numpy.full(8, 3.3), numpy.tile(4.0 / q, 2), curve=numpy.repeat([0, 1], 4),
                label=("n", n))
    assert (got["primary_significance"][[0, 1, 4, 5]] > 10).all()
    assert abs(got["secondary_phase"][0] - 0.4) < 0.03


def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; TLS_E_ARG for a curve out of range, max_bins outside [16, 4096], min_count < 1."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    t, y = _lib._f8(T), _lib._f8(numpy.ones((2, len(T))))
    one = numpy.array([2.0])
    out = numpy.full(1, -7.0, dtype=_lib.PHASE_SCAN_DTYPE)

    def call(curve, n_fits=1, max_bins=4096, min_count=3):
        c = _lib._i8(curve)
        return lib.tls_phase_scan(ctx._h, dp(t), dp(y), len(T), 2, ip(c), dp(one), dp(one), dp(numpy.array([0.1])), n_fits,
                                  max_bins, min_count, out.ctypes.data_as(ctypes.c_void_p))
    assert call([0], n_fits=0) == 0 and out["status"][0] == -7.0
    assert lib.tls_phase_scan(ctx._h, None, None, 0, 0, None, None, None, None, 0, 4096, 3, None) == 0
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(curve=[0], max_bins=15), dict(curve=[0], max_bins=4097),
               dict(curve=[0], min_count=0), dict(curve=[0], n_fits=-1)):
        assert call(**kw) == -1, kw                   # TLS_E_ARG
        assert out["status"][0] == -7.0
    assert call([1]) == 0 and out["status"][0] == 0 and out["n_bins"][0] == 40


# ---- in the pipeline ----------------------------------------------------------------------------------------------------
def run(ctx, flux, k, **more):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return survey.power_batch(T, flux, context=ctx, peaks=k, peak_fits=True, **more, **KW)


def check_pipeline(shared, peaks, label, **kw):
    """Every peak's scan equals the statement on the peak's own (period, T0, duration_days) and its curve's flux."""
    scanned = 0
    for c in range(peaks.shape[0]):
        for r in range(peaks.shape[1]):
            p = peaks[c, r]
            want = spec.expected(T, shared["y"][c], p["period"], p["T0"], p["duration_days"], **kw)
            if p["status"] != 0:
                assert want["status"] == 1, (label, c, r)
            for k in survey.phase_scan_fields():
                expect_equal(p[k], want["status" if k == "scan_status" else k], (label, c, r, k))
            scanned += want["status"] == 0
    return scanned


@pytest.mark.parametrize("n_curves", [17, 33])
def test_pipeline_at_slab_and_group_edges(ctx, shared, n_curves):
    """17 curves x 8 peaks: 136 fits, the slab of 128 ends inside curve 16's candidates; 33 curves: a group of 32 and one.
    Everything else of the call equals the call without the scan, byte for byte."""
    flux = batch(n_curves)
    summary, periods, pk = run(ctx, flux, 8, statistics=True, phase_scan=True)
    peaks, n_peaks = pk["peaks"], pk["n_peaks"]
    assert peaks.shape == (n_curves, 8)
    assert peaks.dtype.names[-len(survey.phase_scan_fields()):] == survey.phase_scan_fields()
    assert check_pipeline(shared, peaks, n_curves) >= 2 * n_curves
    past = numpy.arange(8)[None, :] >= n_peaks[:, None]
    assert past.any()                                                    # (peaks of status 1: no such peak)
    assert (peaks["status"][past] == 1).all() and (peaks["scan_status"][past] == 1).all()
    assert (peaks["scan_status"][~past] == 0).all() and numpy.isnan(peaks["secondary_depth"][past]).all()
    # the two injected planets are the first two peaks: their transits are the primaries, far above the windows' scatter
    assert (peaks["primary_significance"][:, :2] > 10).all()
    without = run(ctx, flux, 8, statistics=True)
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(periods, without[1], "periods")
    expect_equal(n_peaks, without[2]["n_peaks"], "n_peaks")
    assert peaks.dtype.names[:len(without[2]["peaks"].dtype.names)] == without[2]["peaks"].dtype.names
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k


def test_pipeline_bins_and_counts(ctx, shared):
    """The caller's max_bins and min_count reach the kernel; the scans do not need the best pick's statistics."""
    summary, periods, pk = run(ctx, batch(3), 4, phase_scan=True, phase_scan_max_bins=24, phase_scan_min_count=40)
    assert "snr" not in summary.dtype.names
    assert check_pipeline(shared, pk["peaks"], "bins and counts", max_bins=24, min_count=40) >= 6
    fitted = pk["peaks"]["status"] == 0
    assert (pk["peaks"]["n_bins"][fitted] <= 24).all() and (pk["peaks"]["n_bins"][fitted] == 24).sum() >= 6


def test_injected_records_of_every_status(ctx, shared):
    """Peak records nobody searched for (tls_debug_peak_phase_scans): a curve without peaks, ranks past n_peaks (status 1) and
    an index where the search fitted nothing (status 2) give scans of status 1; the fits equal tls_debug_peak_fits'."""
    inp, k = shared["inp"], 4
    y = numpy.ascontiguousarray(shared["y"][:3])
    rows = sorted({int(w): r for r, w in reversed(list(enumerate(inp["table"].width)))}.values())
    rng = numpy.random.RandomState(5)
    n_p = len(inp["periods"])
    rec = numpy.zeros((3, k), dtype=_lib.PEAK_DTYPE)
    rec["index"] = rng.randint(1, n_p - 1, (3, k))
    rec["period"] = inp["periods"][rec["index"]]
    rec["row"] = rng.choice(rows, (3, k))
    rec["depth"] = 1 - rng.uniform(5e-4, 4e-3, (3, k))
    rec["chi2"] = rng.uniform(900, 1000, (3, k))
    power = rng.normal(0, 1, (3, n_p))
    rec["row"][2, 1] = -1
    n_peaks = numpy.array([0, 2, 4])
    ctx.prepare(inp["t"], y[0], numpy.full(len(T), numpy.std(y[0])), inp["periods"], inp["table"], inp["params"])
    root = numpy.array([float(i) ** 0.5 for i in range(len(T) + 1)])
    root_count = numpy.array([float(numpy.sum(i) ** 0.5) for i in range(len(T) + 1)])
    args = (y, rec, n_peaks, power, inp["table"].duration, calculate_fill_factor(inp["t"]), root,
            survey._max_epochs(inp["t"], inp["periods"]))
    fits, scans = ctx.debug_peak_fits(*args, phase_scan=(4096, 3), root_count=root_count)
    assert fits.tobytes() == ctx.debug_peak_fits(*args, root_count=root_count).tobytes()
    expect_equal(fits["status"], [[1, 1, 1, 1], [0, 0, 1, 1], [0, 2, 0, 0]], "fit status")
    expect_equal(scans["status"], [[1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 0, 0]], "scan status")
    for c in range(3):
        for r in range(k):
            want = spec.scan(T, y[c], rec["period"][c, r], fits["T0"][c, r], fits["duration_days"][c, r])
            if fits["status"][c, r] != 0:
                want = spec.scan(T, y[c], numpy.nan, numpy.nan, numpy.nan)
            for name in spec.FIELDS:
                expect_equal(scans[name][c, r], want[name], (c, r, name))


def test_two_contexts_equal_the_one_device_call():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = batch(33)
        one = survey.power_batch(T, f, device=0, peaks=3, peak_fits=True, phase_scan=True, **KW)
        two = survey.power_batch(T, f, devices=[0, 0], peaks=3, peak_fits=True, phase_scan=True, **KW)
    assert one[0].tobytes() == two[0].tobytes()
    assert one[2]["peaks"].dtype == two[2]["peaks"].dtype and "secondary_significance" in one[2]["peaks"].dtype.names
    for k in one[2]["peaks"].dtype.names:
        expect_equal(two[2]["peaks"][k], one[2]["peaks"][k], k)
    expect_equal(two[2]["n_peaks"], one[2]["n_peaks"], "n_peaks")
