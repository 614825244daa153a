"""The variability periodogram on the device (survey.lomb_scargle / tls_lomb_scargle, tls_nudft) and the sine test
(survey.sine_test / tls_sine_test; power_batch(peaks=K, peak_fits=True, sine_test=True)) against tests/gls_spec.py:

  * the sums against the exact sums within the derived bound (n + 2 pi max|f (t - t_0)| + 8) 2^-52 sum|A| -- the a-priori bound
    of an n-term fp64 dot product in any order, the phase's rounding carried through the trigonometry, a few ulp of the
    trigonometry -- at the edges of the row tile (32 and 128 rows: at most 32 rows take the 32-row kernel), of the frequency
    tile (64) and of the time chunk (32), with a gap, with f T = 4500, with duplicate frequencies;
  * the prologue (mean, variance, the centred rows, the weights) bit for bit, and power and amplitude equal to the statement's
    epilogue of the device's OWN sums bit for bit; phase is the device's atan2, held to 4 * 2^-53 cycles: 3 ulp of an angle up
    to pi (2^-51 each) over 2 pi are 2.1e-16, the division adds 2^-54;
  * end to end against scipy.signal.lombscargle at ten times max|statement - scipy| of the same inputs, computed here;
  * the peaks against tests/peaks_spec.py on the device's power; NaN for a constant row and where D <= 0;
  * the sine test: n_used, mean and variance bit for bit, its sums within the same bound, its records from its own sums.

Time stamps are multiples of 1/64 d."""
import ctypes
import warnings

import numpy
import pytest
from scipy.signal import lombscargle

import gls_spec as spec
import peaks_spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

PHASE_TOL = 4 * 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def series(n, gap_at=None, gap=0):
    """n time stamps at 1/64 d, `gap` cadences missing in front of index gap_at."""
    t = 1.0 + numpy.arange(n + gap) / 64.0
    return t if gap_at is None else numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def curves(t, rows, seed=0, dy=False):
    """`rows` curves around 1 with noise 3e-4 and a sinusoid of their own; per-point errors with dy."""
    rng = numpy.random.RandomState(seed)
    y = 1 + rng.normal(0, 3e-4, (rows, len(t))) + 2e-3 * numpy.sin(2 * numpy.pi * t / rng.uniform(0.3, 2.0, (rows, 1)) + 0.4)
    return y, (3e-4 * (1 + 0.5 * rng.uniform(size=y.shape)) if dy else None)


def same(a, b, what=""):
    numpy.testing.assert_array_equal(numpy.asarray(a, dtype=float), numpy.asarray(b, dtype=float), err_msg=str(what))


def within(got, exact, bound, what):
    """|got - exact| <= bound (bound [R] a row), with the largest share of the bound in the message."""
    off = numpy.abs(got - exact)
    bound = numpy.broadcast_to(bound.reshape((-1,) + (1,) * (numpy.ndim(got) - 1)), off.shape)
    share = numpy.max(off[bound > 0] / bound[bound > 0], initial=0.0)         # (a row of zeros has the bound 0, and meets it)
    assert numpy.all(off <= bound), (what, float(share))
    return float(share)


def phase_close(got, want, what):
    d = numpy.abs(got - want)
    d = numpy.minimum(d, 1.0 - d)                    # (phase lives on a circle: -0.5 is 0.5)
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want)) and numpy.all(d[~numpy.isnan(d)] <= PHASE_TOL), what


# ---- kernel A: the sums ------------------------------------------------------------------------------------------------------
# (rows, frequencies, points): one below, at and one above the tiles (32 / 128 rows, 64 frequencies) and the chunk (32 points)
SHAPES = [(1, 1, 3), (31, 63, 31), (32, 64, 32), (33, 65, 33), (127, 1, 64), (128, 64, 65), (129, 65, 33), (2, 130, 97)]


@pytest.mark.parametrize("R, F, n", SHAPES)
def test_nudft_at_the_edges_of_the_tiles(ctx, R, F, n):
    rng = numpy.random.RandomState(R * 1000 + F + n)
    t = series(n, gap_at=n // 2, gap=40)
    rows = rng.normal(0, 1, (R, n))
    f = numpy.sort(rng.uniform(0.05, 30.0, F))
    got = ctx.nudft(rows, t, f)
    assert got.shape == (R, F, 2)
    within(got, spec.exact_sums(t, rows, f), spec.sum_bound(t, rows, f), (R, F, n))


def test_nudft_long_series_high_frequencies_and_duplicates(ctx):
    """2100 points (65 chunks and 20 points) with a gap, 600 frequencies up to f T = 4500, some of them twice."""
    t = series(2100, gap_at=900, gap=300)
    rng = numpy.random.RandomState(5)
    f = numpy.linspace(0.01, 4500.0 / (t[-1] - t[0]), 600)
    f[100:110] = f[90:100]
    f[599] = 4500.0 / (t[-1] - t[0])
    rows = rng.normal(0, 1, (2, len(t)))
    got = ctx.nudft(rows, t, f)
    assert abs(f[599] * (t[-1] - t[0]) - 4500) < 1e-9
    share = within(got, spec.exact_sums(t, rows, f), spec.sum_bound(t, rows, f), "long")
    print("largest share of the bound: %.3g" % share)
    assert got[:, 100:110].tobytes() == got[:, 90:100].tobytes()
    assert share > 1e-7                              # (the device did compute something of its own: not the exact sums)


def test_a_dropped_element_breaks_the_bound():
    """The bound separates a correct product from one with a dropped or doubled element by many orders."""
    t = series(97, gap_at=40, gap=10)
    rows = numpy.random.RandomState(1).normal(0, 1, (2, 97))
    f = numpy.linspace(0.1, 20, 7)
    exact = spec.exact_sums(t, rows, f)
    wrong = rows.copy()
    wrong[:, 50] = 0.0
    share = numpy.abs(spec.exact_sums(t, wrong, f) - exact) / spec.sum_bound(t, rows, f)[:, None, None]
    assert share.max() > 1e6


# ---- the periodogram ---------------------------------------------------------------------------------------------------------
def check_periodogram(ctx, t, y, dy, f, label):
    """ctx.lomb_scargle against the statement: prologue bit for bit, sums within the bound, epilogue from the device's sums."""
    got = ctx.lomb_scargle(t, y, f, dy=dy, debug=True)
    R = len(y)
    want = [spec.prologue(y[r], None if dy is None else dy[r]) for r in range(R)]
    same(got["mean"], [w[2] for w in want], (label, "mean"))
    same(got["variance"], [w[3] for w in want], (label, "variance"))
    same(got["rows"], [w[1] for w in want], (label, "rows"))
    same(got["weights"], want[0][0] if dy is None else [w[0] for w in want], (label, "weights"))
    a = numpy.array([w[1] for w in want])
    w = numpy.array([x[0] for x in want])
    sums = got["sums"]
    assert sums.shape == (R, len(f), 6)
    within(sums[:, :, 0:2], spec.exact_sums(t, a, f), spec.sum_bound(t, a, f), (label, "YC YS"))
    w_exact = spec.exact_sums(t, w if dy is not None else w[:1], f)
    w2_exact = spec.exact_sums(t, w if dy is not None else w[:1], 2.0 * f)
    within(sums[:, :, 2:4], numpy.broadcast_to(w_exact, (R, len(f), 2)), spec.sum_bound(t, w, f), (label, "C S"))
    within(sums[:, :, 4:6], numpy.broadcast_to(w2_exact, (R, len(f), 2)), spec.sum_bound(t, w, 2.0 * f), (label, "C2 S2"))
    power, amplitude, phase = spec.epilogue(*numpy.moveaxis(sums, 2, 0), got["variance"][:, None])
    same(got["power"], power, (label, "power"))
    same(got["amplitude"], amplitude, (label, "amplitude"))
    phase_close(got["phase"], phase, (label, "phase"))
    return got


@pytest.mark.parametrize("with_dy", [False, True])
@pytest.mark.parametrize("R", [3, 40])
def test_periodogram_equals_the_statement(ctx, R, with_dy):
    """3 rows take the 32-row kernel, 40 the 128-row one; a gap; duplicate frequencies; out of order."""
    t = series(330, gap_at=120, gap=70)
    y, dy = curves(t, R, seed=R, dy=with_dy)
    f = survey.variability_frequencies(t, oversampling=2, f_max=12.0)[::-1].copy()
    f[5] = f[17]
    got = check_periodogram(ctx, t, y, dy, f, (R, with_dy))
    assert numpy.isfinite(got["power"]).all() and numpy.isfinite(got["phase"]).all()


@pytest.mark.parametrize("with_dy", [False, True])
def test_periodogram_against_scipy(ctx, with_dy):
    """End to end at ten times the statement's own distance from scipy on the same inputs."""
    t = series(500, gap_at=200, gap=60)
    y, dy = curves(t, 2, seed=11, dy=with_dy)
    f = survey.variability_frequencies(t, oversampling=3, f_max=16.0)
    got = survey.lomb_scargle(t, y, f, dy_batch=dy, context=ctx)
    for r in range(2):
        kw = dict(weights=1 / dy[r] ** 2) if with_dy else {}
        theirs = lombscargle(t, y[r], 2 * numpy.pi * f, normalize=True, floating_mean=True, **kw)
        mine = spec.lomb_scargle(t, y[r], f, None if dy is None else dy[r])["power"]
        scale = numpy.abs(mine - theirs).max()
        print("max|statement - scipy| = %.3g, max|device - scipy| = %.3g" % (scale, numpy.abs(got["power"][r] - theirs).max()))
        assert 0 < scale < 1e-8
        assert numpy.abs(got["power"][r] - theirs).max() <= 10 * scale


def test_constant_rows_and_coinciding_phases(ctx):
    """YY = 0 gives NaN; n = 3 at a frequency where every point has one phase gives D = 0 and NaN."""
    t = numpy.array([0.0, 1.0, 2.0])
    y = numpy.array([[1.0, 1.0, 1.0], [1.0, 1.5, 0.75]])
    f = numpy.array([1.0, 0.3])
    got = check_periodogram(ctx, t, y, None, f, "n = 3")
    assert got["variance"][0] == 0.0 and numpy.isnan(got["power"][0]).all() and numpy.isnan(got["amplitude"][0]).all()
    assert numpy.isnan(got["power"][1, 0]) and numpy.isnan(got["phase"][1, 0]) and numpy.isfinite(got["power"][1, 1])
    t = series(256)                                  # (1 / 256 and the sum are exact: the mean of the constant row is the constant)
    y = numpy.vstack([numpy.full(256, 0.75), curves(t, 1, seed=3)[0][0]])
    got = check_periodogram(ctx, t, y, None, numpy.array([0.5, 1.0, 4.0]), "constant")
    assert numpy.isnan(got["power"][0]).all() and numpy.isfinite(got["power"][1]).all()


def test_two_slabs(ctx):
    """32769 rows of 3 points: the second slab of tls_lomb_scargle (with the shared weight row of the first) and of tls_nudft."""
    rng = numpy.random.RandomState(8)
    t = numpy.array([0.0, 0.5, 2.0])
    y = 1 + rng.normal(0, 1e-2, (32769, 3))
    f = numpy.array([0.3])
    got = ctx.lomb_scargle(t, y, f, debug=True)
    w = numpy.float64(1.0) / numpy.float64(3.0)
    ybar = (w * y[:, 0] + w * y[:, 1]) + w * y[:, 2]                   # (the ordered sum from 0.0: 0.0 + x is x)
    d = y - ybar[:, None]
    a = w * d
    same(got["mean"], ybar, "mean")
    same(got["variance"], (a[:, 0] * d[:, 0] + a[:, 1] * d[:, 1]) + a[:, 2] * d[:, 2], "variance")
    same(got["rows"], a, "rows")
    for r in (0, 1, 32767, 32768):
        want = spec.prologue(y[r])
        assert want[2] == got["mean"][r] and want[3] == got["variance"][r]
    within(got["sums"][:, :, 0:2], spec.exact_sums(t, a, f), spec.sum_bound(t, a, f), "YC YS")
    assert (got["sums"][:, :, 2:] == got["sums"][0, :, 2:]).all()
    power, amplitude, _ = spec.epilogue(*numpy.moveaxis(got["sums"], 2, 0), got["variance"][:, None])
    same(got["power"], power, "power")
    same(got["amplitude"], amplitude, "amplitude")
    within(ctx.nudft(y, t, f), spec.exact_sums(t, y, f), spec.sum_bound(t, y, f), "nudft")


def test_peaks_equal_the_selection_on_the_device_power(ctx):
    t = series(400, gap_at=150, gap=30)
    y, dy = curves(t, 5, seed=21, dy=True)
    f = survey.variability_frequencies(t, oversampling=4, f_max=10.0)
    got = survey.lomb_scargle(t, y, f, dy_batch=dy, peaks=6, context=ctx)
    assert got["peaks"].shape == (5, 6) and set(got) == {"frequencies", "mean", "variance", "power", "amplitude", "phase",
                                                          "peaks", "n_peaks"}
    for r in range(5):
        want, m = peaks_spec.expected(got["power"][r], 1.0 / f, 6, 0.02, (0.5, 2.0))
        assert got["n_peaks"][r] == m >= 1
        for k in want.dtype.names:
            same(got["peaks"][k][r], want[k], (r, k))
    lean = survey.lomb_scargle(t, y, f, dy_batch=dy, peaks=6, with_arrays=False, context=ctx)
    assert set(lean) == {"frequencies", "mean", "variance", "peaks", "n_peaks"}
    assert lean["peaks"].tobytes() == got["peaks"].tobytes() and lean["n_peaks"].tobytes() == got["n_peaks"].tobytes()
    one = survey.lomb_scargle(t, y[2], f, dy_batch=dy[2], peaks=6, context=ctx)
    assert one["power"].shape == (len(f),) and one["peaks"].shape == (6,)
    same(one["power"], got["power"][2])
    assert one["peaks"].tobytes() == got["peaks"][2].tobytes()
    # the highest peak is the row's own sinusoid
    best = got["peaks"]["index"][:, 0]
    assert (got["power"][numpy.arange(5), best] == got["power"].max(axis=1)).all()


def test_contexts_devices_and_detrend(ctx):
    """Two contexts and devices=[0, 0] give the one-context result; detrend= is applied to the rows first."""
    t = series(300)
    y, _ = curves(t, 70, seed=31)
    f = survey.variability_frequencies(t, oversampling=2, f_max=8.0)
    one = survey.lomb_scargle(t, y, f, peaks=3, context=ctx)
    other = _lib.Context(0)
    try:
        two = survey.lomb_scargle(t, y, f, peaks=3, context=other)
        back = survey.lomb_scargle(t, y, f, peaks=3, context=ctx)
    finally:
        other.close()
    split = survey.lomb_scargle(t, y, f, peaks=3, devices=[0, 0])
    for k in one:
        assert one[k].tobytes() == two[k].tobytes() == back[k].tobytes() == split[k].tobytes(), k
    flat = survey.detrend_batch(y, 25, context=ctx)
    a = survey.lomb_scargle(t, y, f, detrend=25, context=ctx)
    b = survey.lomb_scargle(t, flat, f, context=ctx)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and a["power"].tobytes() != one["power"].tobytes()


def test_c_entry_arguments(ctx):
    """Every TLS_E_ARG case returns before any device work with the output untouched; zero rows are a no-op."""
    lib, dp = ctx._lib, _lib._dp
    t = series(16)                                   # (1 / 16 is exact: the ones have the mean 1 and YY = 0)
    y = numpy.ones((1, 16))
    f = numpy.array([1.0, 2.0])
    mean, var = numpy.full(1, 7.0), numpy.full(1, 7.0)
    out = numpy.full((1, 2, 2), 7.0)

    def gls(t=t, n=16, f=f, F=2, rows=1):
        return lib.tls_lomb_scargle(ctx._h, dp(t), dp(y), None, n, rows, dp(f), F, dp(mean), dp(var), None, None, None, 0, 0.02,
                                    None, None, None, None, None)

    def nudft(t=t, n=16, f=f, F=2, rows=1):
        return lib.tls_nudft(ctx._h, dp(y), rows, n, dp(t), dp(f), F, dp(out))
    bad_t = t.copy()
    bad_t[3] = numpy.nan
    for kw in (dict(n=2), dict(n=0), dict(F=0), dict(f=numpy.array([1.0, 0.0])), dict(f=numpy.array([numpy.inf, 1.0])),
               dict(f=numpy.array([-1.0, 1.0])), dict(t=t[::-1].copy()), dict(t=bad_t), dict(rows=-1)):
        assert gls(**kw) == -1, kw
        assert mean[0] == 7.0 and var[0] == 7.0
        if kw != dict(n=2):
            assert nudft(**kw) == -1, kw
        assert (out == 7.0).all()
    assert gls(rows=0) == 0 and nudft(rows=0) == 0 and mean[0] == 7.0 and (out == 7.0).all()
    assert gls() == 0 and var[0] == 0.0 and nudft() == 0 and not (out == 7.0).any()
    rec = numpy.full(1, 7.0, dtype=_lib.SINE_DTYPE)
    rec_h = numpy.full((1, 1), 7.0, dtype=_lib.SINE_HARMONIC_DTYPE)
    curve, P, h = numpy.zeros(1, dtype=numpy.int64), numpy.array([1.0]), numpy.array([1.0])

    def sine(curve=curve, h=h, nH=1, mask=1.5, t=t, T0=None, fits=1):
        return lib.tls_sine_test(ctx._h, dp(t), dp(y), None, 16, 1, dp(P), T0, None, _lib._ip(curve), fits, dp(h), nH, mask,
                                 rec.ctypes.data_as(ctypes.c_void_p), rec_h.ctypes.data_as(ctypes.c_void_p), None)
    for kw in (dict(curve=numpy.array([1])), dict(curve=numpy.array([-1])), dict(nH=0), dict(nH=9), dict(h=numpy.array([0.0])),
               dict(h=numpy.array([numpy.nan])), dict(mask=-1.0), dict(mask=numpy.nan), dict(t=bad_t), dict(T0=dp(P)), dict(fits=-1)):
        assert sine(**kw) == -1, kw
        assert rec["status"][0] == 7.0 and rec_h["power"][0, 0] == 7.0
        assert b"sine test" in lib.tls_last_error(ctx._h), kw
    assert sine(fits=0) == 0 and rec["status"][0] == 7.0
    assert sine() == 0 and rec["status"][0] == 0 and rec["n_used"][0] == 16 and numpy.isnan(rec_h["power"][0, 0])   # (YY = 0)


# ---- kernel B: the sine test -------------------------------------------------------------------------------------------------
def check_sine(ctx, t, y, dy, period, T0=None, duration=None, curve=None, mask=1.5, harmonics=(0.5, 1.0, 2.0), label=""):
    """ctx.sine_test of the candidates against the statement; (records, harmonic records)."""
    y = numpy.atleast_2d(y)
    got, got_h, sums = ctx.sine_test(t, y, period, curve=curve, dy=dy, T0=T0, duration=duration, mask=mask, harmonics=harmonics,
                                     debug=True)
    which = numpy.arange(len(y)) if curve is None else curve
    assert got.shape == (len(period),) and got_h.shape == sums.shape[:2] == (len(period), len(harmonics))
    for i, c in enumerate(which):
        want = spec.sine_test(t, y[c], period[i], None if dy is None else dy[c], None if T0 is None else T0[i],
                              None if T0 is None else duration[i], mask, harmonics)
        for k in ("status", "n_used", "mean", "variance"):
            same(got[k][i], want[k], (label, i, k))
        if want["status"] != 0:
            assert all(numpy.isnan(got_h[k][i]).all() for k in got_h.dtype.names) and numpy.isnan(sums[i]).all(), (label, i)
            continue
        for h, fr in enumerate(want["frequencies"]):
            a, w = numpy.where(want["used"], want["a"], 0.0), numpy.where(want["used"], want["w"], 0.0)
            bound_a, bound_w, bound_w2 = (spec.sum_bound(t, a, [fr])[0], spec.sum_bound(t, w, [fr])[0],
                                          spec.sum_bound(t, w, [2.0 * fr])[0])
            assert numpy.all(numpy.abs(sums[i, h, 0:2] - want["exact"][h, 0:2]) <= bound_a), (label, i, h)
            assert numpy.all(numpy.abs(sums[i, h, 2:4] - want["exact"][h, 2:4]) <= bound_w), (label, i, h)
            assert numpy.all(numpy.abs(sums[i, h, 4:6] - want["exact"][h, 4:6]) <= bound_w2), (label, i, h)
        records = spec.sine_harmonics(sums[i], got["variance"][i], got["n_used"][i])
        for k, v in zip(got_h.dtype.names, records):
            if k == "phase":
                phase_close(got_h[k][i], v, (label, i, k))
            else:
                same(got_h[k][i], v, (label, i, k))
    return got, got_h


@pytest.mark.parametrize("with_dy", [False, True])
def test_sine_test_without_a_mask(ctx, with_dy):
    """The mask removes nothing; n below, at and above the 256 lanes; several candidates a curve; curve out of order."""
    for n in (5, 255, 256, 257, 700):
        t = series(n, gap_at=n // 2, gap=20)
        y, dy = curves(t, 3, seed=n, dy=with_dy)
        got, got_h = check_sine(ctx, t, y, dy, [1.1, 0.7, 3.0, 0.7, 2.2], curve=[2, 0, 1, 0, 2], label=("no mask", n))
        assert (got["status"] == 0).all() and (got["n_used"] == n).all()
        assert got_h[1].tobytes() == got_h[3].tobytes()


def test_sine_test_masks(ctx):
    """A mask that leaves 3 points (status 2), exactly 4, and an ordinary one; a NaN candidate among good ones."""
    t = series(300)
    y, dy = curves(t, 2, seed=41, dy=True)
    P = 1024.0                                       # (one epoch: tau = t - T0, exact)
    T0 = [t[0]] * 3 + [t[7], numpy.nan, t[7], t[7], t[7]]
    d = [(296.5 / 64) / 0.75, (295.5 / 64) / 0.75, (290.5 / 64) / 0.75, 0.125, 0.125, numpy.nan, 0.0, 0.125]
    period = [P, P, P, 0.75, 0.75, 0.75, 0.75, numpy.inf]
    got, got_h = check_sine(ctx, t, y, dy, period, T0, d, curve=[0, 0, 1, 1, 1, 0, 0, 0], label="masks")
    assert got["status"].tolist() == [2, 0, 0, 0, 1, 1, 1, 1]
    assert got["n_used"][:3].tolist() == [3, 4, 9] and 200 <= got["n_used"][3] <= 230     # (13 of 48 cadences an epoch are out)
    assert numpy.isfinite(got_h["significance"][2:4]).all()
    wider, _ = check_sine(ctx, t, y, None, [0.75], [t[7]], [0.125], curve=[1], mask=3.0, label="mask 3")
    assert wider["n_used"][0] < got["n_used"][3]


def test_sine_test_slabs(ctx):
    """1030 candidates: two slabs; every 41st and those around the slab's edge against the statement."""
    t = series(90)
    y, dy = curves(t, 4, seed=51, dy=True)
    rng = numpy.random.RandomState(2)
    period = rng.uniform(0.2, 1.5, 1030)
    curve = rng.randint(0, 4, 1030)
    T0, d = t[0] + rng.uniform(0, 0.2, 1030), rng.uniform(0.01, 0.05, 1030)
    got, got_h = ctx.sine_test(t, y, period, curve=curve, dy=dy, T0=T0, duration=d)
    some = numpy.unique(numpy.r_[0:1030:41, 1022:1027, 1029])
    part, part_h = check_sine(ctx, t, y, dy, period[some], T0[some], d[some], curve=curve[some], label="slabs")
    assert part.tobytes() == got[some].tobytes() and part_h.tobytes() == got_h[some].tobytes()
    assert (got["status"] == 0).all()


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
T = 3.0 + numpy.arange(960) / 48.0                    # 20 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)


def test_pipeline(ctx):
    """power_batch(peaks=4, peak_fits=True, sine_test=True) on 8 curves equals survey.sine_test on its own fits, and every
    other field equals the call without the keyword bit for bit."""
    rows = []
    for s in range(8):
        rng = numpy.random.RandomState(2000 + s)
        f = transit_model.light_curve(T, T[0] + 0.7, 1.9, 0.07, 8.0, 89.8, 0, 90, [0.4, 0.3], "quadratic")
        rows.append(f + rng.normal(0, 4e-4, len(T)) + (2e-3 * numpy.sin(2 * numpy.pi * T / 3.1 + s) if s % 2 else 0.0))
    flux = numpy.array(rows)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(context=ctx, peaks=4, peak_fits=True, **KW)
        summary, periods, pk = survey.power_batch(T, flux, sine_test=True, **more)
        without = survey.power_batch(T, flux, **more)
    peaks = pk["peaks"]
    names = survey.sine_test_fields()
    assert peaks.shape == (8, 4) and peaks.dtype.names[-len(names):] == names
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    same(periods, without[1], "periods")
    same(pk["n_peaks"], without[2]["n_peaks"], "n_peaks")
    assert peaks.dtype.names[:-len(names)] == without[2]["peaks"].dtype.names and set(pk) == set(without[2])
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 8
    args = dict(T0=peaks["T0"][curve, rank], duration=peaks["duration_days"][curve, rank])
    alone = survey.sine_test(T, flux, peaks["period"][curve, rank], curve=curve, context=ctx, **args)
    assert alone.dtype.names == names and alone["sine_power"].shape == (len(curve), 3)
    for k in names:
        same(peaks[k][curve, rank], alone[k], k)
    check_sine(ctx, T, flux, None, peaks["period"][curve, rank][:6], args["T0"][:6], args["duration"][:6], curve=curve[:6],
               label="pipeline")
    rest = peaks["status"] != 0
    assert (peaks["sine_status"][rest] == 1).all() and all(numpy.isnan(peaks[k][rest]).all() for k in names[1:])
    # the planet is among the peaks of the quiet curves, and tested
    assert ((numpy.abs(peaks["period"][::2] - 1.9) < 0.04) & (peaks["sine_status"][::2] == 0)).any(axis=1).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        split = survey.power_batch(T, flux, sine_test=True, devices=[0, 0], peaks=4, peak_fits=True, **KW)
    assert split[2]["peaks"].tobytes() == peaks.tobytes()
