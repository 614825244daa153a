"""Transit times on the device (survey.transit_times / tls_transit_times; power_batch(peaks=K, peak_fits=True,
transit_times=True)) against tests/transit_times_spec.py bit for bit, every field of both records: at the edges of the
statement (the ends of the series, gaps hit exactly, time stamps hit exactly and half-way, ties, constant flux, the gates of the
step and of min_ses, 0 to 3 timed epochs, the epoch limit, bad ephemerides), of the kernel (more units than threads, fewer than
a wave, the widest reach, chunks of epochs) and of the call (several candidates a curve, slabs, two contexts, argument errors),
and in the pipeline with every other result untouched.

Time stamps are multiples of 1/64 d, so every time difference is exact.  Two of the statement's conditions cannot be met:
a held window has (L - 1) // 2 >= 1 samples in front of its centre c and L // 2 >= 1 behind, so c is never 0 or n - 1 and the
epoch status 2 "c at an end of the series" is unreachable; the kernel keeps the check all the same."""
import ctypes
import warnings

import numpy
import pytest

import transit_times_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

WIDTHS = [3, 4, 5, 8, 37, 65]
SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")
DT = 1 / 64.0
_SHAPES = {}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def shapes_of(widths):
    """The rows' shapes, computed once a width."""
    for L in widths:
        if int(L) not in _SHAPES:
            _SHAPES[int(L)] = spec.shapes_of([L], **SHAPE)[0]
    return [_SHAPES[int(L)] for L in widths]


def spans_of(widths, gap_tolerance=0.5):
    return [(int(L) - 1) * DT * (1 + gap_tolerance) for L in widths]


def series(n, gap_at=None, gap=0):
    """n time stamps at 1/64 d, `gap` cadences missing in front of index gap_at."""
    t = 1.0 + numpy.arange(n + gap) / 64.0
    return t if gap_at is None else numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def dips(t, period, T0, width, depth=4e-3, seed=0, sigma=1e-3, shift=None):
    """Noise of `sigma` and a box dip of `width` samples centred on the sample nearest every T0 + e * period (moved by
    shift[e] samples)."""
    rng = numpy.random.RandomState(seed)
    y = 1 + rng.normal(0, sigma, len(t)) if sigma else numpy.ones(len(t))
    e = int(numpy.ceil((t[0] - T0) / period))
    while T0 + e * period <= t[-1]:
        c = int(numpy.argmin(numpy.abs(t - (T0 + e * period)))) + (0 if shift is None else int(shift[e % len(shift)]))
        y[max(0, c - width // 2): max(0, c - width // 2 + width)] -= depth
        e += 1
    return y


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check(ctx, t, y, dy, period, T0, row, reach, widths=WIDTHS, span_max=None, curve=None, label="", **kw):
    """ctx.transit_times of the candidates equals the statement: every field of both records; what the device returned."""
    y = numpy.atleast_2d(y)
    dy = numpy.broadcast_to(numpy.asarray(dy, dtype=float), y.shape) if numpy.ndim(dy) < 2 else dy
    shapes = shapes_of(widths)
    span_max = spans_of(widths) if span_max is None else span_max
    kw.setdefault("max_epochs", 48)
    got = ctx.transit_times(t, y, dy, period, T0, row, reach, widths, shapes, span_max, curve=curve, **kw)
    which = numpy.arange(len(y)) if curve is None else curve
    want = spec.expected(t, y, dy, which, period, T0, row, reach, shapes, span_max, **kw)
    assert got[0].dtype.names == spec.EPHEMERIS_FIELDS and got[1].dtype.names == spec.TIME_FIELDS
    assert got[0].shape == want[0].shape == (len(period),) and got[1].shape == want[1].shape == (len(period), kw["max_epochs"])
    for f in spec.EPHEMERIS_FIELDS:
        expect_equal(got[0][f], want[0][f], (label, f))
    for f in spec.TIME_FIELDS:
        expect_equal(got[1][f], want[1][f], (label, f))
    return got


def statuses(times, f=0):
    e = times["status"][f]
    return e[~numpy.isnan(e)].astype(int).tolist()


@pytest.mark.parametrize("n", [257, 300, 700])
def test_every_row_and_the_ends_of_the_series(ctx, n):
    """Every row of the table, odd and even, with the first epoch on t[0] and the last on t[n-1]: at reach 1 no window of
    theirs lies inside the series (status 1) unless the row is 3 or 4 samples wide; at a reach of the width some do."""
    t = series(n)
    P = (n - 1) * DT / 4
    rows = numpy.arange(len(WIDTHS))
    y = numpy.array([dips(t, P, t[0], L, seed=L) for L in WIDTHS])
    eph, times = check(ctx, t, y, 1e-3, numpy.full(6, P), numpy.full(6, t[0]), rows, numpy.ones(6, dtype=int), label=("reach 1", n))
    for f, L in enumerate(WIDTHS):
        # (centre 1 holds a whole window of (L - 1) // 2 = 1 samples in front, centre n - 2 one of L // 2 = 1 behind)
        assert eph["n_epochs"][f] == 5 and (statuses(times, f)[0] == 1) == (L > 4) and (statuses(times, f)[-1] == 1) == (L > 3), L
        assert times["time_linear"][f][0] == t[0] and times["time_linear"][f][4] == t[-1]
    assert (eph["n_timed"] >= 2).all() and (eph["epoch_first"] == 0).all()
    eph, times = check(ctx, t, y, 1e-3, numpy.full(6, P), numpy.full(6, t[0]), rows, numpy.array(WIDTHS), min_ses=0.0,
                       label=("reach L", n))
    for f, L in enumerate(WIDTHS):
        assert statuses(times, f)[0] != 1 and times["index"][f][0] >= (L - 1) // 2 and times["index"][f][4] <= n - 1 - L // 2


def test_gaps(ctx):
    """An epoch inside a gap: at reach 1 every window of L = 37 runs over it (status 1), at reach 40 some lie beside it.  A
    window that hits span_max exactly is kept, one cadence less and it is not."""
    n = 500
    t = series(n, gap_at=250, gap=20)
    P, T0 = 100 * DT, t[50]                          # epochs at samples 50, 150, [gap: 250], 330, 430
    y = dips(t, P, T0, 37, seed=3)
    eph, times = check(ctx, t, [y], 1e-3, [P, P, P], [T0, T0, T0], [4, 4, 2], [1, 40, 1], curve=[0, 0, 0], label="gap")
    assert statuses(times, 0)[2] == 1 and statuses(times, 1)[2] != 1 and eph["n_timed"][0] == 4
    # L = 5 over the gap of 20: t[hi] - t[lo] = 24 / 64 exactly
    for span, seen in ((24 * DT, True), (23 * DT, False)):
        eph, times = check(ctx, t, [y], 1e-3, [P], [T0 + 10 * DT], [0], [1], widths=[5], span_max=[span], min_ses=-numpy.inf,
                           depth_min=0.0, label=("span", span))
        over = (times["index"][0] >= 248) & (times["index"][0] <= 251)
        assert over.any() == seen


def test_time_stamps_hit_exactly_and_half_way(ctx):
    """tc on a time stamp: that sample; tc half-way between two: the lower one.  Constant flux with one dip sample makes the
    held centre tell which sample was the nearest: with L = 3 and reach 1 the dip is reached only from one side."""
    n = 257
    t = series(n)
    y = numpy.ones(n)
    y[100] -= 0.01                                    # (a single low sample)
    P = 1000.0                                        # one epoch
    for T0, held in ((t[98], 99), (t[98] + DT / 2, 99), (t[97] + DT / 2, None), (t[99] + DT / 2, 100), (t[102] + DT / 2, 101),
                     (t[102], 101), (t[103], None)):
        eph, times = check(ctx, t, [y], 1e-3, [P], [T0], [0], [1], min_ses=0.0, label=("tc", T0))
        assert eph["n_epochs"][0] == 1
        if held is None:
            assert statuses(times) == [1]
        else:
            assert times["index"][0][0] == held, (T0, times["index"][0][0])


def test_ties_constant_flux_and_the_gates(ctx):
    """Box dips on constant flux wider than the window: equal q at several shifts, the first wins.  Constant flux: no window
    passes d > depth_min.  A dip at the reach's edge: the step leaves the sample (status 2).  Shallow dips: status 3."""
    n = 400
    t = series(n)
    P, T0 = 80 * DT, t[40]
    flat = dips(t, P, T0, 15, depth=5e-3, sigma=0)
    eph, times = check(ctx, t, [flat], 1e-3, [P, P], [T0, T0], [2, 3], [4, 4], curve=[0, 0], label="ties")
    assert eph["n_epochs"][0] == 5
    for f, L in ((0, 5), (1, 8)):
        # windows wholly inside the box [c - 7, c + 7] share N and D bit for bit: the first of them is held
        first = numpy.array([40, 120, 200, 280, 360]) - 7 + (L - 1) // 2
        expect_equal(times["index"][f][:5], numpy.maximum(first, numpy.array([40, 120, 200, 280, 360]) - 4), ("first", L))
    eph, times = check(ctx, t, [numpy.ones(n)], 1e-3, [P], [T0], [2], [4], label="constant")
    assert statuses(times) == [1] * 5 and eph["n_timed"][0] == 0 and numpy.isnan(eph["period"][0])
    eph, times = check(ctx, t, [numpy.ones(n)], 1e-3, [P], [T0], [2], [4], depth_min=1e-3, label="depth_min")
    # dips that begin beyond the reach: the best window is the last shift and the slope says "further"
    y = dips(t, P, T0, 9, depth=5e-3, seed=5, sigma=2e-4, shift=[7])
    eph, times = check(ctx, t, [y], 1e-3, [P], [T0], [2], [3], label="step")
    assert statuses(times).count(2) >= 3 and eph["n_timed"][0] <= 2
    assert numpy.isnan(times["time"][0][times["status"][0] == 2]).all() and numpy.isfinite(times["ses"][0][times["status"][0] == 2]).all()
    weak = dips(t, P, T0, 5, depth=1e-3, seed=6)
    eph, times = check(ctx, t, [weak], 1e-3, [P, P], [T0, T0], [2, 2], [2, 2], curve=[0, 0], min_ses=6.0, label="min_ses")
    assert statuses(times).count(3) >= 3
    eph, times = check(ctx, t, [weak], 1e-3, [P], [T0], [2], [2], min_ses=-numpy.inf, label="no gate")
    assert 3 not in statuses(times)


def test_zero_to_three_timed_epochs(ctx):
    """n_timed 0: no ephemeris; 1: none either; 2: a line without residuals; 3: chi^2 and the rest."""
    n = 400
    t = series(n)
    P, T0 = 100 * DT, t[50]                           # epochs at 50, 150, 250, 350
    y = numpy.ones((4, n)) + numpy.random.RandomState(4).normal(0, 2e-4, (4, n))
    for k in range(4):
        for e in range(k):
            y[k, 50 + 100 * e - 2: 50 + 100 * e + 3] -= 6e-3
    eph, times = check(ctx, t, y, 1e-3, numpy.full(4, P), numpy.full(4, T0), numpy.full(4, 2), numpy.full(4, 3), min_ses=10.0,
                       label="n_timed")
    expect_equal(eph["n_timed"], [0, 1, 2, 3], "n_timed")
    assert numpy.isnan(eph["period"][:2]).all() and numpy.isfinite(eph["period"][2:]).all()
    assert numpy.isfinite(eph["T0_err"][2:]).all() and numpy.isnan(eph["ttv_chi2"][:3]).all() and numpy.isfinite(eph["ttv_chi2"][3])
    assert numpy.isnan(eph["ttv_max_epoch"][2]) and eph["ttv_max_epoch"][3] in (0, 1, 2)
    assert abs(eph["period"][3] - P) < 3 * eph["period_err"][3] + 1e-12


def test_the_epoch_limit_and_bad_ephemerides(ctx):
    """n_epochs equal to max_epochs is timed, one more is status 2 with n_epochs reported; a period or T0 that is not finite,
    or a period <= 0, is status 1; an ephemeris without an epoch inside the series is status 2."""
    n = 300
    t = series(n)
    P = 24 * DT                                       # 13 epochs from t[0]: 299 // 24 + 1
    y = dips(t, P, t[0], 5, seed=7)
    nan, inf = numpy.nan, numpy.inf
    period = [P, P, nan, inf, 0.0, -1.0, P, P, P, 5000.0, 5e-324, 1e300]
    T0 = [t[0], t[0] - 24 * DT, 1.0, 1.0, 1.0, 1.0, nan, inf, -inf, 0.3, 1.0, 1.0]
    ones = numpy.ones(12, dtype=int)
    eph, times = check(ctx, t, [y], 1e-3, period, T0, 0 * ones, 2 * ones, curve=0 * ones, max_epochs=13, label="limit 13")
    expect_equal(eph["status"], [0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 0], "status")
    assert eph["n_epochs"][0] == 13 and eph["epoch_first"][1] == 1 and eph["n_epochs"][9] == 0 and eph["n_epochs"][10] == numpy.inf
    assert eph["n_epochs"][11] == 1 and times["time_linear"][11][0] == 1.0         # (one epoch of a period of 1e300 d)
    assert numpy.isnan(times["epoch"][2:11]).all() and not numpy.isnan(times["epoch"][:2]).any()
    eph, times = check(ctx, t, [y], 1e-3, period[:2], T0[:2], [0, 0], [2, 2], curve=[0, 0], max_epochs=12, label="limit 12")
    expect_equal(eph["status"], [2, 2], "one more")
    expect_equal(eph["n_epochs"], [13, 13], "reported")
    assert numpy.isnan(times["epoch"]).all() and numpy.isnan(eph["n_timed"]).all()


def test_units_threads_and_chunks(ctx):
    """40 epochs x 17 shifts (more units than the workgroup has threads), 3 epochs x 3 shifts (fewer than a wave), reach 4096
    (one epoch a chunk of the LDS, most shifts outside the series), reach 100 with 40 epochs (chunks of 40 epochs and a tail is
    not needed: 8193 // 201 = 40), reach 300 with 40 epochs (chunks of 13 epochs and a tail of 1), per-point dy throughout."""
    n = 650
    t = series(n)
    rng = numpy.random.RandomState(8)
    dy = rng.uniform(5e-4, 2e-3, (2, n))
    P40, P3 = 16 * DT, 300 * DT
    y = numpy.array([dips(t, P40, t[5], 5, seed=9), dips(t, P3, t[20], 37, seed=10)])
    period = [P40, P3, P3, P40, P40, P40]
    T0 = [t[5], t[20], t[20], t[5], t[5], t[5]]
    reach = [8, 1, 4096, 100, 300, 102]
    eph, times = check(ctx, t, y, dy, period, T0, [2, 4, 4, 1, 0, 3], reach, curve=[0, 1, 1, 0, 0, 0], label="units")
    expect_equal(eph["n_epochs"], [41, 3, 3, 41, 41, 41], "epochs")
    assert eph["n_timed"][0] >= 30 and eph["n_timed"][1] >= 2 and eph["n_timed"][2] >= 1


def test_candidates_curves_and_slabs(ctx):
    """Several candidates a curve, curves out of order, 1030 candidates (more than the slab of 1024), and max_epochs at the
    entry's limit (the slab is 64 candidates then; 3 are enough to see the records past n_epochs filled)."""
    n = 257
    t = series(n)
    rng = numpy.random.RandomState(11)
    P = 64 * DT
    y = numpy.array([dips(t, P, t[10 + 3 * i], 5, seed=20 + i) for i in range(5)])
    dy = numpy.full((5, n), 1e-3)
    n_fits = 1030
    curve = rng.randint(0, 5, n_fits)
    period = numpy.where(rng.uniform(size=n_fits) < 0.1, P / 2, P)
    T0 = t[10 + 3 * curve] + rng.randint(-2, 3, n_fits) * DT / 4
    row = rng.randint(0, 4, n_fits)
    reach = rng.randint(1, 6, n_fits)
    eph, times = check(ctx, t, y, dy, period, T0, row, reach, curve=curve, max_epochs=9, label="slabs")
    assert (eph["status"] == 0).all() and (eph["n_timed"] >= 2).sum() > 900
    again = ctx.transit_times(t, y, dy, period[1024:], T0[1024:], row[1024:], reach[1024:], WIDTHS, shapes_of(WIDTHS),
                              spans_of(WIDTHS), curve=curve[1024:], max_epochs=9)
    assert again[0].tobytes() == eph[1024:].tobytes() and again[1].tobytes() == times[1024:].tobytes()
    eph, times = check(ctx, t, y, dy, period[:3], T0[:3], row[:3], reach[:3], curve=[4, 0, 4], max_epochs=65536, label="65536")
    assert numpy.isnan(times["epoch"][:, 9:]).all()


def test_a_slab_that_ends_on_its_curve_slots(ctx):
    """n = 2^15 points: 256 MB of curves are 2^28 / (32 n) = 256 slots, and 300 candidates visit 257 curves, so the first slab
    ends where the 257th curve appears, not at a candidate count.  The whole call equals, byte for byte, the two calls on the
    candidates in front of that cut and behind it, and the statement next to the cut.  Every curve has a dip of its own depth
    at its own place at four epochs (flat elsewhere, one vectorised expression), so a curve in a wrong slot shows; curves
    100 .. 119 are first met in order, one copy of twenty rows."""
    n, n_curves, n_fits, P = 1 << 15, 257, 300, 8192 * DT
    t = series(n)
    rng = numpy.random.RandomState(21)
    move, depth = rng.randint(-40, 41, n_curves), 3e-3 + 1e-5 * numpy.arange(n_curves)
    y = numpy.ones((n_curves, n))
    y[numpy.arange(n_curves)[:, None, None],
      (4096 + move)[:, None, None] + 8192 * numpy.arange(4)[None, :, None] + numpy.arange(-2, 3)[None, None, :]] -= depth[:, None, None]
    dy = numpy.full((n_curves, n), 1e-3)
    others = rng.permutation(numpy.r_[0:100, 120:n_curves])
    curve = numpy.r_[others[:60], 100:120, others[60:]]
    for at in numpy.sort(rng.randint(1, n_curves, 30))[::-1]:      # repeats: 30 on the way, each after its first visit, ...
        curve = numpy.insert(curve, at, curve[rng.randint(0, at)])
    curve = numpy.r_[curve, rng.randint(0, n_curves, n_fits - len(curve))]        # ... and 13 behind the last curve
    assert len(curve) == n_fits and len(set(curve.tolist())) == n_curves
    slab, slot, runs = _lib.candidate_slabs(curve, n_fits, 256, n_fits)
    cut = int(numpy.flatnonzero(slab == 1)[0])
    assert slab[-1] == 1 and cut < n_fits and len(set(curve[:cut].tolist())) == 256 and runs[0] <= 256 - 19
    period, T0 = numpy.full(n_fits, P), t[4096 + move[curve]] + rng.randint(-2, 3, n_fits) * DT / 4
    row, reach = rng.randint(0, 4, n_fits), rng.randint(1, 6, n_fits)
    tables = (WIDTHS, shapes_of(WIDTHS), spans_of(WIDTHS))
    eph, times = ctx.transit_times(t, y, dy, period, T0, row, reach, *tables, curve=curve, max_epochs=4)
    assert (eph["n_epochs"] == 4).all() and (eph["n_timed"] >= 2).sum() > 250
    for part in (slice(0, cut), slice(cut, n_fits)):
        alone = ctx.transit_times(t, y, dy, period[part], T0[part], row[part], reach[part], *tables, curve=curve[part], max_epochs=4)
        assert alone[0].tobytes() == eph[part].tobytes() and alone[1].tobytes() == times[part].tobytes(), part
    near = slice(cut - 4, min(cut + 4, n_fits))
    want = spec.expected(t, y, dy, curve[near], period[near], T0[near], row[near], reach[near], tables[1], tables[2], max_epochs=4)
    for f in spec.EPHEMERIS_FIELDS:
        expect_equal(eph[near][f], want[0][f], ("cut", f))
    for f in spec.TIME_FIELDS:
        expect_equal(times[near][f], want[1][f], ("cut", f))


def test_two_contexts(ctx):
    n = 300
    t = series(n)
    y = dips(t, 50 * DT, t[7], 8, seed=12)
    args = (t, [y], numpy.full((1, n), 1e-3), [50 * DT, 25 * DT], [t[7], t[7]], [3, 1], [8, 2], WIDTHS, shapes_of(WIDTHS),
            spans_of(WIDTHS))
    one = ctx.transit_times(*args, curve=[0, 0], max_epochs=16)
    other = _lib.Context(0)
    try:
        two = other.transit_times(*args, curve=[0, 0], max_epochs=16)
        back = ctx.transit_times(*args, curve=[0, 0], max_epochs=16)
    finally:
        other.close()
    assert one[0].tobytes() == two[0].tobytes() == back[0].tobytes() and one[1].tobytes() == two[1].tobytes() == back[1].tobytes()
    assert one[0]["n_timed"][0] >= 4


def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; every TLS_E_ARG case returns before any device work with the outputs untouched."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = series(n)
    good = dict(t=t, y=numpy.ones((2, n)), dy=numpy.full((2, n), 1e-3), n_curves=2, curve=[1], period=[1.0], T0=[1.5], row=[1],
                reach=[2], n_fits=1, shape_values=numpy.ones(8), shape_offset=[0, 3], width=[3, 5], span_max=[0.1, 0.2],
                n_rows=2, depth_min=0.0, min_ses=3.0, max_epochs=4)
    eph = numpy.full(1, -7.0, dtype=_lib.EPHEMERIS_DTYPE)
    times = numpy.full((1, 4), -7.0, dtype=_lib.TRANSIT_TIME_DTYPE)

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "y", "dy", "period", "T0", "shape_values", "span_max")}
        i8 = {k: _lib._i8(a[k]) for k in ("curve", "row", "reach", "shape_offset", "width")}
        return lib.tls_transit_times(ctx._h, dp(f8["t"]), dp(f8["y"]), dp(f8["dy"]), len(f8["t"]), a["n_curves"], ip(i8["curve"]),
                                     dp(f8["period"]), dp(f8["T0"]), ip(i8["row"]), ip(i8["reach"]), a["n_fits"],
                                     dp(f8["shape_values"]), ip(i8["shape_offset"]), ip(i8["width"]), dp(f8["span_max"]),
                                     a["n_rows"], a["depth_min"], a["min_ses"], a["max_epochs"],
                                     eph.ctypes.data_as(ctypes.c_void_p), times.ctypes.data_as(ctypes.c_void_p))

    def untouched():
        return all((eph[k] == -7.0).all() for k in eph.dtype.names) and all((times[k] == -7.0).all() for k in times.dtype.names)

    assert call(n_fits=0) == 0 and untouched()
    assert lib.tls_transit_times(ctx._h, None, None, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, 0,
                                 0.0, 3.0, 1, None, None) == 0
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - DT
    bad_t = t.copy()
    bad_t[5] = nan
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(row=[2]), dict(row=[-1]), dict(reach=[0]), dict(reach=[4097]),
               dict(max_epochs=0), dict(max_epochs=65537), dict(width=[2, 5]), dict(width=[3, 4097]), dict(width=[5, 3]),
               dict(width=[3, 3]), dict(shape_offset=[0, -1]), dict(n_rows=0), dict(span_max=[0.1, inf]), dict(span_max=[-0.1, 0.2]),
               dict(span_max=[nan, 0.2]), dict(t=late), dict(t=bad_t), dict(min_ses=nan), dict(depth_min=-1e-9), dict(depth_min=inf),
               dict(depth_min=nan), dict(n_fits=-1), dict(n_curves=-1)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"transit times" in lib.tls_last_error(ctx._h), kw
    assert call() == 0 and eph["status"][0] == 0 and eph["n_epochs"][0] == 4 and not untouched()
    empty = ctx.transit_times(t, numpy.ones((2, n)), numpy.ones((2, n)), [], [], [], [], [3], [numpy.ones(3)], [0.1], curve=[])
    assert empty[0].shape == (0,) and empty[1].shape == (0, 1)


# ---- survey.transit_times and the pipeline --------------------------------------------------------------------------------
T = 3.0 + numpy.arange(600) / 48.0                    # 12.5 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))                   # period [d], a / R_star


def curve_of(s):
    rng = numpy.random.RandomState(1000 + s)
    f = numpy.ones(len(T))
    for per, a in PLANETS:
        tp = T[0] + rng.uniform(0.1, 0.9) * per
        f += transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3], "quadratic") - 1
    return f + rng.normal(0, 4e-4, len(T)) + 2e-3 * numpy.sin(T / 1.7 + s)


def expected_survey(flux, period, T0, duration, curve, search, min_ses, max_epochs, dy=None):
    """survey.transit_times stated with the spec: the rows _batch_inputs hands out, the table of transit_time_rows."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, dy_rows = survey._batch_inputs(T, flux, dy, dict(oversampling_factor=1))
    widths, span_max, row, reach = survey.transit_time_rows(T, period, duration, search)
    shapes = spec.shapes_of(widths, **inp["shape"])
    return spec.expected(T, y_rows, dy_rows, curve, period, T0, row, reach, shapes, span_max, 0.0, min_ses, max_epochs)


def equal_records(got, want, names, label):
    for k in names:
        expect_equal(got[k], want[k], (label, k))


@pytest.mark.parametrize("detrend", [None, 25])
def test_pipeline(ctx, detrend):
    """power_batch(peaks=3, peak_fits=True, transit_times=True) on 4 curves: the tt_ fields and the transit_times rows equal
    survey.transit_times on the fits' (period, T0, duration_days), which equals the statement; summary, peaks, fits and scans
    equal the call without the keyword bit for bit."""
    flux = numpy.array([curve_of(s) for s in range(4)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(context=ctx, peaks=3, peak_fits=True, phase_scan=True, detrend=detrend, **KW)
        summary, periods, pk = survey.power_batch(T, flux, transit_times=True, **more)
        without = survey.power_batch(T, flux, **more)
        searched = flux if detrend is None else survey.detrend_batch(flux, detrend, context=ctx)
    peaks, times = pk["peaks"], pk["transit_times"]
    max_epochs = survey._max_epochs(T, periods)
    assert times.shape == (4, 3, max_epochs) and times.dtype.names == survey.transit_time_fields()
    names = [k for k, _ in survey.TRANSIT_TIMES_PEAK_FIELDS]
    assert list(peaks.dtype.names[-len(names):]) == names
    # everything else of the call is untouched
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(periods, without[1], "periods")
    expect_equal(pk["n_peaks"], without[2]["n_peaks"], "n_peaks")
    assert peaks.dtype.names[:-len(names)] == without[2]["peaks"].dtype.names and "transit_times" not in without[2]
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    # the fitted peaks, against survey.transit_times and against the statement
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 8
    args = (peaks["period"][curve, rank], peaks["T0"][curve, rank], peaks["duration_days"][curve, rank])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eph, alone = survey.transit_times(T, searched, *args, curve=curve, max_epochs=max_epochs, context=ctx)
        auto = survey.transit_times(T, searched, *args, curve=curve, context=ctx)
    assert eph.dtype.names == survey.ephemeris_fields() and alone.dtype.names == survey.transit_time_fields()
    for name, source in survey.TRANSIT_TIMES_PEAK_FIELDS:
        expect_equal(peaks[name][curve, rank], eph[source], name)
    equal_records(times[curve, rank], alone, survey.transit_time_fields(), "rows")
    want_eph, want_times = expected_survey(searched, *args, curve, 1.0, 3.0, max_epochs)
    equal_records(eph, want_eph, spec.EPHEMERIS_FIELDS, "ephemeris")
    equal_records(alone, want_times, spec.TIME_FIELDS, "times")
    with numpy.errstate(all="ignore"):
        expect_equal(alone["oc"], alone["time"] - (eph["T0"][:, None] + alone["epoch"] * eph["period"][:, None]), "oc")
    # max_epochs=None: the largest epoch count among the candidates
    assert auto[1].shape[1] == int(eph["n_epochs"].max()) <= max_epochs
    equal_records(auto[1], alone[:, :auto[1].shape[1]], survey.transit_time_fields(), "auto")
    # peaks without a fit: status 1 and NaN
    rest = peaks["status"] != 0
    assert (peaks["tt_status"][rest] == 1).all() and numpy.isnan(peaks["tt_period"][rest]).all()
    assert numpy.isnan(times["epoch"][rest]).all()
    # the two injected planets are among the timed candidates (what the times say about them is the host tests' business: the
    # statement is checked there on white noise, where time_err holds; here the rows carry a slow variation, or went through a
    # median filter as wide as five transits)
    found = sum(int((numpy.abs(peaks["period"] - per) < 0.02 * per)[peaks["tt_n_timed"] >= 3].sum()) for per, _ in PLANETS)
    assert found >= 6


def test_survey_call_options(ctx):
    """search, min_ses, gap_tolerance, transit_depth_min, per-point dy and one row [n] reach the device as the statement has
    them."""
    flux = numpy.array([curve_of(s) for s in range(2)])
    rng = numpy.random.RandomState(3)
    dy = rng.uniform(3e-4, 6e-4, flux.shape)
    period, T0, duration = [1.9, 3.1, 1.9], [3.4, 4.0, 3.9], [0.09, 0.11, 0.02]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eph, times = survey.transit_times(T, flux, period, T0, duration, curve=[0, 1, 1], dy_batch=dy, search=2.0, min_ses=5.0,
                                          context=ctx)
        inp, y_rows, dy_rows = survey._batch_inputs(T, flux, dy, dict(oversampling_factor=1))
        one = survey.transit_times(T, flux[0], [1.9], [3.4], [0.09], search=2.0, min_ses=5.0, max_epochs=times.shape[1], context=ctx)
    widths, span_max, row, reach = survey.transit_time_rows(T, period, duration, 2.0)
    assert widths.tolist() == [3, 4, 5] and reach.tolist() == [8, 10, 6]
    want = spec.expected(T, y_rows, dy_rows, [0, 1, 1], period, T0, row, reach, spec.shapes_of(widths, **inp["shape"]), span_max,
                         0.0, 5.0, times.shape[1])
    equal_records(eph, want[0], spec.EPHEMERIS_FIELDS, "dy")
    equal_records(times, want[1], spec.TIME_FIELDS, "dy")
    assert one[0].shape == (1,) and one[1].shape == (1, times.shape[1]) and one[0]["n_epochs"][0] == eph["n_epochs"][0]
