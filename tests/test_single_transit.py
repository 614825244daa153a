"""Single-transit events on the device (survey.single_transits / tls_single_transits) against tests/single_transit_spec.py
bit for bit, every field of every record and every plane: at the edges of the statistic kernel (its tile of centres, the
first and last valid centre of odd and even rows, the widest row, a row wider than the series), of the statement (gaps hit
exactly, islands, constant flux, ties, the selection's options) and of the call (batches, slabs, two contexts, detrend=,
argument errors)."""
import ctypes
import warnings

import numpy
import pytest

import single_transit_spec as spec
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu

TILE = _lib.SINGLE_TILE
WIDTHS = [3, 4, 5, 8, 37, 64, 65, 257]
SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")
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


def spans_of(t, widths, gap_tolerance=0.5):
    dt = float(numpy.median(numpy.diff(t)))
    return [(int(L) - 1) * dt * (1 + gap_tolerance) for L in widths]


def series(n, gap_at=None, gap=0):
    """n time stamps at 1/64 d (every difference exact), `gap` cadences missing in front of index gap_at."""
    t = 1.0 + numpy.arange(n + gap) / 64.0
    return t if gap_at is None else numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def curves(n, n_curves, seed, dips=((0.3, 9, 4e-3), (0.7, 30, 2e-3))):
    """Noise of 1e-3 and box dips (place as a fraction of n, samples, depth), each curve's a little elsewhere."""
    rng = numpy.random.RandomState(seed)
    y = 1 + rng.normal(0, 1e-3, (n_curves, n))
    for i in range(n_curves):
        for place, width, depth in dips:
            at = int(place * n) + 3 * i
            y[i, at: at + width] -= depth
    return y


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check(ctx, t, y, dy, widths, span_max=None, label="", **kw):
    """ctx.single_transits of the rows equals the statement: every field of every record, the counts and the three planes;
    what the device returned."""
    y = numpy.atleast_2d(y)
    dy = numpy.broadcast_to(numpy.asarray(dy, dtype=float), y.shape) if numpy.ndim(dy) < 2 else dy
    shapes = shapes_of(widths)
    span_max = spans_of(t, widths) if span_max is None else span_max
    got = ctx.single_transits(t, y, dy, widths, shapes, span_max, with_arrays=True, **kw)
    want = spec.expected(t, y, dy, widths, shapes, span_max, **kw)
    assert got[0].dtype.names == spec.FIELDS and got[0].shape == want[0].shape == (len(y), kw.get("k", 8))
    for f in spec.FIELDS:
        expect_equal(got[0][f], want[0][f], (label, f))
    for a, b, name in zip(got[1:], want[1:], ("n_events", "ses", "row", "depth")):
        expect_equal(a, b, (label, name))
    assert got[3].dtype == numpy.int64
    without = ctx.single_transits(t, y, dy, widths, shapes, span_max, **kw)
    assert len(without) == 2 and without[0].tobytes() == got[0].tobytes() and without[1].tobytes() == got[1].tobytes()
    return got


@pytest.mark.parametrize("n", [64, TILE - 1, TILE, TILE + 1, 2 * TILE + 907])
def test_series_lengths_around_the_tile(ctx, n):
    """Rows of odd and even widths, two of them wider than the halo of a neighbouring tile is long: the first valid centre is
    (L - 1) // 2, the last n - 1 - L // 2, whatever tile they fall into; rows wider than the series have none."""
    t = series(n)
    ev, n_events, ses, row, depth = check(ctx, t, curves(n, 2, n), 1e-3, WIDTHS, label="n %d" % n, k=6)
    fits = [L for L in WIDTHS if L <= n]
    assert numpy.isnan(ses[:, : (fits[0] - 1) // 2]).all() and numpy.isnan(ses[:, n - fits[0] // 2:]).all()
    assert set(numpy.unique(row)) <= set(range(-1, len(fits))) and (n_events > 0).all()
    # every row reaches its first and its last valid centre: alone, each holds exactly those
    for r, L in enumerate(WIDTHS):
        alone = ctx.single_transits(t, numpy.full(n, 0.999), numpy.full(n, 1e-3), [L], shapes_of([L]), [10.0], with_arrays=True)
        held = numpy.flatnonzero(alone[3][0] >= 0)
        if L > n:
            assert len(held) == 0 and alone[1][0] == 0
        else:
            assert held[0] == (L - 1) // 2 and held[-1] == n - 1 - L // 2 and len(held) == n - L + 1, (n, L)


def test_the_widest_row(ctx):
    """Width 4096 (the limit) on 4500 points: the halo of a tile is 2047 slots in front and 2048 behind."""
    n = 4500
    t = series(n)
    y = curves(n, 1, 5, dips=((0.4, 1500, 1e-3),))
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, [3, 4096], label="widest", k=4)
    assert (row[0] == 1).sum() > 0 and numpy.flatnonzero(row[0] == 1).max() <= n - 1 - 2048
    assert numpy.flatnonzero(row[0] == 1).min() >= 2047
    assert ev["width"][0, 0] == 4096


def test_a_row_wider_than_the_series(ctx):
    n = 100
    t = series(n)
    y = curves(n, 2, 6, dips=((0.3, 9, 4e-3),))
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, [101], label="too wide")
    assert (n_events == 0).all() and numpy.isnan(ses).all() and (row == -1).all() and (ev["index"] == -1).all()
    assert numpy.isnan(ev["time"]).all()
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, [9, 100, 101], label="one too wide")
    assert (row < 2).all() and (n_events > 0).all()


def test_gaps_hit_exactly(ctx):
    """Every difference of t is exact, so a whole window of row L spans (L - 1) / 64 to the bit: with span_max equal to it
    the window counts, with span_max one ulp below it does not, and a window over the gap (3 cadences missing) never does."""
    n = 700
    t = series(n, 300, 3)
    y = curves(n, 2, 8, dips=((0.2, 9, 4e-3), (0.42, 12, 4e-3)))          # the second dip lies across the gap
    widths = [5, 9, 33]
    exact = [(L - 1) / 64.0 for L in widths]
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, widths, span_max=exact, label="span hit")
    over = (numpy.arange(n) >= 300 - 2) & (numpy.arange(n) < 300 + 2)     # (centres whose width-5 window holds the gap)
    assert numpy.isnan(ses[:, over]).all() and (row[:, 250:296] >= 0).any()
    below = [exact[0], numpy.nextafter(exact[1], 0.0), exact[2]]
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, widths, span_max=below, label="one ulp below")
    assert (row != 1).all() and (row == 0).any() and (row == 2).any()
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, widths, span_max=[0.0, 0.0, 0.0], label="span 0")
    assert (n_events == 0).all()


def test_islands_shorter_than_every_row(ctx):
    """Four points, then four cadences missing, again and again: no window of 5 or 8 samples is whole under the default
    gap tolerance of half a window."""
    k = numpy.arange(600)
    t = 1.0 + (k + 4 * (k // 4)) / 64.0
    y = curves(600, 2, 9)
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, [5, 8], label="islands")
    assert (n_events == 0).all() and numpy.isnan(ses).all() and numpy.isnan(depth).all() and (row == -1).all()
    ev, n_events, ses, row, depth = check(ctx, t, y, 1e-3, [3, 5, 8], label="islands, width 3")
    assert (row <= 0).all() and (row == 0).any()


def test_per_point_dy_against_the_default(ctx):
    """survey.single_transits with a dy_batch and without one: the rows are those a search of the batch gets
    (survey._batch_inputs), and the two results differ."""
    n = 1000
    t = series(n, 400, 40)
    flux = curves(n, 3, 10)
    dy = numpy.random.RandomState(11).uniform(0.5, 2.0, flux.shape) * 1e-3
    results = []
    for dy_batch in (None, dy):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = survey.single_transits(t, flux, dy_batch, context=ctx, with_arrays=True, **SHAPE)
            inp, y_rows, dy_rows = survey._batch_inputs(t, flux, dy_batch, dict(SHAPE, oversampling_factor=1))
        widths = survey.single_transit_widths(t)
        want = spec.expected(t, y_rows, dy_rows, widths, spec.shapes_of(widths, **inp["shape"]), spans_of(t, widths))
        assert got[0].dtype.names == survey.single_event_fields()
        for f in spec.FIELDS:
            expect_equal(got[0][f], want[0][f], ("dy" if dy_batch is not None else "no dy", f))
        expect_equal(got[0]["duration_days"], want[0]["width"] * (1 / 64.0), "duration_days")
        for a, b in zip(got[1:], want[1:]):
            expect_equal(a, b, "planes")
        results.append(got)
    assert not numpy.array_equal(results[0][2], results[1][2], equal_nan=True)


def test_constant_flux_holds_nothing(ctx):
    n = 2 * TILE + 50
    ev, n_events, ses, row, depth = check(ctx, series(n), numpy.ones((2, n)), 1e-3, WIDTHS, label="constant")
    assert (n_events == 0).all() and numpy.isnan(ses).all() and (row == -1).all() and numpy.isnan(depth).all()
    # a constant below 1 is a dip of the same depth everywhere: every whole window holds the row of the largest sum of weights
    ev, n_events, ses, row, depth = check(ctx, series(n), numpy.full((1, n), 0.75), 1e-3, [3, 8], label="constant 0.75", depth_min=0.2)
    assert (row[0, 4: n - 4] == 1).all() and n_events[0] > 0
    ev, n_events, ses, row, depth = check(ctx, series(n), numpy.full((1, n), 0.75), 1e-3, [3, 8], label="depth_min", depth_min=0.3)
    assert n_events[0] == 0


def test_ties_report_the_first(ctx):
    """Two bit-identical dips in flat flux: the same ses at both, the earlier one is rank 1; and inside a flat-bottomed dip
    many centres tie, of which the lowest index is taken."""
    n = 3 * TILE
    y = numpy.ones((1, n))
    dip = numpy.array([0.999, 0.998, 0.997, 0.997, 0.997, 0.997, 0.997, 0.998, 0.999])
    y[0, 100:109] = dip
    y[0, 500:509] = dip
    ev, n_events, ses, row, depth = check(ctx, series(n), y, 1e-3, [3, 5, 9], label="ties")
    assert n_events[0] == 2 and ev["ses"][0, 0] == ev["ses"][0, 1] and ev["index"][0, 0] + 400 == ev["index"][0, 1]
    expect_equal(ses[0, 90:120], ses[0, 490:520], "the two dips")
    y[0, 100:109] = 0.997
    y[0, 500:509] = 0.997
    ev, n_events, ses, row, depth = check(ctx, series(n), y, 1e-3, [3], label="flat ties", separation=0.0, k=16)
    assert ev["index"][0, 0] == 101 and (ses[0, 101:108] == ses[0, 101]).all()


def test_selection_options(ctx):
    n = 1500
    t = series(n, 600, 30)
    y = curves(n, 3, 12)
    base = check(ctx, t, y, 1e-3, WIDTHS, label="k 32", k=32, min_ses=2.5)
    assert (base[1] < 32).all() and (base[1] >= 2).all()                    # (k larger than the events there are)
    assert (base[0]["index"][:, -1] == -1).all()
    cut = check(ctx, t, y, 1e-3, WIDTHS, label="min_ses", k=32, min_ses=8.0)
    assert (cut[1] < base[1]).all() and (cut[1] >= 1).all()
    assert numpy.nanmin(cut[0]["ses"]) >= 8.0
    one = check(ctx, t, y, 1e-3, WIDTHS, label="k 1", k=1, min_ses=-numpy.inf)
    expect_equal(one[0]["ses"][:, 0], base[0]["ses"][:, 0], "rank 1")
    wide = check(ctx, t, y, 1e-3, WIDTHS, label="separation 2", k=32, separation=2.0, min_ses=2.5)
    none = check(ctx, t, y, 1e-3, WIDTHS, label="separation 0", k=32, separation=0.0, min_ses=2.5)
    assert (wide[1] <= base[1]).all() and (none[1] >= base[1]).all() and (none[1] > wide[1]).any()
    check(ctx, t, y, 1e-3, WIDTHS, label="separation 1e300", k=4, separation=1e300)
    check(ctx, t, y, 1e-3, WIDTHS, label="depth_min", k=8, depth_min=1e-3)


def test_a_batch_equals_its_curves_one_by_one(ctx):
    n = TILE + 300
    t = series(n, 200, 10)
    y = curves(n, 33, 13)
    dy = numpy.random.RandomState(14).uniform(0.5, 2.0, y.shape) * 1e-3
    widths = [3, 8, 37]
    whole = check(ctx, t, y, dy, widths, label="33 curves", k=5)
    for i in (0, 1, 31, 32):
        alone = ctx.single_transits(t, y[i], dy[i], widths, shapes_of(widths), spans_of(t, widths), k=5, with_arrays=True)
        for a, b in zip(alone, whole):
            assert a[0].tobytes() == b[i].tobytes(), i


def test_the_longest_series_in_two_slabs(ctx):
    """2^20 points (the limit: the selection's mask fills 128 KiB of LDS) and 8 curves, one more than a slab of 256 MB
    holds; k = 1, so the one event is numpy's first argmax of the statement's plane."""
    n = _lib.SINGLE_MAX_POINTS
    t = 1.0 + numpy.arange(n) / 1024.0
    y = 1 + numpy.random.RandomState(15).normal(0, 1e-3, (8, n))
    for i in range(8):
        y[i, n - 5000 - 7 * i: n - 4997 - 7 * i] -= 1e-2
    dy = numpy.full(y.shape, 1e-3)
    shapes = shapes_of([3])
    ev, n_events, ses, row, depth = ctx.single_transits(t, y, dy, [3], shapes, [1.0], k=1, with_arrays=True)
    want = spec.statistic(t, y, dy, [3], shapes, [1.0])
    for a, b, name in zip((ses, row, depth), want, ("ses", "row", "depth")):
        expect_equal(a, b, name)
    best = numpy.nanargmax(want[0], axis=1)
    expect_equal(ev["index"][:, 0], best, "index")
    expect_equal(ev["ses"][:, 0], want[0][numpy.arange(8), best], "ses of the event")
    expect_equal(ev["t_first"][:, 0], t[best - 1], "t_first")
    assert (n_events == 1).all() and (abs(best - (n - 4999 - 7 * numpy.arange(8))) <= 1).all()


def test_two_contexts_equal_one(ctx):
    n = 900
    t = series(n, 400, 40)
    flux = curves(n, 5, 16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = survey.single_transits(t, flux, context=ctx, with_arrays=True, k=4, **SHAPE)
        two = survey.single_transits(t, flux, devices=[0, 0], with_arrays=True, k=4, **SHAPE)
    assert len(one) == len(two) == 5
    for a, b in zip(one, two):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = survey.single_transits(t, flux, devices=[0, 0], k=4, **SHAPE)        # (no planes to join)
    assert len(plain) == 2 and plain[0].tobytes() == one[0].tobytes() and plain[1].tobytes() == one[1].tobytes()


def test_detrend_equals_the_call_on_detrended_rows(ctx):
    n = 900
    t = series(n)
    flux = curves(n, 3, 17) * (1 + 0.01 * numpy.sin(t / 3.0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flat = survey.detrend_batch(flux, 25, context=ctx)
        direct = survey.single_transits(t, flat, context=ctx, with_arrays=True, **SHAPE)
        inside = survey.single_transits(t, flux, detrend=25, context=ctx, with_arrays=True, **SHAPE)
        raw = survey.single_transits(t, flux, context=ctx, with_arrays=True, **SHAPE)
    for a, b in zip(direct, inside):
        assert a.tobytes() == b.tobytes()
    assert raw[2].tobytes() != inside[2].tobytes()


def test_argument_errors_of_the_c_entry_leave_the_outputs_untouched(ctx):
    n, k = 300, 4
    t = series(n)
    y, dy = numpy.ascontiguousarray(curves(n, 2, 18)), numpy.full((2, n), 1e-3)
    good = dict(t=t, n=n, n_curves=2, values=numpy.concatenate(shapes_of([3, 5])), offset=numpy.array([0, 3], dtype=numpy.int64),
                width=numpy.array([3, 5], dtype=numpy.int64), span=numpy.array([0.1, 0.2]), n_rows=2, depth_min=0.0, k=k,
                min_ses=0.0, separation=0.5)
    lib = ctx._lib

    def call(**kw):
        a = dict(good, **kw)
        events = numpy.full((2, a["k"] if 1 <= a["k"] <= 32 else 4, 8), 7.0)
        n_events = numpy.full(2, 77, dtype=numpy.int64)
        ses, depth, row = numpy.full((2, n), 7.0), numpy.full((2, n), 7.0), numpy.full((2, n), 77, dtype=numpy.int64)
        rc = lib.tls_single_transits(ctx._h, _lib._dp(a["t"]), _lib._dp(y), _lib._dp(dy), a["n"], a["n_curves"],
                                     _lib._dp(a["values"]), _lib._ip(a["offset"]), _lib._ip(a["width"]), _lib._dp(a["span"]),
                                     a["n_rows"], a["depth_min"], a["k"], a["min_ses"], a["separation"],
                                     events.ctypes.data_as(ctypes.c_void_p), _lib._ip(n_events), _lib._dp(ses), _lib._ip(row),
                                     _lib._dp(depth))
        touched = not ((events == 7.0).all() and (n_events == 77).all() and (ses == 7.0).all() and (depth == 7.0).all()
                       and (row == 77).all())
        return rc, touched

    assert call() == (0, True)
    assert call(n_curves=0) == (0, False)
    i64 = lambda *v: numpy.array(v, dtype=numpy.int64)
    bad = [dict(width=i64(5, 3)), dict(width=i64(3, 3)), dict(width=i64(2, 5)), dict(width=i64(3, 4097)), dict(k=0), dict(k=33),
           dict(n_curves=-1), dict(n_rows=-1), dict(n_rows=0), dict(n=-1), dict(n=0), dict(n=(1 << 20) + 1),
           dict(depth_min=-1e-9), dict(depth_min=numpy.inf), dict(depth_min=numpy.nan),
           dict(separation=-0.5), dict(separation=numpy.inf), dict(separation=numpy.nan),
           dict(span=numpy.array([0.1, -0.2])), dict(span=numpy.array([numpy.nan, 0.2])), dict(span=numpy.array([0.1, numpy.inf])),
           dict(min_ses=numpy.nan), dict(offset=i64(0, -3)),
           dict(t=numpy.ascontiguousarray(t[::-1])), dict(t=numpy.where(numpy.arange(n) == 9, numpy.nan, t))]
    for kw in bad:
        assert call(**kw) == (-1, False), kw                # (TLS_E_ARG)
        assert b"single transits" in lib.tls_last_error(ctx._h), kw
    assert call() == (0, True)                               # (the context still works)
