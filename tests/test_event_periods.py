"""Event periods on the device (survey.event_periods / tls_event_periods) against tests/event_periods_spec.py bit for bit, every
field of both records: at the edges of the plane kernel's tile and of the series, on both memory paths of the alias kernel, at a
gap (epochs on its edge samples, the offset met exactly and missed by one ulp, windows over it, an alias whose other epochs all
fall into it), at the alias limit and the pass boundary of a thread per alias, for every status, ties, no veto, slabs and groups,
Julian dates, two contexts and two device slices, detrending, poisoned memory and the C entry's argument errors.

Time stamps are multiples of 1/64 d, so every time difference is exact."""
import ctypes

import numpy
import pytest

import event_periods_spec as spec
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu

WIDTHS = [3, 4, 8, 37, 65]
SHAPE = spec.DEFAULT_SHAPE
DT = 1 / 64.0
TILE = _lib.ALIAS_TILE
_SHAPES = {}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def shapes_of(widths):
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


def curve_with(n, events, seed=0, sigma=1e-3, depth=6e-3):
    """Noise of `sigma` and a dip of `depth` over the window of every (centre, width) of `events`."""
    y = 1 + numpy.random.RandomState(seed).normal(0, sigma, n) if sigma else numpy.ones(n)
    for c, L in events:
        lo = c - (L - 1) // 2
        y[max(lo, 0):max(lo + L, 0)] -= depth
    return y


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check(ctx, t, y, dy, curve, ia, ib, row, reach, offset, period_min, widths=WIDTHS, label="", **kw):
    """ctx.event_periods of the pairs equals the statement in every field of both records, the ranks past n_evaluated hold NaN
    and with_aliases=False gives the same pair bytes; what the device returned."""
    y = numpy.atleast_2d(y)
    dy = numpy.broadcast_to(numpy.asarray(dy, dtype=float), y.shape) if numpy.ndim(dy) < 2 else dy
    shapes, span_max = shapes_of(widths), spans_of(widths)
    kw.setdefault("max_aliases", 32)
    offset = numpy.broadcast_to(numpy.asarray(offset, dtype=float), numpy.shape(curve))
    args = (t, y, dy, curve, ia, ib, row, reach, offset, widths, shapes, span_max, period_min)
    got = ctx.event_periods(*args, **kw)
    want = spec.expected(t, y, dy, curve, ia, ib, row, reach, offset, shapes, span_max, period_min, **kw)
    assert got[0].dtype.names == spec.PAIR_FIELDS and got[1].dtype.names == spec.ALIAS_FIELDS
    assert got[0].shape == want[0].shape == (len(curve),) and got[1].shape == want[1].shape == (len(curve), kw["max_aliases"])
    for f in spec.PAIR_FIELDS:
        expect_equal(got[0][f], want[0][f], (label, f))
    for f in spec.ALIAS_FIELDS:
        expect_equal(got[1][f], want[1][f], (label, f))
    done = numpy.where(got[0]["status"] == 0, got[0]["n_evaluated"], 0)
    past = numpy.arange(kw["max_aliases"])[None, :] >= done[:, None]
    assert all(numpy.isnan(got[1][f][past]).all() and not numpy.isnan(got[1]["period"][~past]).any() for f in spec.ALIAS_FIELDS)
    bare = ctx.event_periods(*args, with_aliases=False, **kw)
    assert bare[1] is None and bare[0].tobytes() == got[0].tobytes()
    return got


@pytest.mark.parametrize("n", [64, TILE - 1, TILE, TILE + 1, 2 * TILE + 907])
def test_the_tile_edges_and_the_ends_of_the_series(ctx, n):
    """Events on the first and the last valid centre of an odd and an even row, every row, and a row wider than the series."""
    t = series(n)
    last3, last4 = n - 1 - 1, n - 1 - 2                              # the last centre whose window of 3, of 4 samples is whole
    mid = [(n // 4, n - n // 4, r) for r in (2, 3, 4)]
    y = curve_with(n, [(1, 3), (last3, 3), (1, 4), (last4, 4)] + [(c, WIDTHS[r]) for a, b, r in mid for c in (a, b)], seed=n)
    pairs = [(1, last3, 0), (1, last4, 1), (0, n - 1, 0), (2, last3 - 1, 1)] + mid
    ia, ib, row = (numpy.array(v) for v in zip(*pairs))
    got = check(ctx, t, y, 1e-3, numpy.zeros(len(pairs), dtype=int), ia, ib, row, numpy.full(len(pairs), 2), 2.5 * DT,
                (n - 4) * DT / 20.5, label=n)
    assert got[0]["status"][0] == 0 and got[0]["status"][1] == 0 and got[0]["n_evaluated"][0] == 20
    if n == 64:
        assert got[0]["status"][6] == 2                                  # a row of 65 samples: no whole window


@pytest.mark.parametrize("n", [_lib.ALIAS_LDS_POINTS - 1, _lib.ALIAS_LDS_POINTS, _lib.ALIAS_LDS_POINTS + 1])
def test_both_memory_paths(ctx, n):
    """The series and the plane in the LDS up to ALIAS_LDS_POINTS, in device memory above: the same bits as the statement."""
    t = series(n)
    ca, cb = 700, n - 900
    y = curve_with(n, [(ca, 8), (cb, 8), (ca + (cb - ca) // 2, 8)], seed=n)
    got = check(ctx, t, y, 1e-3, [0, 0], [ca, ca + 1], [cb, cb], [0, 0], [2, 3], [2.5 * DT, 3.5 * DT], (cb - ca) * DT / 8.5,
                widths=[8], max_aliases=8, label=n)
    assert got[0]["status"].tolist() == [0, 0] and got[0]["n_evaluated"].tolist() == [8, 8]
    assert got[1]["n_covered"][0, 1] == 3 and got[1]["n_seen"][0, 1] == 3          # k = 2 meets the dip half-way


def test_a_gap(ctx):
    """600 samples with 200 cadences missing behind index 299 (cadences 0..299 and 500..799)."""
    n, L = 600, 8
    t = series(n, 300, 200)
    y = curve_with(n, [(c, L) for c in (100, 497, 500, 120, 480)], seed=3)
    # index 497 is cadence 697 and index 500 cadence 700.  From cadence 100 that is 597 = 3 * 199 and 600 = 3 * 200, so alias 3
    # lands on cadence 299 (the last sample in front of the gap) and on 498 (in the gap), or on 300 (in the gap) and on 500 (the
    # first sample behind it).  The first whole window of 3 samples behind the gap is centred on cadence 501, three cadences
    # from 498: an offset of 3 cadences meets it exactly
    ia, ib = [100, 100, 100, 100, 120], [497, 497, 497, 500, 480]
    exact = 3 * DT
    offset = [2.5 * DT, exact, numpy.nextafter(exact, 0.0), 2.5 * DT, 2.5 * DT]
    got = check(ctx, t, y, 1e-3, [0] * 5, ia, ib, [2, 0, 0, 2, 2], [2] * 5, offset, 40 * DT, label="gap")
    pairs, aliases = got
    assert pairs["status"].tolist() == [0] * 5
    assert aliases["period"][0, 2] == 199 * DT and aliases["period"][3, 2] == 200 * DT
    # the epoch on cadence 498: covered by the centre three cadences away while the offset reaches it, not one ulp below
    assert aliases["n_covered"][1, 2] == aliases["n_covered"][2, 2] + 1
    # cadence 120 to 680, alias 2: the only other epoch inside the series is cadence 400, in the gap
    assert numpy.isnan(aliases["worst_sigma"][4, 1]) and aliases["n_covered"][4, 1] == 2 and aliases["n_epochs"][4, 1] == 3
    assert pairs["n_allowed"][4] >= 1
    # windows over the gap are no windows: an event whose window would cross it is uncovered
    over = check(ctx, t, y, 1e-3, [0], [298], [400], [2], [1], 1.5 * DT, 40 * DT, label="over the gap")
    assert over[0]["status"][0] == 2 and numpy.isnan(over[0]["pair_mes"][0])


def test_the_alias_limit_and_every_status(ctx):
    n = 700
    t = series(n)
    t[40] = t[39]                                                        # (two samples share a time stamp)
    y = curve_with(n, [(150, 8), (470, 8)], seed=5)
    y[596:604] += 8e-3                                                   # a bump
    y[636:644] += 8e-3
    dT = 320 * DT
    for k_hi, status in ((9, 0), (10, 0), (11, 0), (0, 3)):
        got = check(ctx, t, y, 1e-3, [0], [150], [470], [2], [2], 2.5 * DT, dT / (k_hi + 0.5), max_aliases=10, label=k_hi)
        assert got[0]["status"][0] == status and got[0]["n_aliases"][0] == k_hi and got[0]["n_evaluated"][0] == min(k_hi, 10)
    got = check(ctx, t, y, 1e-3, [0, 0, 0], [39, 600, 150], [40, 640, 470], [0, 2, 2], [1, 1, 2], [1.5 * DT, 0.0, 2.5 * DT], 0.5,
                veto_sigma=numpy.inf, label="statuses")
    assert got[0]["status"].tolist() == [1, 2, 0] and got[0]["dT"][0] == 0 and got[0]["pair_mes"][1] < 0
    assert got[0]["n_allowed"][2] == got[0]["n_evaluated"][2] == 10 and got[0]["shortest_k"][2] == 10      # inf: no veto
    # constant flux: every q is 0 and the pair shows no dip; constant but for the two events: the epochs tie at q = 0, the first
    # shift is held and the smallest k wins equal mes
    flat = check(ctx, t, numpy.ones(n), 1e-3, [0], [150], [470], [2], [2], 2.5 * DT, 0.5, label="constant")
    assert flat[0]["status"][0] == 2 and flat[0]["pair_mes"][0] == 0
    quiet = curve_with(n, [(150, 8), (470, 8)], sigma=0)
    check(ctx, t, quiet, 1e-3, [0], [150], [470], [2], [2], 2.5 * DT, 0.5, veto_sigma=1e9, label="ties")


@pytest.mark.parametrize("count", [255, 256, 257])
def test_the_pass_boundary_of_a_thread_per_alias(ctx, count):
    n = 1400
    t = series(n)
    y = curve_with(n, [(50, 4), (1335, 4)], seed=count)
    got = check(ctx, t, y, 1e-3, [0], [50], [1335], [1], [1], 1.5 * DT, 1285 * DT / (count + 0.5), max_aliases=512, label=count)
    assert got[0]["n_evaluated"][0] == count and got[0]["status"][0] == 0


def test_slabs_groups_and_shuffled_curves(ctx):
    """1030 pairs over three curves at n = 64: more than one slab, pairs that share a (curve, row) group, a curve with two rows."""
    n, m = 64, 1030
    t = series(n)
    rng = numpy.random.RandomState(11)
    y = numpy.stack([curve_with(n, [(10, 3), (40, 3), (25, 4)], seed=s) for s in range(3)])
    dy = rng.uniform(5e-4, 2e-3, (3, n))
    curve = rng.randint(0, 3, m)
    row = numpy.where(curve == 1, rng.randint(0, 2, m), 0)
    ia = rng.randint(1, 30, m)
    ib = ia + rng.randint(1, 30, m)
    got = check(ctx, t, y, dy, curve, ia, ib, row, rng.randint(1, 4, m), rng.randint(0, 5, m) * DT, 4 * DT, max_aliases=8,
                label="slabs")
    assert set(got[0]["status"].tolist()) >= {0, 2}


def test_julian_dates(ctx):
    n = 500
    t = series(n, 200, 60) + 2457000.0
    y = curve_with(n, [(90, 8), (410, 8), (250, 8)], seed=8)
    got = check(ctx, t, y, 1e-3, [0, 0], [90, 90], [410, 250], [2, 2], [2, 2], 2.5 * DT, 30 * DT, label="JD")
    assert got[0]["status"].tolist() == [0, 0]


def _survey_case(n=700, seed=2):
    t = series(n, 400, 100)
    flux = numpy.stack([curve_with(n, [(60, 8), (260, 8), (560, 8)], seed=seed + s, depth=8e-3) for s in range(4)])
    flux *= 1 + 2e-3 * numpy.sin(numpy.arange(n) / 90.0)[None, :]
    return t, flux


def test_two_contexts_and_two_device_slices(ctx):
    t, flux = _survey_case()
    pairs = ([0, 0, 1, 2, 3, 3], [60, 60, 60, 260, 60, 260], [260, 560, 560, 560, 260, 560], [1, 1, 1, 1, 0, 1])
    kw = dict(pairs=pairs, widths=[4, 8], period_min=0.4, max_aliases=24)
    one = survey.event_periods(t, flux, context=ctx, **kw)
    other = _lib.Context(0)
    try:
        two = survey.event_periods(t, flux, context=other, **kw)
    finally:
        other.close()
    both = survey.event_periods(t, flux, devices=[0, 0], **kw)
    for got in (two, both):
        assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
    assert one[0]["status"].tolist() == [0] * 6 and one[0]["curve"].tolist() == pairs[0]
    assert one[1]["k"][0].tolist() == list(range(1, 25)) and one[1].dtype.names[:2] == ("k", "allowed")
    with numpy.errstate(invalid="ignore"):
        want = (one[1]["k"] <= one[0]["n_evaluated"][:, None]) & ~(one[1]["worst_sigma"] > 3.0)
    assert (one[1]["allowed"] == want).all() and (one[1]["allowed"].sum(axis=1) == one[0]["n_allowed"]).all()
    assert one[0]["reach"].tolist() == [2, 2, 2, 2, 1, 2] and one[0]["offset"][0] == 2.5 * DT


def test_detrending_events_and_the_statement(ctx):
    """detrend=25 equals the call on rows detrended beforehand; without pairs the events of single_transits on the same rows are
    paired; the survey call equals the statement on the rows a search gets."""
    t, flux = _survey_case()
    kw = dict(widths=[4, 8], period_min=0.4, max_aliases=24, context=ctx)
    flat = survey.detrend_batch(flux, 25, context=ctx)
    inside = survey.event_periods(t, flux, detrend=25, **kw)
    before = survey.event_periods(t, flat, **kw)
    assert inside[0].tobytes() == before[0].tobytes() and inside[1].tobytes() == before[1].tobytes() and len(inside[0]) >= 4
    events, n_events = survey.single_transits(t, flat, widths=[4, 8], context=ctx)
    found = survey.event_pairs(events, n_events)
    assert len(found[0]) == len(inside[0]) and inside[0]["index_a"].tolist() == found[1].tolist()
    chained = survey.event_periods(t, flat, events=events, n_events=n_events, **kw)
    assert chained[0].tobytes() == inside[0].tobytes() and chained[1].tobytes() == inside[1].tobytes()
    inp, y_rows, dy_rows = survey._batch_inputs(t, flat, None, dict(oversampling_factor=1))
    shapes = spec.shapes_of([4, 8], **inp["shape"])
    want = spec.expected(inp["t"], y_rows, dy_rows, *found, inside[0]["reach"], inside[0]["offset"], shapes, spans_of([4, 8]), 0.4,
                         24)
    for f in spec.PAIR_FIELDS:
        expect_equal(inside[0][f], want[0][f], f)
    for f in spec.ALIAS_FIELDS:
        expect_equal(inside[1][f], want[1][f], f)
    best = inside[0][(inside[0]["status"] == 0) & (inside[0]["n_allowed"] > 0)]     # (a pair may have every alias vetoed)
    assert len(best) and numpy.all(best["best_n_covered"] >= 2)


def test_poisoned_lds_and_reused_scratch(ctx):
    """The same bytes before and after poison_lds, and for a small call behind a large one: neither path reads LDS or scratch it
    has not written."""
    shapes, span_max = shapes_of(WIDTHS), spans_of(WIDTHS)

    def small():
        n = 300
        y = curve_with(n, [(40, 8), (240, 8)], seed=1)
        return ctx.event_periods(series(n), y, numpy.full(n, 1e-3), [0, 0], [40, 41], [240, 240], [2, 3], [2, 2], [2.5 * DT] * 2,
                                 WIDTHS, shapes, span_max, 10 * DT, 16)

    def large():
        n = _lib.ALIAS_LDS_POINTS + 300
        y = numpy.stack([curve_with(n, [(400, 37), (5000, 37)], seed=s) for s in range(3)])
        return ctx.event_periods(series(n), y, numpy.full((3, n), 1e-3), [0, 1, 2, 2], [400] * 4, [5000] * 4, [3, 3, 3, 4],
                                 [4] * 4, [4.5 * DT] * 4, WIDTHS, shapes, span_max, 300 * DT, 64)

    first_small, first_large = small(), large()
    behind = small()
    ctx.poison_lds()
    after_small = small()
    ctx.poison_lds()
    after_large = large()
    for got, want in ((behind, first_small), (after_small, first_small), (after_large, first_large)):
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert first_small[0]["status"].tolist() == [0, 0] and first_large[0]["status"].tolist() == [0] * 4


def test_c_entry_arguments(ctx):
    """n_pairs == 0 is a no-op; every TLS_E_ARG case returns before any device work with the outputs untouched."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = series(n)
    good = dict(t=t, y=numpy.ones((2, n)), dy=numpy.full((2, n), 1e-3), n_curves=2, curve=[1], index_a=[20], index_b=[200],
                row=[1], reach=[2], offset=[0.04], n_pairs=1, shape_values=numpy.ones(8), shape_offset=[0, 3], width=[3, 5],
                span_max=[0.1, 0.2], n_rows=2, period_min=0.5, max_aliases=4, min_ses=3.0, veto_sigma=3.0)
    pairs = numpy.full(1, -7.0, dtype=_lib.EVENT_PAIR_DTYPE)
    aliases = numpy.full((1, 4), -7.0, dtype=_lib.EVENT_ALIAS_DTYPE)

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "y", "dy", "offset", "shape_values", "span_max")}
        i8 = {k: _lib._i8(a[k]) for k in ("curve", "index_a", "index_b", "row", "reach", "shape_offset", "width")}
        return lib.tls_event_periods(ctx._h, dp(f8["t"]), dp(f8["y"]), dp(f8["dy"]), len(f8["t"]), a["n_curves"], ip(i8["curve"]),
                                     ip(i8["index_a"]), ip(i8["index_b"]), ip(i8["row"]), ip(i8["reach"]), dp(f8["offset"]),
                                     a["n_pairs"], dp(f8["shape_values"]), ip(i8["shape_offset"]), ip(i8["width"]),
                                     dp(f8["span_max"]), a["n_rows"], a["period_min"], a["max_aliases"], a["min_ses"],
                                     a["veto_sigma"], pairs.ctypes.data_as(ctypes.c_void_p), aliases.ctypes.data_as(ctypes.c_void_p))

    def untouched():
        return all((pairs[k] == -7.0).all() for k in pairs.dtype.names) and all((aliases[k] == -7.0).all() for k in aliases.dtype.names)

    assert call(n_pairs=0) == 0 and untouched()
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - DT
    bad_t = t.copy()
    bad_t[5] = nan
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(row=[2]), dict(row=[-1]), dict(reach=[0]), dict(reach=[4097]),
               dict(index_a=[-1]), dict(index_b=[257]), dict(index_a=[200]), dict(index_a=[201]), dict(offset=[-1e-9]),
               dict(offset=[inf]), dict(offset=[nan]), dict(period_min=0.0), dict(period_min=-1.0), dict(period_min=inf),
               dict(period_min=nan), dict(period_min=(t[-1] - t[0]) / 65534.5), dict(max_aliases=0), dict(max_aliases=4097),
               dict(min_ses=nan), dict(veto_sigma=nan), dict(width=[2, 5]), dict(width=[3, 4097]), dict(width=[5, 3]),
               dict(shape_offset=[0, -1]), dict(n_rows=0), dict(span_max=[0.1, inf]), dict(span_max=[-0.1, 0.2]), dict(t=late),
               dict(t=bad_t), dict(n_pairs=-1), dict(n_curves=-1), dict(t=numpy.zeros((1 << 20) + 1))):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"event periods" in lib.tls_last_error(ctx._h), kw
    assert call(veto_sigma=inf, period_min=(t[-1] - t[0]) / 65533.5) == 0 and not untouched()
    assert call() == 0 and pairs["status"][0] == 2      # (constant flux: no dip)
    empty = ctx.event_periods(t, numpy.ones((2, n)), numpy.ones((2, n)), [], [], [], [], [], [], [3], [numpy.ones(3)], [0.1], 0.5)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 256)
