"""The folded views on the device (survey.folded_views / tls_folded_views; power_batch(peaks=K, peak_fits=True, views=True))
against tests/folded_views_spec.py bit for bit (NaN equal to NaN), every field of the record and every entry of every array:
at the sizes of the series (1 to 257, and around _lib.VIEWS_LDS_POINTS, the points the LDS holds), at the populations of a bin
(0 to 4, around _lib.VIEWS_LANE_MEMBERS -- the largest bin a lane selects alone --, around the 64 lanes of the wave that
selects a larger one, and 3000 members in one bin), at the edges of the bins on dyadic values, for every parity and secondary
phase, over the candidates of a call (none, two slabs, several a curve, bad ones among good ones, argument errors), after
poisoned LDS and scratch, and in the pipeline with every other result untouched.

Time stamps are multiples of 1/64 d (1/8 d in the edge cases), so every time difference is exact."""
import ctypes
import warnings

import numpy
import pytest

import folded_views_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

DT = 1 / 64.0
SMALL = dict(n_global=37, n_local=21)


@pytest.fixture
def ctx(gpu):
    return gpu


def same(a, b):
    """Bit for bit: the same type, shape and bytes."""
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(got, want, err_msg=str(what))       # (NaN equal to NaN)
    assert same(got, want), what


def as_views(out):
    return out[0], survey._views_dict(*out[1:], lead=(len(out[0]),))


def check(ctx, t, y, period, T0, duration, curve=None, phi=None, label="", **table):
    """ctx.folded_views of the candidates equals the statement in every field and entry; (records, views) of the device."""
    y = numpy.atleast_2d(numpy.asarray(y, dtype=float))
    if curve is None and len(period) != len(y):
        curve = numpy.zeros(len(period), dtype=int)
    records, views = as_views(ctx.folded_views(t, y, period, T0, duration, curve=curve, secondary_phase=phi, **table))
    want_records, want = spec.folded_views(t, y, period, T0, duration, curve=curve, secondary_phase=phi, **table)
    assert records.dtype.names == spec.FIELDS and records.shape == (len(period),)
    for i, f in enumerate(spec.FIELDS):
        expect_equal(records[f], want_records[:, i], (label, f))
    assert set(views) == set(want)
    for k in want:
        expect_equal(views[k], want[k], (label, k))
    return records, views


def noisy(n, seed, levels=None):
    """n values about 1: noise, or -- levels -- draws from that many values, so that equal values abound."""
    rng = numpy.random.RandomState(seed)
    return 1.0 + 1e-3 * rng.normal(size=n) if levels is None else 1.0 + 1e-3 * rng.randint(0, levels, n)


# ---- sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, _lib.VIEWS_LDS_POINTS - 1, _lib.VIEWS_LDS_POINTS, _lib.VIEWS_LDS_POINTS + 1])
def test_sizes(ctx, n):
    """Around the wave, the workgroup and the points the LDS holds (beyond them the series is ordered in device scratch): the
    default tables -- n_global = 2001 bins, mostly empty -- and small ones, a planet's and a short period's candidate."""
    t = 1.0 + numpy.arange(n) * DT
    y = numpy.array([noisy(n, n), noisy(n, n + 1, levels=3)])
    span = max(t[-1] - t[0], 1.0)
    period, T0, duration = [span / 3.3, 0.37, span / 3.3], [t[0] + 0.1, t[0] + 0.2, t[n // 2]], [span / 40, 0.05, span / 40]
    records, views = check(ctx, t, y, period, T0, duration, curve=[0, 1, 1], phi=[0.5, 0.31, numpy.nan], label=n)
    assert records["status"].tolist() == [0, 0, 0] and records["secondary_status"].tolist() == [0, 0, 1]
    check(ctx, t, y, period, T0, duration, curve=[1, 0, 0], phi=[0.5, 0.31, 0.77], label=(n, "small"), **SMALL)


def test_bin_populations(ctx):
    """One epoch on a regular series, bins of c cadences: every population from 0 to 4, around VIEWS_LANE_MEMBERS (a lane
    selects a bin up to it alone, a wave a larger one), around the 64 and the 128 members a wave takes in one and two strides
    -- on noise, on three levels (equal values across the middle) and on a constant row (a bin of all-equal values)."""
    n = 3000
    t = 1.0 + numpy.arange(n) * DT
    y = numpy.array([noisy(n, 5), noisy(n, 6, levels=3), numpy.ones(n)])
    lane = _lib.VIEWS_LANE_MEMBERS
    seen = set()
    for c in (1, 2, 3, 4, lane - 1, lane, lane + 1, 63, 64, 65, 127, 128, 129, 400):
        # d = 1, k = 4: the view spans 512 cadences from T0 - 4, the first tenth of them in front of the series (empty bins)
        records, views = check(ctx, t, y, [1000.0] * 3, [t[0] + 3.6 + DT / 2] * 3, [1.0] * 3, n_global=16, n_local=16,
                               local_width=c * DT, label=c)
        seen |= set(views["local_count"].ravel().tolist())
        full = views["local_count"][2] > 0
        assert (views["local"][2][full] == 1.0).all() and numpy.isnan(views["local"][2][~full]).all()
    wanted = {0, 1, 2, 3, 4, lane - 1, lane, lane + 1, 63, 64, 65, 127, 128, 129, 400}
    assert wanted <= seen, sorted(wanted - seen)


def test_one_bin_holds_every_point(ctx):
    """B = 2 and w = the whole range, a range wider than the period: both bins hold all of n = 3000 points -- the large
    population, by the wave that takes every bin above VIEWS_LANE_MEMBERS, in 47 strides."""
    n = 3000
    t = numpy.arange(n) * DT
    y = numpy.array([noisy(n, 7), noisy(n, 8, levels=2)])
    records, views = check(ctx, t, y, [2.0, 2.0], [0.0, 0.25], [0.5, 0.5], phi=[0.5, 0.01], n_global=2, n_local=2,
                           local_width=8.0)
    assert (views["local_count"] == n).all() and (views["secondary_count"] == n).all()
    assert (views["local_even_count"] + views["local_odd_count"] == n).all() and (records["n_local"] == n).all()
    expect_equal(views["local"][:, 0], numpy.array([spec.median_of(y[0]), spec.median_of(y[1])]), "median of everything")


@pytest.mark.parametrize("width, kind", [(0.16, "overlapping"), (0.5, "disjoint"), (0.25, "gapped")])
def test_tables(ctx, width, kind):
    """k = 4, d = 1, 16 bins: w = 0.5 is s exactly (disjoint), 0.25 leaves gaps (points in no bin), and 201 bins of 0.16
    overlap four deep."""
    n = 2000
    t = 1.0 + numpy.arange(n) * DT
    y = noisy(n, 9)
    bins = 201 if kind == "overlapping" else 16
    records, views = check(ctx, t, y, [9.0], [3.0 + DT / 4], [1.0], phi=[0.4], n_global=64, n_local=bins, local_width=width,
                           label=kind)
    inside = int((numpy.fabs(spec.fold(t, 9.0, 3.0 + DT / 4, 0.0)[0]) < 4.0).sum())
    total = int(views["local_count"].sum())
    if kind == "overlapping":
        assert total > 3 * inside and records["n_local"][0] == inside
    elif kind == "disjoint":
        assert total == inside == records["n_local"][0]
    else:
        assert total == records["n_local"][0] < 0.6 * inside


# ---- edges: P = 2, T0 = 0, t in multiples of 1/8, d = 0.5 -- every edge is a representable number ---------------------------------
@pytest.mark.parametrize("k", [1.0, 2.0, 4.0])
def test_edges_on_dyadic_values(ctx, k):
    """tau runs over the multiples of 1/8 in [-1, 1): tau == lo_b (a member) and tau == lo_b + w (not one) in every bin,
    tau == x_min (k = 1, 2: in bin 0), tau == x_max (k = 1: in no bin), phase -0.5 (tau = -1, never +1); k = 4 is a local range
    wider than the period.  The global view's 16 bins are [lo, lo + 1/8): one phase each."""
    t = numpy.arange(-80, 240) / 8.0
    y = noisy(len(t), 10)
    for bins, width in ((17, 0.5), (5, 2.0 * k), (8, 0.25 * k)):
        records, views = check(ctx, t, y, [2.0], [0.0], [0.5], phi=[0.5], n_global=16, n_local=bins, local_durations=k,
                               local_width=width, label=(k, bins))
        assert (views["global_count"] == len(t) // 16).all() and records["n_global"][0] == len(t)
    tau = spec.fold(t, 2.0, 0.0, 0.0)[0]
    assert tau.min() == -1.0 and tau.max() == 0.875
    lo, hi = spec.edges(-0.5 * k, 0.5 * k, 0.125 * k, 8)                # (the last table: w == s == k / 8, disjoint bins)
    assert (k > 2 or numpy.isin(lo, tau).all()) and hi[-1] == 0.5 * k and (hi[:-1] == lo[1:]).all()   # (an edge is a point's tau)
    expect_equal(views["local_count"][0], numpy.array([((tau >= a) & (tau < b)).sum() for a, b in zip(lo, hi)], dtype=numpy.int32),
                 "counts")
    if k == 1.0:
        assert records["n_local"][0] == int(((tau >= -0.5) & (tau < 0.5)).sum()) < int((numpy.fabs(tau) <= 0.5).sum())


# ---- parity -----------------------------------------------------------------------------------------------------------------
def test_parities(ctx):
    """Only even epochs in the series, only odd ones, T0 in the middle of the series (negative e) and behind its last point."""
    t = 1.0 + numpy.arange(1600) * DT                                         # 25 d
    y = noisy(len(t), 11)
    P, d = 2.5, 0.125
    e = numpy.floor((t - 1.25) / P + 0.5)
    for label, keep, T0 in (("even only", e % 2 == 0, 1.25), ("odd only", e % 2 == 1, 1.25), ("middle", e > -9, 1.25 + 5 * P),
                            ("behind", e > -9, 1.25 + 12 * P)):
        records, views = check(ctx, t[keep], y[keep], [P], [T0], [d], phi=[0.5], label=label, **SMALL)
        if label == "even only":
            assert records["n_local_odd"][0] == 0 and records["n_local_even"][0] == records["n_local"][0] > 0
            assert same(views["local_even"], views["local"]) and numpy.isnan(views["local_odd"]).all()
        elif label == "odd only":
            assert records["n_local_even"][0] == 0 and records["n_local_odd"][0] == records["n_local"][0] > 0
            assert same(views["local_odd"], views["local"])
        else:
            assert records["n_local_even"][0] > 0 and records["n_local_odd"][0] > 0
            assert records["n_local_even"][0] + records["n_local_odd"][0] == records["n_local"][0]


# ---- secondary --------------------------------------------------------------------------------------------------------------
def test_secondary_phases(ctx):
    """phi_s = 0.5, the wrap at 0.01 and 0.99, 0 (the local view again), NaN and inf among them, and no phases at all."""
    t = 1.0 + numpy.arange(1600) * DT
    y = numpy.array([noisy(len(t), 12), noisy(len(t), 13)])
    phi = [0.5, 0.01, 0.99, numpy.nan, 0.0, numpy.inf, 0.25]
    m = len(phi)
    records, views = check(ctx, t, y, [2.5] * m, [1.3] * m, [0.125] * m, curve=[0, 1, 0, 1, 0, 1, 0], phi=phi, **SMALL)
    assert records["secondary_status"].tolist() == [0, 0, 0, 1, 0, 1, 0] and (records["status"] == 0).all()
    assert same(views["secondary"][4], views["local"][4]) and numpy.isnan(views["secondary"][[3, 5]]).all()
    assert (views["secondary_count"][[3, 5]] == 0).all() and (records["n_secondary"][[3, 5]] == 0).all()
    records, views = check(ctx, t, y, [2.5, 2.5], [1.3, 1.4], [0.125, 0.125], phi=None, **SMALL)
    assert records["secondary_status"].tolist() == [1, 1] and numpy.isnan(views["secondary"]).all()
    assert not numpy.isnan(views["local"]).all()


# ---- candidates -------------------------------------------------------------------------------------------------------------
def test_candidates_curves_and_slabs(ctx):
    """More candidates than one launch slab (VIEWS_SLAB) on n = 64: several a curve, the curves in shuffled order, bad
    candidates (NaN, inf, P <= 0, d <= 0) among good ones; and no candidate at all."""
    n, curves, m = 64, 40, _lib.VIEWS_SLAB + 37
    rng = numpy.random.RandomState(14)
    t = 1.0 + numpy.arange(n) * DT
    y = 1.0 + 1e-3 * rng.normal(size=(curves, n))
    curve = rng.randint(0, curves, m)
    period, T0, duration = rng.uniform(0.1, 1.5, m), rng.uniform(0.0, 3.0, m), rng.uniform(0.01, 0.2, m)
    phi = rng.uniform(0.0, 1.0, m)
    bad = {5: (numpy.nan, 1.0, 0.1), 6: (1.0, numpy.inf, 0.1), 7: (1.0, 1.0, numpy.nan), 300: (0.0, 1.0, 0.1),
           301: (-1.0, 1.0, 0.1), 1023: (1.0, 1.0, 0.0), 1024: (1.0, 1.0, -0.1), 1025: (numpy.inf, 1.0, 0.1), m - 1: (1.0, 1.0, numpy.inf)}
    for f, v in bad.items():
        period[f], T0[f], duration[f] = v
    phi[[8, 1030]] = numpy.nan
    records, views = check(ctx, t, y, period, T0, duration, curve=curve, phi=phi, n_global=12, n_local=7)
    assert sorted(numpy.nonzero(records["status"])[0].tolist()) == sorted(bad)
    assert sorted(numpy.nonzero(records["secondary_status"])[0].tolist()) == sorted(list(bad) + [8, 1030])
    for f in bad:
        assert numpy.isnan(views["global"][f]).all() and (views["local_count"][f] == 0).all() and records["n_global"][f] == 0
    for m in (_lib.VIEWS_SLAB - 1, _lib.VIEWS_SLAB, _lib.VIEWS_SLAB + 1):     # (one slab to its last place; a second of one)
        check(ctx, t, y, period[-m:], T0[-m:], duration[-m:], curve=curve[-m:], phi=phi[-m:], n_global=12, n_local=7, label=m)
    none = ctx.folded_views(t, y, [], [], [], curve=[], **SMALL)
    assert none[0].shape == (0,) and none[1].shape == (0, 37) and none[3].shape == (0, 4, 21)


def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; every TLS_E_ARG case returns before any device work with the outputs untouched; curve NULL takes
    candidate i on curve i."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = 1.0 + numpy.arange(n) * DT
    y = numpy.array([noisy(n, 15), noisy(n, 16)])
    good = dict(t=t, n_curves=2, period=[1.0, 1.5], T0=[1.5, 1.25], duration=[0.1, 0.2], phi=[0.5, 0.25], curve=[1, 0], n_fits=2,
                n_global=16, n_local=8, k=4.0, width=0.16)
    outs = {}

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "period", "T0", "duration")}
        phi = None if a["phi"] is None else _lib._f8(a["phi"])
        curve = None if a["curve"] is None else _lib._i8(a["curve"])
        outs.update(rec=numpy.full(2, -7.0, dtype=_lib.VIEWS_DTYPE), g=numpy.full((2, 16), -7.0),
                    gc=numpy.full((2, 16), -7, dtype=numpy.int32), l=numpy.full((2, 4, 8), -7.0),
                    lc=numpy.full((2, 4, 8), -7, dtype=numpy.int32))
        vp = ctypes.c_void_p
        return lib.tls_folded_views(ctx._h, dp(f8["t"]), dp(y), len(f8["t"]), a["n_curves"], dp(f8["period"]), dp(f8["T0"]),
                                    dp(f8["duration"]), None if phi is None else dp(phi), None if curve is None else ip(curve),
                                    a["n_fits"], a["n_global"], a["n_local"], a["k"], a["width"], outs["rec"].ctypes.data_as(vp),
                                    dp(outs["g"]), outs["gc"].ctypes.data_as(vp), dp(outs["l"]), outs["lc"].ctypes.data_as(vp))

    def untouched():
        return all((outs["rec"][k] == -7.0).all() for k in spec.FIELDS) and all((outs[k] == -7).all() for k in ("g", "gc", "l", "lc"))

    assert call(n_fits=0) == 0 and untouched()
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - DT
    bad_t = t.copy()
    bad_t[5] = nan
    for kw in (dict(curve=[2, 0]), dict(curve=[0, -1]), dict(curve=None, n_curves=1), dict(n_global=1), dict(n_local=1),
               dict(n_global=0), dict(n_local=-3), dict(n_global=_lib.VIEWS_MAX_BINS + 1), dict(k=0.0), dict(k=-1.0), dict(k=nan),
               dict(k=inf), dict(width=0.0), dict(width=-0.1), dict(width=nan), dict(width=8.0 + 2.0 ** -40), dict(t=late),
               dict(t=bad_t), dict(n_fits=-1), dict(n_curves=-1)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"folded views" in lib.tls_last_error(ctx._h), kw
    assert call() == 0 and not untouched()
    want_records, want = spec.folded_views(t, y, good["period"], good["T0"], good["duration"], curve=[1, 0],
                                           secondary_phase=good["phi"], n_global=16, n_local=8)
    expect_equal(outs["g"], want["global"], "global")
    expect_equal(outs["lc"][:, 2], want["local_odd_count"], "local_odd_count")
    assert call(curve=None, width=8.0) == 0                                 # (one bin as wide as the view)
    want_records, want = spec.folded_views(t, y, good["period"], good["T0"], good["duration"], curve=None,
                                           secondary_phase=good["phi"], n_global=16, n_local=8, local_width=8.0)
    expect_equal(outs["l"][:, 3], want["secondary"], "secondary, curve NULL")
    expect_equal(outs["rec"]["n_local_even"], want_records[:, 4], "n_local_even")


# ---- memory -----------------------------------------------------------------------------------------------------------------
def test_poisoned_lds_and_reused_scratch(ctx):
    """The same call before and after tls_debug_poison_lds (every CU's LDS and the call's device buffers smeared) agrees byte
    for byte, in the LDS and beyond it; a call with small tables behind one with large tables reuses the buffers and agrees."""
    for n in (1000, _lib.VIEWS_LDS_POINTS + 300):
        t = 1.0 + numpy.arange(n) * DT
        y = numpy.array([noisy(n, 17), noisy(n, 18, levels=4)])
        args = (t, y, [2.5, 0.7, numpy.nan], [1.3, 1.1, 1.0], [0.125, 0.06, 0.1])
        kw = dict(curve=[0, 1, 1], secondary_phase=[0.5, numpy.nan, 0.5])
        small = ctx.folded_views(*args, n_global=9, n_local=5, **kw)
        large = ctx.folded_views(*args, **kw)
        ctx.poison_lds(0xFFFFFFFF)
        again = ctx.folded_views(*args, n_global=9, n_local=5, **kw)
        ctx.poison_lds(0x7FF00000)
        large_again = ctx.folded_views(*args, **kw)
        for a, b in zip(small + large, again + large_again):
            assert same(a, b), n
        want_records, want = spec.folded_views(*args, curve=[0, 1, 1], secondary_phase=kw["secondary_phase"], n_global=9, n_local=5)
        expect_equal(again[1], want["global"], n)
        expect_equal(again[3][:, 0], want["local"], n)


# ---- survey.folded_views and the pipeline -----------------------------------------------------------------------------------
T = 3.0 + numpy.arange(500) / 16.0                    # 31 d at 90 min
KW = dict(period_min=1.5, period_max=6, oversampling_factor=1)
_RUNS = {}


def flux_rows():
    """4 rows of 500 points: two with a planet, one with a binary that has a secondary, one quiet."""
    if "flux" not in _RUNS:
        rows = []
        for s, (per, rp, sec) in enumerate(((2.9, 0.1, 0.0), (4.3, 0.12, 0.0), (3.7, 0.15, 6e-3), (0.0, 0.0, 0.0))):
            rng = numpy.random.RandomState(2000 + s)
            f = 1.0 + rng.normal(0, 3e-4, len(T)) + 1e-3 * numpy.sin(T / 2.3 + s)
            if per:
                f += transit_model.light_curve(T, T[0] + 0.8, per, rp, 9.0, 89.9, 0, 90, [0.4, 0.3], "quadratic") - 1
                f -= sec * (numpy.fabs((T - T[0] - 0.8) / per - 0.5 - numpy.round((T - T[0] - 0.8) / per - 0.5)) * per < 0.1)
            rows.append(f)
        _RUNS["flux"] = numpy.array(rows)
    return _RUNS["flux"]


def run(ctx, **more):
    """power_batch(peaks=2, peak_fits=True, ...) of the four rows, each variant once a session."""
    key = tuple(sorted((k, repr(v)) for k, v in more.items()))
    if "floor" not in _RUNS:
        # a power between those of the eight peaks of a plain run: the weaker peaks are not taken, and their places in the
        # table -- status 1, no such peak -- are candidates without an ephemeris
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            power = numpy.sort(survey.power_batch(T, flux_rows(), peaks=2, context=ctx, **KW)[2]["peaks"]["power"].ravel())
        power = power[~numpy.isnan(power)]
        assert len(power) >= 5 and power[1] < power[2]
        _RUNS["floor"] = float(0.5 * (power[1] + power[2]))
    if key not in _RUNS:
        kw = dict(more, peak_min_power=_RUNS["floor"])
        if "devices" not in kw:
            kw["context"] = ctx
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _RUNS[key] = survey.power_batch(T, flux_rows(), peaks=2, peak_fits=True, **kw, **KW)
    return _RUNS[key]


def expect_rest_equal(got, without):
    """Everything but the views is byte-equal with and without the keyword."""
    assert got[0].dtype == without[0].dtype and got[0].tobytes() == without[0].tobytes()
    expect_equal(got[1], without[1], "periods")
    pk, base = got[2], without[2]
    assert set(pk) == set(base) | {"views"}
    added = ("views_status",) + tuple("views_" + k for k in survey.folded_view_fields()[2:])
    assert pk["peaks"].dtype.names == base["peaks"].dtype.names + added
    for k in base["peaks"].dtype.names:
        assert pk["peaks"][k].tobytes() == base["peaks"][k].tobytes(), k
    for k in base:
        if k != "peaks":
            assert same(pk[k], base[k]), k


def expect_views_of(ctx, got, rows, scan, **table):
    """The views of the result equal survey.folded_views, and the statement, on the returned records and the rows given."""
    peaks, views = got[2]["peaks"], got[2]["views"]
    fitted = (peaks["status"] == 0).reshape(-1)
    assert fitted.any()
    period, T0, duration = (numpy.where(fitted, peaks[k].reshape(-1), numpy.nan) for k in ("period", "T0", "duration_days"))
    phi = numpy.where(fitted, peaks["secondary_phase"].reshape(-1), numpy.nan) if scan else None
    curve = numpy.repeat(numpy.arange(4), 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y_rows = survey._batch_inputs(T, rows, None, dict(KW))[1]
    records, alone = survey.folded_views(T, y_rows, period, T0, duration, curve=curve, secondary_phase=phi, context=ctx, **table)
    want_records, want = spec.folded_views(T, y_rows, period, T0, duration, curve=curve, secondary_phase=phi, **table)
    assert set(views) == set(alone) == set(want)
    for k in want:
        assert views[k].shape == (4, 2) + want[k].shape[1:], k
        expect_equal(views[k].reshape(want[k].shape), alone[k], k)
        expect_equal(alone[k], want[k], k)
    for i, f in enumerate(spec.FIELDS):
        expect_equal(records[f], want_records[:, i], f)
        if f != "secondary_status":
            expect_equal(peaks["views_status" if f == "status" else "views_" + f].reshape(-1), records[f], f)
    assert (records["status"] == numpy.where(fitted, 0, 1)).all()
    assert numpy.isnan(views["secondary"]).all() != bool(scan)
    return views


def test_pipeline(ctx):
    """views=True with and without phase_scan: the views are those of survey.folded_views on the returned records and the rows
    searched, every other array is byte-equal to the call without the keyword, and the planets show in their local views."""
    flux = flux_rows()
    for scan in (False, True):
        got = run(ctx, views=True, phase_scan=scan)
        expect_rest_equal(got, run(ctx, phase_scan=scan))
        views = expect_views_of(ctx, got, flux, scan)
        assert 3 <= (got[2]["peaks"]["views_status"] == 0).sum() < 8       # (the peaks under the floor: no such candidate)
        assert views["global"].shape == (4, 2, 2001) and views["local_odd_count"].dtype == numpy.int32
        deep = survey.normalize_views(views)["local"][:3, 0]
        assert (numpy.argmin(deep, axis=1) > 80).all() and (numpy.argmin(deep, axis=1) < 120).all()   # (the dip is in the middle)


def test_pipeline_tables_devices_and_detrend(ctx):
    """Other tables; devices=[0, 0] equals one device; detrend=25 views the filtered rows."""
    table = dict(views_global_bins=301, views_local_bins=31, views_local_durations=3.0, views_local_width=0.5)
    plain = dict(n_global=301, n_local=31, local_durations=3.0, local_width=0.5)
    one = run(ctx, views=True, phase_scan=True, **table)
    expect_views_of(ctx, one, flux_rows(), True, **plain)
    two = run(ctx, views=True, phase_scan=True, devices=[0, 0], **table)
    assert two[0].tobytes() == one[0].tobytes() and two[2]["peaks"].tobytes() == one[2]["peaks"].tobytes()
    for k in one[2]["views"]:
        assert same(two[2]["views"][k], one[2]["views"][k]), k
    flat = run(ctx, views=True, phase_scan=True, detrend=25)
    expect_rest_equal(flat, run(ctx, phase_scan=True, detrend=25))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        searched = survey.detrend_batch(flux_rows(), 25, context=ctx)
    expect_views_of(ctx, flat, searched, True)
    assert not same(flat[2]["views"]["global"], run(ctx, views=True, phase_scan=True)[2]["views"]["global"])
