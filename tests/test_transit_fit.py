"""The limb-darkened transit fit on the device (survey.transit_fit / tls_transit_fit; power_batch(peaks=K, peak_fits=True,
transit_fit=True)) against tests/transit_fit_spec.py bit for bit, every field of the record: over the units (27, fewer than the
256 threads; 315, more than them and no multiple of the four a thread carries), the profile's resolution (M = 16 and 1024),
the sub-exposures (1, 3 and 16), with and without per-point dy, curve=None and a shuffled curve, bad candidates (status 1), a
curve no unit fits (status 2), second rows at both edges of the table, an impact table that holds 0 exactly and equal
neighbours; with more members than the LDS holds, exactly as many and one more; over two slabs; behind poisoned LDS and
smeared, reused scratch; with every argument error; and in the pipeline with every other result untouched."""
import ctypes
import warnings

import numpy
import pytest

import transit_fit_spec as spec
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

DT = 1 / 48.0
TABLES = {
    27: ([0.0, 0.5, 0.9], [0.8, 1.0, 1.25], [-0.1, 0.0, 0.1]),
    315: ([0.0, 0.0, 0.3, 0.6, 0.9], numpy.geomspace(0.7, 1.4, 7), numpy.linspace(-0.1, 0.1, 9)),
}
K_ROWS = numpy.geomspace(0.04, 0.1, 7)
RP = (0.03, 0.05, 0.07, 0.09, 0.12)                    # (the first and the last lie outside K_ROWS: second rows at both edges)
_PROFILES = {}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def profile(M, k_rows=K_ROWS):
    key = (M, tuple(k_rows))
    if key not in _PROFILES:
        _PROFILES[key] = survey.transit_profile(k_rows, M, u=[0.4, 0.4], limb_dark="quadratic")
    return _PROFILES[key]


def series(n, gap_at=None, gap=0, dt=DT):
    t = 1.0 + numpy.arange(n + gap) * dt
    return t if gap_at is None else numpy.concatenate([t[:gap_at], t[gap_at + gap:]])


def expect_equal(got, want, what):
    numpy.testing.assert_array_equal(numpy.asarray(got, dtype=float), numpy.asarray(want, dtype=float), err_msg=str(what))


def check(ctx, t, y, dy, period, T0, duration, rows, table, tables, sub, curve=None, label="", **kw):
    """ctx.transit_fit of the candidates equals the statement in every field; what the device returned."""
    y = numpy.atleast_2d(y)
    dy = numpy.broadcast_to(numpy.asarray(dy, dtype=float), y.shape) if numpy.ndim(dy) < 2 else dy
    got = ctx.transit_fit(t, y, dy, period, T0, duration, rows, table[0], table[1], *tables, sub, curve=curve, **kw)
    which = numpy.arange(len(y)) if curve is None else curve
    want = spec.transit_fit_batch(t, y, dy, period, T0, duration, which, rows, table[0], table[1], *tables, sub, **kw)
    assert got.dtype.names == spec.FIELDS and got.shape == (len(period),)
    for i, f in enumerate(spec.FIELDS):
        expect_equal(got[f], want[:, i], (label, f))
    return got


# ---- the base shape: 700 points with a gap, 40 candidates on 6 curves -------------------------------------------------------
def base():
    """t [700], y [6, 700] (five planets of RP and a constant curve), per-point dy, and 40 candidates."""
    t = series(700, gap_at=300, gap=60)
    rng = numpy.random.RandomState(5)
    P = numpy.array([2.1, 2.6, 3.1, 3.7, 2.9])
    T0 = t[0] + numpy.array([0.7, 1.1, 0.4, 1.9, 1.3])
    a_rs = numpy.array([8.0, 9.0, 10.0, 12.0, 9.5])
    y = numpy.ones((6, len(t)))
    T14 = numpy.zeros(5)
    for i in range(5):
        y[i] = transit_model.light_curve(t, T0[i], P[i], RP[i], a_rs[i], 89.0, 0, 90, [0.4, 0.4], "quadratic") \
            + rng.normal(0, 1e-4, len(t))
        T14[i] = P[i] / numpy.pi * numpy.arcsin(numpy.sqrt((1 + RP[i]) ** 2 - (a_rs[i] * numpy.cos(numpy.radians(89.0))) ** 2) / a_rs[i])
    dy = rng.uniform(0.8e-4, 1.3e-4, y.shape)
    curve = numpy.array([f % 6 for f in range(40)])
    planet = numpy.minimum(curve, 4)
    period = P[planet].copy()
    T0s = T0[planet] + rng.randint(-2, 3, 40) * 0.004
    duration = T14[planet] * rng.uniform(0.9, 1.1, 40)
    rows = rng.randint(0, len(K_ROWS), 40)
    rows[:6] = [1, 2, 3, 5, 6, 0]                      # (near the truth for the first candidate of a curve: some second rows stay)
    for bad, values in ((7, (numpy.nan, T0s[7], duration[7])), (14, (period[14], numpy.inf, duration[14])),
                        (21, (0.0, T0s[21], duration[21])), (28, (-period[28], T0s[28], duration[28])),
                        (33, (period[33], T0s[33], -0.1)), (39, (0.3, T0s[39], 0.2))):
        period[bad], T0s[bad], duration[bad] = values
    return t, y, dy, period, T0s, duration, rows, curve


CASES = [(27, 16, 1, False, False), (27, 1024, 3, True, True), (315, 16, 16, True, False), (315, 1024, 1, False, True),
         (315, 1024, 3, True, True), (27, 1024, 16, False, True), (27, 4096, 1, True, False)]   # (M = 4096: 80 KB of LDS)


@pytest.mark.parametrize("units, M, S, with_dy, shuffled", CASES)
def test_the_base_shape(ctx, units, M, S, with_dy, shuffled):
    t, y, dy, period, T0, duration, rows, curve = base()
    tables = TABLES[units]
    assert len(tables[0]) * len(tables[1]) * len(tables[2]) == units
    if shuffled:
        order = numpy.random.RandomState(units + M + S).permutation(40)
        period, T0, duration, rows, curve = (v[order] for v in (period, T0, duration, rows, curve))
    else:                                              # curve=None: one candidate a curve, in order
        period, T0, duration, rows, curve = period[:6], T0[:6], duration[:6], rows[:6], None
    sub = spec.sub_offsets(DT, S)
    got = check(ctx, t, y, dy if with_dy else 1e-4, period, T0, duration, rows, profile(M), tables, sub, curve=curve,
                label=(units, M, S))
    which = numpy.arange(6) if curve is None else curve
    assert (got["status"][which == 5] != 0).all()       # (the constant curve: no unit is valid, or a bad candidate)
    assert (got["status"][which == 5] == 2).any()
    fitted = got["status"] == 0
    assert fitted.sum() >= (5 if curve is None else 28)
    assert all((got[k + "_lo"][fitted] <= got[k][fitted]).all() and (got[k][fitted] <= got[k + "_hi"][fitted]).all()
               for k in ("k", "b", "duration", "shift"))
    if shuffled:
        assert (got["status"] == 1).sum() == 6 and all(numpy.isnan(got[k][got["status"] == 1]).all() for k in spec.FIELDS[1:-1])
        assert (got["reserved"] == 0).all()
        assert (got["row"][fitted] == 0).any() and (got["row"][fitted] == len(K_ROWS) - 1).any()      # both edges of the table
        assert (got["row"][fitted] != got["row_first"][fitted]).any() and (got["row"][fitted] == got["row_first"][fitted]).any()


# ---- members beyond the LDS -------------------------------------------------------------------------------------------------
def test_more_members_than_the_lds_holds(ctx):
    """n = 2600, d = 0.24 P, window 1.9: 2371 members, two tiles staged from device scratch, over two rounds of units."""
    dt = 1 / 64.0
    t = series(2600, dt=dt)
    P, d = 8.0, 1.92
    rng = numpy.random.RandomState(8)
    y = transit_model.light_curve(t, t[0] + 3.0, P, 0.07, 3.0, 88.0, 0, 90, [0.4, 0.4], "quadratic") + rng.normal(0, 1e-4, len(t))
    got = check(ctx, t, y, 1e-4, [P], [t[0] + 3.0], [d], [3], profile(1024), TABLES[315], spec.sub_offsets(dt, 3), window=1.9,
                label="beyond")
    assert got["status"][0] == 0 and got["n_points"][0] > _lib.SHAPE_LDS_MEMBERS


@pytest.mark.parametrize("half_way, members", [(True, 2048), (False, 2049)])
def test_the_capacity_of_the_lds_and_one_more(ctx, half_way, members):
    """One epoch, d = 8 d, window 2: 2048 members with T0 half-way between two stamps (exactly what the LDS holds), 2049 with
    T0 on one (one tile more)."""
    dt = 1 / 64.0
    t = series(2600, dt=dt)
    T0 = t[1300] + (dt / 2 if half_way else 0.0)
    rng = numpy.random.RandomState(9)
    y = transit_model.light_curve(t, T0, 64.0, 0.07, 3.0, 89.0, 0, 90, [0.4, 0.4], "quadratic") + rng.normal(0, 1e-4, len(t))
    got = check(ctx, t, y, 1e-4, [64.0], [T0], [8.0], [3], profile(16), TABLES[27], spec.sub_offsets(0, 1), window=2.0,
                label=members)
    assert members - 1 <= _lib.SHAPE_LDS_MEMBERS <= members
    assert got["n_points"][0] == members and got["status"][0] == 0


# ---- slabs, poison and reuse ------------------------------------------------------------------------------------------------
def test_two_slabs(ctx):
    """520 candidates: the slab of _lib.TRANSIT_FIT_SLAB = 512 (tls_transit_fit.hip.h kTransitSlab) is cut in the middle of
    the shuffled curves; the tail alone returns the same bits."""
    t, y, dy, period, T0, duration, rows, curve = base()
    n_fits = _lib.TRANSIT_FIT_SLAB + 8
    pick = numpy.random.RandomState(3).randint(0, 40, n_fits)
    args = [v[pick] for v in (period, T0, duration, rows)]
    tables, sub = TABLES[27], spec.sub_offsets(0, 1)
    got = check(ctx, t[:330], y[:, :330], dy[:, :330], *args, profile(16), tables, sub, curve=curve[pick], label="slabs")
    assert (got["status"] == 0).sum() > 300 and (got["status"] == 1).sum() > 20
    k_rows, table = profile(16)
    tail = ctx.transit_fit(t[:330], y[:, :330], dy[:, :330], *(v[500:] for v in args), k_rows, table, *tables, sub,
                           curve=curve[pick][500:])
    assert tail.tobytes() == got[500:].tobytes()


def test_poisoned_lds_and_reused_scratch(ctx):
    """The same call before and after tls_debug_poison_lds (every CU's LDS and the call's device buffers smeared) agrees byte
    for byte; the small call behind the large one reuses the buffers and agrees."""
    t, y, dy, period, T0, duration, rows, curve = base()
    small = (t, y, dy, period, T0, duration, rows) + profile(16) + TABLES[27] + (spec.sub_offsets(0, 1),)
    large = (t, y, dy, period, T0, duration, rows) + profile(1024) + TABLES[315] + (spec.sub_offsets(DT, 3),)
    first_small = ctx.transit_fit(*small, curve=curve)
    first_large = ctx.transit_fit(*large, curve=curve)
    ctx.poison_lds(0x7FF80000)
    again_small = ctx.transit_fit(*small, curve=curve)
    ctx.poison_lds(0x7FF80000)
    again_large = ctx.transit_fit(*large, curve=curve)
    behind = ctx.transit_fit(*small, curve=curve)
    assert first_small.tobytes() == again_small.tobytes() == behind.tobytes()
    assert first_large.tobytes() == again_large.tobytes()
    assert (first_small["status"] == 0).sum() >= 28 and first_small.tobytes() != first_large.tobytes()[:first_small.nbytes]


# ---- the entry's arguments --------------------------------------------------------------------------------------------------
def test_c_entry_arguments(ctx):
    """n_fits == 0 is a no-op; every TLS_E_ARG case returns before any device work with the output untouched."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    n = 257
    t = series(n)
    k_rows, table = profile(16)
    good = dict(t=t, y=numpy.ones((2, n)), dy=numpy.full((2, n), 1e-3), n_curves=2, curve=[1], period=[1.0], T0=[1.5],
                duration=[0.1], row_first=[2], n_fits=1, k_rows=k_rows, profile=table, M=16, impact=[0.0, 0.5],
                ratio=[0.8, 1.0], shift=[-0.1, 0.1], sub=[-0.005, 0.005], window=1.0, min_count=3, delta=1.0)
    out = numpy.full(1, -7.0, dtype=_lib.TRANSIT_FIT_DTYPE)

    def call(**kw):
        a = dict(good, **kw)
        f8 = {k: _lib._f8(a[k]) for k in ("t", "y", "dy", "period", "T0", "duration", "k_rows", "profile", "impact", "ratio",
                                          "shift", "sub")}
        curve, rows = _lib._i8(a["curve"]), _lib._i8(a["row_first"])
        return lib.tls_transit_fit(ctx._h, dp(f8["t"]), dp(f8["y"]), dp(f8["dy"]), len(f8["t"]), a["n_curves"], ip(curve),
                                   dp(f8["period"]), dp(f8["T0"]), dp(f8["duration"]), ip(rows), a["n_fits"], dp(f8["k_rows"]),
                                   dp(f8["profile"]), len(f8["k_rows"]), a["M"], dp(f8["impact"]), len(f8["impact"]),
                                   dp(f8["ratio"]), len(f8["ratio"]), dp(f8["shift"]), len(f8["shift"]), dp(f8["sub"]),
                                   len(f8["sub"]), a["window"], a["min_count"], a["delta"], out.ctypes.data_as(ctypes.c_void_p))

    def untouched():
        return all((out[k] == -7.0).all() for k in out.dtype.names)

    assert call(n_fits=0) == 0 and untouched()
    late, nan, inf = t.copy(), numpy.nan, numpy.inf
    late[100] = late[99] - DT
    bad_t = t.copy()
    bad_t[5] = nan
    bad_profile = table.copy()
    bad_profile[3, 4] = nan
    for kw in (dict(curve=[2]), dict(curve=[-1]), dict(row_first=[-1]), dict(row_first=[len(k_rows)]), dict(ratio=[1.0, 0.5]),
               dict(ratio=[0.0, 1.0]), dict(ratio=[nan]), dict(ratio=[]), dict(impact=[0.5, 0.0]), dict(impact=[-0.1, 0.5]),
               dict(impact=[0.0, 1.0]), dict(impact=[]), dict(shift=[0.1, -0.1]), dict(shift=[inf]), dict(sub=[nan]),
               dict(sub=[]), dict(sub=numpy.zeros(17)), dict(M=0), dict(M=4097), dict(k_rows=-k_rows[::-1]),
               dict(k_rows=k_rows[::-1]), dict(profile=bad_profile), dict(impact=numpy.linspace(0.0, 0.9, 16385)),
               dict(window=0.59), dict(window=0.62), dict(window=nan), dict(window=inf), dict(min_count=0), dict(delta=-1e-9),
               dict(delta=nan), dict(t=late), dict(t=bad_t), dict(n_fits=-1), dict(n_curves=-1)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"transit fit" in lib.tls_last_error(ctx._h), kw
    # (0.5 * 1.0 + 0.1 = 0.6 of d = 0.1 plus half an exposure of 0.005 d is 0.65 of d: window 0.66 holds it, 0.62 does not)
    assert call(window=0.66) == 0
    assert call() == 0 and out["status"][0] == 2 and out["n_points"][0] > 0 and not untouched()      # (constant flux)
    assert call(duration=[nan], window=0.6) == 0 and out["status"][0] == 1   # (no duration: nothing for the window to hold)
    empty = ctx.transit_fit(t, numpy.ones((2, n)), numpy.ones((2, n)), [], [], [], [], k_rows, table, *TABLES[27], [0.0], curve=[])
    assert empty.shape == (0,)


# ---- survey.transit_fit and the pipeline -------------------------------------------------------------------------------------
def test_pipeline(ctx):
    """power_batch(peaks=3, peak_fits=True, transit_fit=True) on 5 curves of 700 points: the fit_ fields equal
    survey.transit_fit on the returned peaks, which equals the statement; every other key equals the call without the keyword
    byte for byte."""
    t = 3.0 + numpy.arange(700) / 48.0
    rows = []
    for s in range(5):
        rng = numpy.random.RandomState(2000 + s)
        f = transit_model.light_curve(t, t[0] + 0.3 + 0.2 * s, 1.9 + 0.3 * s, 0.06 + 0.01 * s, 7.0 + s, 89.5, 0, 90,
                                      [0.4, 0.3], "quadratic")
        rows.append(f + rng.normal(0, 3e-4, len(t)))
    flux = numpy.array(rows)
    request = dict(window=1.5)                         # (wide enough for half an exposure beside the shortest fitted duration)
    kw = dict(period_min=1, period_max=5, oversampling_factor=1, u=[0.4, 0.3])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        more = dict(context=ctx, peaks=3, peak_fits=True, **kw)
        summary, periods, pk = survey.power_batch(t, flux, transit_fit=request, **more)
        without = survey.power_batch(t, flux, **more)
    peaks = pk["peaks"]
    names = survey.transit_fit_fields()
    assert peaks.shape == (5, 3) and peaks.dtype.names[-len(names):] == names
    assert summary.dtype == without[0].dtype and summary.tobytes() == without[0].tobytes()
    expect_equal(periods, without[1], "periods")
    assert set(pk) == set(without[2]) and peaks.dtype.names[:-len(names)] == without[2]["peaks"].dtype.names
    expect_equal(pk["n_peaks"], without[2]["n_peaks"], "n_peaks")
    for k in without[2]["peaks"].dtype.names:
        assert peaks[k].tobytes() == without[2]["peaks"][k].tobytes(), k
    curve, rank = numpy.nonzero(peaks["status"] == 0)
    assert len(curve) >= 5
    args = (peaks["period"][curve, rank], peaks["T0"][curve, rank], peaks["duration_days"][curve, rank],
            1.0 - peaks["depth"][curve, rank])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alone = survey.transit_fit(t, flux, *args, curve=curve, context=ctx, u=[0.4, 0.3], **request)
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, None, dict(oversampling_factor=1))
    assert alone.dtype.names == names
    for k in names:
        expect_equal(peaks[k][curve, rank], alone[k], k)
    k_rows, table = survey.transit_profile(u=[0.4, 0.3])
    seed = [spec.nearest_row(k_rows, float(numpy.sqrt(v))) for v in args[3]]
    want = spec.transit_fit_batch(t, y_rows, dy_rows, args[0], args[1], args[2], curve, seed, k_rows, table,
                                  spec.DEFAULT_IMPACTS, spec.DEFAULT_RATIOS, spec.DEFAULT_SHIFTS,
                                  spec.sub_offsets(float(numpy.median(numpy.diff(t))), 5),   # (exposure=None: the median cadence)
                                  window=1.5)
    for i, f in enumerate(spec.FIELDS):
        expect_equal(alone["fit_" + f], want[:, i], f)
    expect_equal(alone["fit_T0"], args[1] + alone["fit_shift"], "T0")
    geometry = survey.transit_fit_geometry(args[0], alone["fit_k"], alone["fit_b"], alone["fit_duration"])
    for k, v in zip(("fit_a_rs", "fit_inc", "fit_rho_star"), geometry):
        expect_equal(alone[k], v, k)
    rest = peaks["status"] != 0
    assert (peaks["fit_status"][rest] == 1).all() and all(numpy.isnan(peaks[k][rest]).all() for k in names[1:] if k != "fit_reserved")
    assert (peaks["fit_status"][:, 0] == 0).all()       # (the injected planets are fitted)
