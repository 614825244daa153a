"""The ephemeris match on the device (survey.ephemeris_match / tls_ephemeris_match; power_batch(peaks=K, peak_fits=True,
ephemeris_match=True)) against tests/ephemeris_match_spec.py bit for bit: the standalone entry at the edges of the kernel (its
tile, the chunks of the other side) and of the statement (the by-hand boundary cases, one star, ties, bad candidates), and the
pipeline across the group edge, with every other result untouched."""
import ctypes
import warnings

import numpy
import pytest

import ephemeris_match_spec as spec
from tls_amd import _lib, survey, synthetic, transit_model

pytestmark = pytest.mark.gpu

TILE = _lib.MATCH_TILE
# the light curves and keywords of tests/test_peak_fits.py
T = numpy.linspace(3.0, 43.0, 1920)          # 40 d at 30 min
KW = dict(period_min=1, period_max=5, oversampling_factor=1)
PLANETS = ((1.9, 8.0), (3.1, 11.0))          # period [d], a / R_star


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, args, label="", **kw):
    """survey.ephemeris_match of the candidates equals the statement, field by field; the device's records."""
    got = survey.ephemeris_match(*args, context=ctx, **kw)
    want = spec.match(*args, **kw)
    assert got.shape == want.shape and got.dtype.names == survey.ephemeris_match_fields() == spec.FIELDS
    for k in spec.FIELDS:
        numpy.testing.assert_array_equal(got[k], want[k], err_msg=str((label, k)))
    return got


def with_clusters(args, edges, half=9):
    """The candidates with a run of IDENTICAL ones (distinct stars, one strength: every tie goes to the lowest index) laid
    across each of `edges`."""
    star, period, T0, duration, strength, span = (numpy.array(a) if numpy.ndim(a) else a for a in args)
    for e in edges:
        run = slice(max(0, e - half), min(len(star), e + half))
        star[run] = 10 ** 6 + numpy.arange(len(star))[run]
        period[run], T0[run], duration[run], strength[run] = 2.5, 1.25, 0.125, 0.5
    return star, period, T0, duration, strength, span


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_candidate_counts(ctx, n):
    got = check(ctx, spec.clustered(n, n), n)
    assert n < 8 or got["n_match"].sum() > n // 2


@pytest.mark.parametrize("n", [3 * TILE + 5, 17 * TILE + 5])
def test_matches_across_tiles_and_chunks(ctx, n):
    """3 T + 5: four chunks of a tile each; 17 T + 5: eighteen tiles in sixteen chunks, two of them of two tiles.  A run of
    identical candidates lies across every tile edge -- inside a chunk and between two -- so counts add up over the chunks and
    the tie for the best goes to the lowest index wherever it lies."""
    edges = _lib.match_chunks(n)
    sizes = numpy.diff(edges[:-1])
    assert (len(edges) - 1, sorted(set(sizes))) == ((4, [TILE]) if n == 3 * TILE + 5 else (16, [TILE, 2 * TILE]))
    tile_edges = list(range(TILE, n, TILE))
    assert set(edges[1:-1]) <= set(tile_edges) and (n < 8 * TILE or set(edges[1:-1]) < set(tile_edges))
    args = with_clusters(spec.clustered(7, n, n_stars=1024), tile_edges)
    got = check(ctx, args, n)
    members = numpy.flatnonzero(args[1] == 2.5)
    assert len(members) >= 14 * len(tile_edges)
    assert (got["n_match"][members] >= len(members) - 1).all()
    assert (got["n_match"] > 0).mean() > 0.5 and (got["best"] > numpy.arange(n)).any() and (got["best"] >= 0).sum() > n // 2


def test_all_on_one_star(ctx):
    star, period, T0, duration, strength, span = spec.clustered(3, 2 * TILE + 1)
    got = check(ctx, (numpy.full(len(star), -5), period, T0, duration, strength, span), "one star")
    assert (got["status"] == 0).all()
    for k in ("n_same", "n_period", "n_match"):
        assert (got[k] == 0).all()
    assert (got["best"] == -1).all() and numpy.isnan(got["child"]).all()


def test_ties(ctx):
    """All identical on distinct stars: everyone matches everyone, the best is the lowest index -- 1 for candidate 0."""
    n = 2 * TILE + 1
    one = numpy.ones(n)
    got = check(ctx, (numpy.arange(n) * 2 ** 40, 3.0 * one, 4.0 * one, 0.1 * one, 0.25 * one, 40.0), "ties")
    for k in ("n_same", "n_period", "n_match"):
        assert (got[k] == n - 1).all()
    numpy.testing.assert_array_equal(got["best"], [1] + [0] * (n - 1))
    assert (got["child"] == 0).all() and (got["best_ratio"] == 1).all() and (got["best_dt"] == 0).all()


@pytest.mark.parametrize("case", spec.by_hand(), ids=lambda c: c[0])
def test_boundary_cases_by_hand(ctx, case):
    name, kw, want = case
    got = survey.ephemeris_match(context=ctx, **kw)
    for k in spec.FIELDS:
        numpy.testing.assert_array_equal(got[k], want[k], err_msg=str((name, k)))


def test_bad_candidates_mixed_in(ctx):
    """Every kind of bad candidate among matching ones, across two tiles: status 1, NaN, and nobody sees them; extreme but
    good values (a period ratio that overflows, a denormal period) go through the arithmetic as the statement has it."""
    star, period, T0, duration, strength, span = (numpy.array(a) if numpy.ndim(a) else a for a in spec.clustered(11, TILE + 40))
    rng = numpy.random.RandomState(0)
    bad = rng.choice(len(star), 60, replace=False)
    values = [numpy.nan, numpy.inf, -numpy.inf, 0.0, -1.0]
    for i, f in enumerate(bad[:40]):
        (period, T0, duration, strength)[i % 4][f] = values[(i // 4) % 5]
    period[bad[40:44]] = [1e308, 1e-308, 5e-324, 1.7976931348623157e308]
    T0[bad[44:46]] = [1e308, -1e308]
    duration[bad[46:48]] = [5e-324, 1e308]
    strength[bad[48:50]] = [-1e308, 1e308]
    got = check(ctx, (star, period, T0, duration, strength, span), "bad")
    assert (got["status"] == 1).sum() == 32 and (got["n_match"][got["status"] == 0] > 0).sum() > TILE // 2
    assert numpy.isnan(got["best"][got["status"] == 1]).all()


@pytest.mark.parametrize("kw", [dict(drift_tolerance=0.0, epoch_tolerance=0.0), dict(max_ratio=1), dict(max_ratio=64),
                                dict(drift_tolerance=3.0, epoch_tolerance=0.125, max_ratio=2)], ids=str)
def test_tolerances_and_ratios(ctx, kw):
    check(ctx, spec.clustered(5, TILE + 3), kw, **kw)


@pytest.mark.parametrize("seed", [0, 1])
def test_a_diluted_binary_on_the_device(ctx, seed):
    args, members = spec.field(seed)
    got = check(ctx, args, "field")
    assert (survey.ephemeris_groups(got)[members] == members[0]).all() and (got["n_match"].sum() == 6)


def test_c_entry_arguments(ctx):
    """n == 0 is a no-op, null pointers and all; TLS_E_ARG before any device work for a bad span, tolerance, max_ratio or n."""
    lib, dp, ip = ctx._lib, _lib._dp, _lib._ip
    star, two = _lib._i8([0, 1]), _lib._f8([2.0, 2.0])
    out = numpy.full(2, -7.0, dtype=_lib.MATCH_DTYPE)

    def call(n=2, span=40.0, drift=0.5, epoch=0.5, max_ratio=3):
        return lib.tls_ephemeris_match(ctx._h, ip(star), dp(two), dp(two), dp(two), dp(two), n, span, drift, epoch, max_ratio,
                                       out.ctypes.data_as(ctypes.c_void_p))
    assert call(n=0) == 0 and out["status"][0] == -7.0
    assert lib.tls_ephemeris_match(ctx._h, None, None, None, None, None, 0, 40.0, 0.5, 0.5, 3, None) == 0
    for kw in (dict(span=0.0), dict(span=-1.0), dict(span=numpy.inf), dict(span=numpy.nan), dict(drift=-0.5), dict(drift=numpy.nan),
               dict(epoch=-0.5), dict(epoch=numpy.inf), dict(max_ratio=0), dict(max_ratio=65), dict(n=-1),
               dict(n=_lib.MATCH_MAX_CANDIDATES + 1)):
        assert call(**kw) == -1, kw                   # TLS_E_ARG
        assert out["status"][0] == -7.0
    assert lib.tls_ephemeris_match(ctx._h, None, dp(two), dp(two), dp(two), dp(two), 2, 40.0, 0.5, 0.5, 3,
                                   out.ctypes.data_as(ctypes.c_void_p)) == -1
    assert call() == 0
    numpy.testing.assert_array_equal(out["n_match"], [1, 1])
    assert len(survey.ephemeris_match([], [], [], [], [], 40.0, context=ctx)) == 0


def test_a_prepared_plan_stays(ctx):
    t, flux = synthetic.light_curve(30.0, 24, 2e-4, per=4.321, rp=0.05, a=12)
    inp = synthetic.search_inputs(t, flux, period_min=3.5, period_max=5.5, oversampling_factor=2)
    ctx.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    ctx.execute()
    first = ctx.fetch()
    check(ctx, spec.clustered(2, TILE + 1), "between two executes")
    ctx.execute()
    for a, b in zip(first, ctx.fetch()):
        numpy.testing.assert_array_equal(a, b)


# ---- in the pipeline ----------------------------------------------------------------------------------------------------
BINARY = (0, 16, 32)                         # the curves that carry the eclipse, the deepest first: both launch groups
DILUTION = (1.0, 0.4, 0.15)


def batch(n_curves=33):
    """Noise curves with the two planets of tests/test_peak_fits.py at epochs of their own; the curves BINARY carry ONE deep
    eclipse (P = 2.3 d) instead, at three dilutions."""
    eclipse = transit_model.light_curve(T, T[0] + 0.7, 2.3, 0.2, 7.0, 89.8, 0, 90, [0.4, 0.3], "quadratic") - 1
    rows = []
    for s in range(n_curves):
        rng = numpy.random.RandomState(1000 + s)
        f = numpy.ones(len(T))
        if s in BINARY:
            f += DILUTION[BINARY.index(s)] * eclipse
        else:
            for per, a in PLANETS:
                tp = T[0] + rng.uniform(0.1, 0.9) * per
                f += transit_model.light_curve(T, tp, per, float(rng.uniform(0.05, 0.08)), a, 89.8, 0, 90, [0.4, 0.3],
                                               "quadratic") - 1
        rows.append(f + rng.normal(0, 4e-4, len(T)))
    return numpy.array(rows)


def run(flux, k, **more):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return survey.power_batch(T, flux, peaks=k, peak_fits=True, with_arrays=True, statistics=True, **more, **KW)


@pytest.mark.parametrize("how", [dict(device=0), dict(devices=[0, 0])], ids=["one context", "two contexts"])
def test_pipeline(how):
    flux = batch()
    k = 4
    got = run(flux, k, ephemeris_match=True, **how)
    peaks = got[-1]["peaks"]
    names = survey.ephemeris_match_peak_fields()
    assert peaks.shape == (33, k) and peaks.dtype.names[-len(names):] == names
    # the statement applied to the peaks and fits the call returned
    at = numpy.flatnonzero(peaks["status"].reshape(-1) == 0)
    flat = peaks.reshape(-1)
    assert 2 * 33 <= len(at) < 33 * k                                    # (peaks of status 1 exist: no such peak)
    want = spec.match(at // k, flat["period"][at], flat["T0"][at], flat["duration_days"][at], 1 - flat["depth"][at],
                      numpy.max(T) - numpy.min(T))
    for name, source in zip(names[:4] + names[6:], spec.FIELDS[:4] + spec.FIELDS[5:]):
        numpy.testing.assert_array_equal(flat[name][at], want[source], err_msg=name)
    target = at[numpy.where(want["best"] >= 0, want["best"], 0).astype(int)]
    numpy.testing.assert_array_equal(flat["match_curve"][at], numpy.where(want["best"] >= 0, target // k, -1))
    numpy.testing.assert_array_equal(flat["match_rank"][at], numpy.where(want["best"] >= 0, target % k, -1))
    rest = numpy.setdiff1d(numpy.arange(33 * k), at)
    assert (flat["match_status"][rest] == 1).all() and (flat["match_curve"][rest] == -1).all()
    assert numpy.isnan(flat["match_n_match"][rest]).all() and numpy.isnan(flat["match_child"][rest]).all()
    # the diluted curves' top peak is a child of the deepest curve's
    deep, mid, faint = BINARY
    for c in (mid, faint):
        assert peaks["match_child"][c, 0] == 1 and (peaks["match_curve"][c, 0], peaks["match_rank"][c, 0]) == (deep, 0), c
        assert peaks["match_strength"][c, 0] == 1 - peaks["depth"][deep, 0] and abs(peaks["match_ratio"][c, 0]) == 1
    assert peaks["match_child"][deep, 0] == 0 and peaks["match_curve"][deep, 0] == mid and peaks["match_n_match"][deep, 0] >= 2
    # the planets share two periods and no epoch: a pile-up, not a match
    planets = numpy.setdiff1d(numpy.arange(33), BINARY)
    assert (peaks["match_n_same"][planets, 0] >= 10).all()
    # everything else is the call without the keyword
    without = run(flux, k, **how)
    assert len(got) == len(without) == 7
    assert got[0].dtype == without[0].dtype and got[0].tobytes() == without[0].tobytes()
    for a, b in zip(got[1:6], without[1:6]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert got[-1]["n_peaks"].tobytes() == without[-1]["n_peaks"].tobytes() and set(got[-1]) == set(without[-1])
    before = without[-1]["peaks"]
    assert peaks.dtype.names[:len(before.dtype.names)] == before.dtype.names
    for name in before.dtype.names:                                      # (the peak records and their fits)
        assert peaks[name].tobytes() == before[name].tobytes(), name
