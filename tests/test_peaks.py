"""Periodogram peaks on the device (tls_find_peaks, tls_power_batch_peaks) against the selection's numpy statement
(tests/peaks_spec.py), bit for bit: the selection copies values, no arithmetic reaches its output."""
import warnings
from fractions import Fraction

import numpy
import pytest

import peaks_spec
from tls_amd import _lib, survey, transit_model
from tls_amd.planning import search_inputs

pytestmark = pytest.mark.gpu

SIXTEEN = tuple(float(x) for x in (0.5, 2.0, 1 / 3, 3.0, 2 / 3, 1.5, 0.25, 4.0, 0.2, 5.0, 0.75, 4 / 3, 0.4, 2.5, 0.6, 5 / 3))


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_rows(ctx, power, periods, k, sep, ratios, min_power=None, chi2=None, row=None, depth=None, label=""):
    """find_peaks on the device equals the spec on every row: bytes of index, period, power (and chi2, depth, row), n_peaks,
    NaN and -1 past n_peaks."""
    power = numpy.atleast_2d(power)
    got, n_got = ctx.find_peaks(power, periods, k, sep, ratios, min_power, chi2=chi2, row=row, depth=depth)
    assert got.shape == (len(power), k) and n_got.shape == (len(power),)
    for r in range(len(power)):
        want, m = peaks_spec.expected(power[r], periods, k, sep, ratios, min_power,
                                      *(None if a is None else numpy.atleast_2d(a)[r] for a in (chi2, row, depth)))
        assert n_got[r] == m, (label, r, n_got[r], m)
        for name in want.dtype.names:
            assert same_bits(got[r][name][:m], want[name][:m]), (label, r, name, got[r][name], want[name])
        for name in ("period", "power", "chi2", "depth"):
            assert numpy.isnan(got[r][name][m:]).all(), (label, r, name)
            if chi2 is None and name == "chi2" or depth is None and name == "depth":
                assert numpy.isnan(got[r][name]).all(), (label, r, name)
        assert (got[r]["index"][m:] == -1).all() and (got[r]["row"][m:] == -1).all(), (label, r)
        if row is None:
            assert (got[r]["row"] == -1).all()
    return got, n_got


def crafted_rows(n, seed):
    """Ties and plateaus everywhere (eight integer values), the monotone and constant rows, NaNs at the ends and inside."""
    rng = numpy.random.RandomState(seed)
    rows = [rng.randint(0, 8, n).astype(numpy.float64) for _ in range(4)]
    rows += [numpy.full(n, 3.0), numpy.arange(n, dtype=numpy.float64), -numpy.arange(n, dtype=numpy.float64)]
    for where in ([0], [n - 1], [n // 2], [0, n - 1, n // 2, n // 3], list(range(0, n, 5))):
        r = rng.randint(0, 8, n).astype(numpy.float64)
        r[where] = numpy.nan
        rows.append(r)
    smooth = numpy.convolve(rng.normal(0, 1, n + 8), numpy.ones(9) / 9, mode="valid")
    rows.append(smooth)
    rows.append(numpy.where(rng.uniform(size=n) < 0.1, -numpy.inf, smooth))
    return numpy.array(rows)


def grid(n, descending=False):
    periods = 0.6 * (40.0 / 0.6) ** (numpy.arange(n) / max(n - 1, 1))   # 0.6 .. 40 d, 4.2 octaves: every ratio lands inside
    return periods[::-1].copy() if descending else periods


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_crafted_rows_at_the_wave_and_workgroup_edges(ctx, n):
    rows = crafted_rows(n, seed=n)
    for descending in (False, True):
        periods = grid(n, descending)
        for k in (1, 3, 32):
            for ratios in ((), peaks_spec.HARMONICS, SIXTEEN):
                _, n_got = check_rows(ctx, rows, periods, k, 0.02, ratios, label=(n, descending, k, len(ratios)))
        assert n_got[4] == 1 and n_got[5] == 1 and n_got[6] == 1       # constant, ascending, descending: one candidate
    # a threshold above every value, and one that splits the values
    _, n_got = check_rows(ctx, rows, grid(n), 32, 0.02, peaks_spec.HARMONICS, min_power=1e300, label=(n, "above"))
    assert (n_got == 0).all()
    check_rows(ctx, rows, grid(n), 32, 0.0, (), min_power=4.0, label=(n, "split"))
    # the search's values ride along
    rng = numpy.random.RandomState(n + 1)
    chi2, depth = rng.uniform(900, 1000, rows.shape), rng.uniform(0.99, 1.0, rows.shape)
    row = rng.randint(0, 300, rows.shape).astype(numpy.int64)
    check_rows(ctx, rows, grid(n), 3, 0.02, peaks_spec.HARMONICS, chi2=chi2, row=row, depth=depth, label=(n, "values"))
    check_rows(ctx, rows, grid(n), 3, 0.02, peaks_spec.HARMONICS, row=row, label=(n, "row alone"))


@pytest.mark.parametrize("n_rows", [1, 33, 97])
def test_row_counts(ctx, n_rows):
    rng = numpy.random.RandomState(n_rows)
    power = rng.randint(0, 8, (n_rows, 257)).astype(numpy.float64) + numpy.round(rng.uniform(size=(n_rows, 257)), 1)
    _, n_got = check_rows(ctx, power, grid(257), 32, 0.01, peaks_spec.HARMONICS, label=n_rows)
    assert n_got.min() >= 4
    one, n_one = survey.find_peaks(power[0], grid(257), 5, context=ctx)
    many, n_many = survey.find_peaks(power, grid(257), 5, context=ctx)
    assert one.shape == (5,) and many.shape == (n_rows, 5) and same_bits(one, many[0]) and n_one == n_many[0]
    assert ctx.find_peaks(numpy.zeros((0, 257)), grid(257), 5)[0].shape == (0, 5)     # no rows: a no-op


def test_an_index_exactly_on_a_windows_edge(ctx):
    """Dyadic periods: r * P, sep * r * P and periods[i] - r * P are all exact, and fabs(periods[i] - r * P) == sep * r * P at
    some index for every ratio used -- the index leaves with `<=`.  One step further out (one ulp) it stays."""
    sep = 2.0 ** -5
    P = 4.0
    ratios = (0.5, 2.0, 1.5)
    edges = []
    for r in (1.0,) + ratios:
        c = r * P
        edges += [c + sep * c, c - sep * c, numpy.nextafter(c + sep * c, numpy.inf), numpy.nextafter(c - sep * c, 0.0)]
    periods = numpy.array([P] + edges + [64.0])
    n = len(periods)
    # every period its own candidate: values between zeros, the peak at P the highest
    wide = numpy.zeros(2 * n + 1)
    wide_periods = numpy.full(2 * n + 1, 1000.0)
    wide[1::2] = numpy.arange(n, 0, -1) + 10.0
    wide_periods[1::2] = periods
    wide_periods[0::2] = 1000.0 + numpy.arange(n + 1)
    on_edge = [i for i in range(len(wide_periods)) for r in (1.0,) + ratios
               if i != 1 and numpy.fabs(wide_periods[i] - r * P) == sep * (r * P)]
    assert len(on_edge) == 8                                              # such indices exist: two per window
    inside = peaks_spec.windows(wide_periods, P, sep, ratios)
    assert inside[on_edge].all() and inside.sum() == 9                    # P itself and the eight edges; the ulp-further ones stay
    got, n_got = check_rows(ctx, wide, wide_periods, 32, sep, ratios, label="dyadic edge")
    taken = set(got[0]["index"][:n_got[0]].tolist())
    assert 1 in taken and not taken & set(on_edge)
    assert n_got[0] >= 2


def contraction_cases(r, sep, count, seed):
    """Periods P and per = fl(c + w) (c = fl(r P), w = fl(sep c)) for which the test `fabs(per - c) <= w` in three IEEE
    operations and the same test with per - r P fused into one rounding disagree: an FMA flips the index."""
    rng = numpy.random.RandomState(seed)
    found = []
    while len(found) < count or len({plain for _, _, plain in found}) < 2:
        P = float(rng.uniform(1.0, 2.0))
        c = r * P
        w = sep * c
        for per in (c + w, numpy.nextafter(c + w, 0.0), numpy.nextafter(c + w, 4.0), c - w, numpy.nextafter(c - w, 0.0)):
            per = float(per)
            plain = abs(per - c) <= w
            fused = abs(float(Fraction(per) - Fraction(r) * Fraction(P))) <= w
            if plain != fused:
                found.append((P, per, plain))
                break
    return found


def test_windows_are_not_contracted(ctx):
    """periods[i] - r * P with an inexact product: where a fused multiply-add would decide the edge the other way, the
    device decides as the three separate operations do."""
    r, sep = 1 / 3, 0.02
    cases = contraction_cases(r, sep, 12, seed=5)
    assert {plain for _, _, plain in cases} == {True, False}               # flips in both directions are covered
    for P, per, plain in cases:
        periods = numpy.array([P, 1000.0, per, 2000.0, 3000.0])
        power = numpy.array([5.0, 0.0, 4.0, 0.0, 3.0])
        assert bool(peaks_spec.windows(periods, P, sep, (r,))[2]) == plain
        got, n_got = check_rows(ctx, power, periods, 3, sep, (r,), label=("contraction", P))
        assert got[0]["index"][:n_got[0]].tolist() == ([0, 4] if plain else [0, 2, 4])


def smooth_spectrum(n, seed):
    rng = numpy.random.RandomState(seed)
    x = numpy.cumsum(rng.normal(0, 1, n + 64))
    power = (x[64:] - x[:-64]) / 8.0                                        # a moving sum of 64: broad peaks, few candidates
    power += rng.normal(0, 0.05, n)
    return power


def test_kepler_grid_row(ctx):
    """182 388 periods: the largest grid of the reference's data sets, its alive mask (23 KB) in LDS."""
    n = 182388
    periods = 1.0 / numpy.linspace(1 / 0.6, 1 / 730.0, n)                   # ascending, uniform in frequency
    power = smooth_spectrum(n, 11)
    _, n_got = check_rows(ctx, power, periods, 32, 0.02, peaks_spec.HARMONICS, label="kepler")
    assert n_got[0] == 32
    check_rows(ctx, power[::-1].copy(), periods[::-1].copy(), 8, 0.002, SIXTEEN, label="kepler descending")


def test_one_row_past_the_lds_mask(ctx):
    """One period more than the mask in LDS takes (PEAKS_LDS_PERIODS): the same selection with the mask in device memory;
    and the last grid on the LDS side."""
    for n in (_lib.PEAKS_LDS_PERIODS + 1, _lib.PEAKS_LDS_PERIODS):
        periods = 1.0 / numpy.linspace(1 / 0.6, 1 / 730.0, n)
        power = smooth_spectrum(n, 13)
        power[-1] = power.max() + 1.0                                       # the very last index is the first peak
        got, n_got = check_rows(ctx, power, periods, 8, 0.02, peaks_spec.HARMONICS, label=("mask", n))
        assert n_got[0] == 8 and got[0]["index"][0] == n - 1


# ---- the pipeline: power_batch(peaks=K) --------------------------------------------------------------------------------
T960 = numpy.linspace(3.14, 23.14, 960)          # 20 days at 48 a day


def curves(t, n_curves, seed, flat=()):
    """Light curves on shared time stamps, one planet each, white noise of 4e-4; those in `flat` fit nothing."""
    rng = numpy.random.RandomState(seed)
    rows = []
    for s in range(n_curves):
        f = transit_model.light_curve(t, t[0] + 0.2 + rng.uniform(0, 1), float(rng.uniform(1.5, 5.0)), float(rng.uniform(0.03, 0.08)),
                                      12, 89.8, 0, 90, [0.4, 0.3], "quadratic") + rng.normal(0, 4e-4, len(t))
        if s in flat:
            f = numpy.ones(len(t))
            f[::7] += 1e-7
        rows.append(f)
    return numpy.array(rows)


def run(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return survey.power_batch(*args, **kwargs)


def check_pipeline(ctx, t, flux, k=8, **kw):
    """power_batch(peaks=k, with_arrays=True): the peaks are the spec on the returned power, the other fields gathered from
    the returned arrays; the first peak is index_power; a no-fit curve has none; duration from the table."""
    summary, periods, chi2, row, depth, power, pk = run(t, flux, context=ctx, with_arrays=True, peaks=k, **kw)
    peaks, n_peaks = pk["peaks"], pk["n_peaks"]
    assert peaks.shape == (len(flux), k) and n_peaks.shape == (len(flux),)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        duration = search_inputs(t, flux[0], **kw)["table"].duration
    for c in range(len(flux)):
        if summary["no_fit"][c]:
            assert n_peaks[c] == 0
            want, m = peaks_spec.expected(power[c], periods, k, min_power=numpy.inf)
        else:
            want, m = peaks_spec.expected(power[c], periods, k, 0.02, peaks_spec.HARMONICS, None, chi2[c], row[c], depth[c])
            assert m >= 1 and peaks[c]["index"][0] == summary["index_power"][c]
        assert n_peaks[c] == m, (c, n_peaks[c], m)
        for name in want.dtype.names:
            assert same_bits(peaks[c][name], want[name]), (c, name, peaks[c][name], want[name])
        assert same_bits(peaks[c]["duration"][:m], duration[want["row"][:m]]) and numpy.isnan(peaks[c]["duration"][m:]).all()
    return summary, peaks, n_peaks


@pytest.mark.parametrize("n_curves,flat", [(1, ()), (1, (0,)), (32, (0, 31)), (33, (0, 32)), (65, (0, 64))])
def test_pipeline_batches(ctx, n_curves, flat):
    flux = curves(T960, n_curves, seed=n_curves, flat=flat)
    summary, peaks, n_peaks = check_pipeline(ctx, T960, flux, period_max=6.0)
    assert summary["no_fit"].nonzero()[0].tolist() == list(flat)
    fit = summary["no_fit"] == 0
    assert (n_peaks[fit] >= 2).all()


def same_fields(a, b):
    """Structured arrays equal field by field: NaNs at the same places, the same bits elsewhere."""
    assert a.dtype == b.dtype and a.shape == b.shape
    for name in a.dtype.names:
        x, y = a[name], b[name]
        if x.dtype.kind == "f":
            assert (numpy.isnan(x) == numpy.isnan(y)).all(), name
            x, y = numpy.where(numpy.isnan(x), 0.0, x), numpy.where(numpy.isnan(y), 0.0, y)
        assert same_bits(x, y), name


def test_nothing_else_moves(ctx):
    flux = curves(T960, 40, seed=77, flat=(0, 39))
    kw = dict(period_max=6.0, context=ctx)
    plain = run(T960, flux, **kw)
    with_peaks = run(T960, flux, peaks=8, **kw)
    assert len(with_peaks) == len(plain) + 1
    same_fields(with_peaks[0], plain[0])
    assert same_bits(with_peaks[1], plain[1])
    stats = run(T960, flux, statistics=True, per_transit=True, **kw)
    stats_peaks = run(T960, flux, statistics=True, per_transit=True, peaks=8, **kw)
    assert len(stats_peaks) == len(stats) + 1
    same_fields(stats_peaks[0], stats[0])
    for name in stats[2]:
        x, y = stats[2][name], stats_peaks[2][name]
        assert (numpy.isnan(x) == numpy.isnan(y)).all() and same_bits(numpy.nan_to_num(x), numpy.nan_to_num(y)), name
    # statistics without the per-transit rows: the records lie elsewhere on the device, the results do not move
    stats_only = run(T960, flux, statistics=True, peaks=8, **kw)
    same_fields(stats_only[0], stats[0])
    for other in (stats_peaks, stats_only):
        same_fields(other[-1]["peaks"], with_peaks[-1]["peaks"])
        assert same_bits(other[-1]["n_peaks"], with_peaks[-1]["n_peaks"])
    # two contexts on one device, the batch dealt out: what one context returns
    two = run(T960, flux, peaks=8, period_max=6.0, devices=[0, 0])
    same_fields(two[0], with_peaks[0])
    same_fields(two[-1]["peaks"], with_peaks[-1]["peaks"])
    assert same_bits(two[-1]["n_peaks"], with_peaks[-1]["n_peaks"])
    # detrending in front, other peak arguments
    flat = run(T960, flux, peaks=3, peak_separation=0.05, peak_ratios=(), peak_min_power=5.0, detrend=25, **kw)
    assert flat[-1]["peaks"].shape == (40, 3)
    strong = flat[-1]["peaks"]["power"]
    assert (strong[~numpy.isnan(strong)] >= 5.0).all()


def test_two_planets():
    """Planets at 1.9 d and 3.1 d in eight noise realisations: with the harmonic windows the second planet is the second
    peak; without them its rank is taken by harmonics of the first (the CPU oracle had it at rank 5 to 7)."""
    t = T960
    clean = transit_model.light_curve(t, 3.3, 1.9, 0.07, 12, 89.8, 0, 90, [0.4, 0.3], "quadratic") \
        * transit_model.light_curve(t, 3.9, 3.1, 0.05, 15, 89.8, 0, 90, [0.4, 0.3], "quadratic")
    flux = numpy.array([clean + numpy.random.RandomState(s).normal(0, 4e-4, 960) for s in range(8)])
    with_h = run(t, flux, peaks=8, period_max=6.0)[-1]
    assert (with_h["n_peaks"] >= 2).all()
    first, second = with_h["peaks"]["period"][:, 0], with_h["peaks"]["period"][:, 1]
    print("two planets, HARMONICS: first", first, "second", second)
    assert (numpy.abs(first - 1.9) <= 0.02 * 1.9).all(), first
    assert (numpy.abs(second - 3.1) <= 0.02 * 3.1).all(), second
    without = run(t, flux, peaks=8, period_max=6.0, peak_ratios=())[-1]
    top3 = without["peaks"]["period"][:, :3]
    print("two planets, no ratios: first three", top3)
    assert not (numpy.abs(top3 - 3.1) <= 0.02 * 3.1).any(), top3


def test_one_context_across_two_grid_sizes(ctx):
    """A context reused across grids of different sizes (buffers grown, then reused smaller): each size's own peaks."""
    t_b = numpy.linspace(3.0, 33.0, 720)
    for t, kw, seed in ((T960, dict(period_max=6.0), 1), (t_b, dict(period_min=1.5, period_max=9.0, oversampling_factor=2), 2),
                        (T960, dict(period_max=6.0), 3)):
        check_pipeline(ctx, t, curves(t, 5, seed=seed, flat=(4,)), k=4, **kw)
