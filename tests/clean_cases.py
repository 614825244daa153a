"""The cases of test_clean_host.py (plain Python against numpy) and test_clean.py (the device against clean_spec): name ->
(t, y [rows, n], bad or None, keywords of clean_spec.clean).  Small on purpose: every path of the statement at the smallest
size at which it can go wrong.  The statement of a case is formed once (expected) and shared."""
import math

import numpy

import clean_spec

INF = math.inf


def series(n, per_day=48.0, gap_at=None, gap=3.0):
    """n time stamps at per_day a day, with a gap of `gap` days in front of index gap_at."""
    t = numpy.arange(n, dtype=numpy.float64) / per_day
    if gap_at is not None:
        t[gap_at:] += gap
    return t


def dirty_rows(n, rows, seed, noise=3e-4, nan_share=0.03, flares=2, dips=2):
    """rows x n: 1 + noise, a transit-like box, NaN / inf / zero / negative values, flares and single low samples."""
    rng = numpy.random.default_rng(seed)
    y = 1.0 + noise * rng.standard_normal((rows, n))
    for r in range(rows):
        if n >= 40:
            a = int(rng.integers(5, n - 12))
            y[r, a:a + 7] -= 5e-3                     # a transit: a run of low samples
        for _ in range(flares if n >= 16 else 0):
            a = int(rng.integers(0, n - 6))
            y[r, a:a + 6] += 1e-2 * numpy.exp(-numpy.arange(6) / 2.0)
        for _ in range(dips if n >= 8 else 0):
            y[r, int(rng.integers(0, n))] -= 3e-3
        k = max(1, int(nan_share * n)) if n >= 3 else 0
        at = rng.choice(n, size=k, replace=False)
        y[r, at] = rng.choice([numpy.nan, numpy.inf, -numpy.inf, 0.0, -1.0, -0.0], size=k)
    return y


# a row whose largest value alone is flagged in every round, sixteen rounds long
ONE_A_ROUND_SIGMA = 3.0


def one_a_round():
    """y [40] for window_length None, sigma_upper = ONE_A_ROUND_SIGMA, sigma_lower inf: the largest value alone is flagged in
    each of 16 rounds (test_clean_host.py checks that the statement says so).  Built from the last round backwards: on top of a
    convex ramp of 24 values, each new top value lies 1 % above the clip of the set it tops -- a top value's size moves neither
    median -- and the ramp is steep enough at its middle that the clip of the next larger set lies above it again."""
    base = [(k / 24.0) ** 2 for k in range(24)]
    for _ in range(16):
        trial = numpy.array(base + [1e9])
        m = clean_spec.median(trial)
        r = trial - m
        c0 = clean_spec.median(r)
        sigma = clean_spec.K_MAD * clean_spec.median(numpy.abs(r - c0))
        base.append(float(m + c0 + ONE_A_ROUND_SIGMA * sigma * 1.01))
    return 1.0 + 1e-3 * numpy.array(base)


def _cases():
    c = {}
    # sizes and row counts, the row's median and a sliding centre; 257, 300 and 1367 points make several tiles at this window
    for n, rows in ((1, 1), (2, 2), (3, 3), (7, 4), (64, 5), (257, 2), (300, 3), (1367, 2)):
        t = series(n, gap_at=(n * 2) // 3 if n >= 7 else None)
        y = dirty_rows(n, rows, seed=n)
        c["flat_n%d" % n] = (t, y, None, dict(sigma_upper=4.0, sigma_lower=5.0, n_iter=5))
        c["slide_n%d" % n] = (t, y, None, dict(window_length=0.5, sigma_upper=4.0, sigma_lower=5.0, n_iter=5))
    t = series(300, gap_at=200)
    y = dirty_rows(300, 2, seed=11)
    c["window_of_one"] = (t, y, None, dict(window_length=1e-3, sigma_upper=3.0, min_points=1))
    c["window_over_row"] = (t, y, None, dict(window_length=1000.0, break_tolerance=INF, sigma_upper=3.0, sigma_lower=3.0))
    edge = y.copy()
    edge[:, 2] = 1.02                                 # a high point whose window holds 14 other points: no residual at min_points 20
    c["few_members"] = (t, edge, None, dict(window_length=0.5, sigma_upper=3.0, sigma_lower=3.0, min_points=20))
    c["max_run_3"] = (t, y, None, dict(window_length=0.5, sigma_upper=4.0, sigma_lower=3.0, max_run=3, n_iter=4))
    c["max_run_3_flat"] = (t, y, None, dict(sigma_upper=4.0, sigma_lower=3.0, max_run=3, n_iter=4))
    ends = y.copy()
    ends[:, 0] = numpy.nan
    ends[:, -1] = numpy.nan
    c["nan_at_both_ends"] = (t, ends, None, dict(window_length=0.3, sigma_upper=4.0, sigma_lower=4.0))
    # three segments, the middle one missing altogether (row 0) and in part (row 1)
    t3 = numpy.concatenate([series(60), 5.0 + series(20), 10.0 + series(60)])
    y3 = dirty_rows(140, 2, seed=3)
    y3[0, 60:80] = numpy.nan
    y3[1, 60:70] = -1.0
    c["segment_missing"] = (t3, y3, None, dict(sigma_upper=4.0))
    c["segment_missing_slide"] = (t3, y3, None, dict(window_length=0.4, sigma_upper=4.0, sigma_lower=4.0))
    gone = numpy.full((2, 64), numpy.nan)
    gone[1] = dirty_rows(64, 1, seed=5)[0]
    c["row_missing"] = (series(64), gone, None, dict(sigma_upper=3.0))
    c["row_missing_slide"] = (series(64), gone, None, dict(window_length=0.5, sigma_upper=3.0))
    c["constant"] = (series(50), numpy.full((1, 50), 0.75), None, dict(sigma_upper=3.0, sigma_lower=3.0))
    const = numpy.full((1, 50), 0.75)
    const[0, 7] = numpy.nan
    c["constant_slide"] = (series(50), const, None, dict(window_length=0.3, sigma_upper=3.0, sigma_lower=3.0))
    # ties: values on a grid of 1e-4, even and odd member counts (67 and 68 points a row, windows of 9 and 10 and their edges)
    rng = numpy.random.default_rng(21)
    for n in (67, 68):
        yq = numpy.round(1.0 + 3e-4 * rng.standard_normal((2, n)), 4)
        yq[0, 10] = 1.01
        yq[1, 30] = numpy.nan
        c["ties_n%d" % n] = (series(n), yq, None, dict(sigma_upper=3.0, sigma_lower=3.0))
        c["ties_slide_n%d" % n] = (series(n), yq, None, dict(window_length=9.5 / 48.0, sigma_upper=3.0, sigma_lower=3.0))
    # duplicated time stamps around flagged points
    td = numpy.repeat(series(20), 2)
    yd = 1.0 + 1e-3 * numpy.arange(40, dtype=numpy.float64)[None, :]
    yd = numpy.vstack([yd, yd])
    yd[0, [4, 5, 11, 20, 39]] = numpy.nan
    yd[1, [0, 1, 2, 7, 8, 9, 10]] = numpy.nan
    c["duplicate_stamps"] = (td, yd, None, dict(sigma_upper=INF, sigma_lower=INF))
    # runs of low candidates: one that ends at a segment boundary, one bridged by a missing point, one longer than max_run
    tr = series(120, gap_at=60)
    base = 1.0 + 1e-4 * numpy.sin(numpy.arange(120.0))
    yr = numpy.vstack([base, base, base])
    yr[0, 58:60] -= 0.01                              # two candidates up to the boundary, one right behind it: runs 2 and 1
    yr[0, 60] -= 0.01
    yr[1, 30] -= 0.01                                 # candidate, missing, candidate: one run of 2
    yr[1, 31] = numpy.nan
    yr[1, 32] -= 0.01
    yr[1, 90] -= 0.01                                 # alone
    yr[2, 20:24] -= 0.01                              # a run of 4
    yr[2, 24] += 0.05                                 # a high point ends it
    yr[2, 25:27] -= 0.01                              # a run of 2
    for run in (1, 2, 3):
        c["runs_max%d" % run] = (tr, yr, None, dict(sigma_upper=5.0, sigma_lower=5.0, max_run=run))
        c["runs_slide_max%d" % run] = (tr, yr, None, dict(window_length=0.5, sigma_upper=5.0, sigma_lower=5.0, max_run=run))
    # a point a round
    for it in (0, 1, 16):
        c["one_a_round_%d" % it] = (series(40), one_a_round()[None, :], None,
                                    dict(sigma_upper=ONE_A_ROUND_SIGMA, n_iter=it))
    # the guard: a round that would leave one valid point is not applied
    c["guard"] = (series(3), numpy.array([[1.0, 2.0, 100.0], [1.0, 2.0, 2.5]]), None, dict(sigma_upper=0.5, sigma_lower=0.5))
    c["guard_after_bad"] = (series(5), numpy.array([[1.0, 2.0, 100.0, 3.0, numpy.nan]]), numpy.array([[0, 0, 0, 1, 0]], dtype=numpy.uint8),
                            dict(sigma_upper=0.5, sigma_lower=0.5))
    # the caller's flags
    t = series(257, gap_at=100)
    y = dirty_rows(257, 3, seed=8)
    bad = (numpy.random.default_rng(9).random((3, 257)) < 0.05).astype(numpy.uint8)
    c["bad"] = (t, y, bad, dict(sigma_upper=4.0, sigma_lower=5.0))
    c["bad_slide"] = (t, y, bad.astype(bool), dict(window_length=0.5, sigma_upper=4.0, sigma_lower=5.0))
    c["no_clip"] = (t, y, bad, dict(sigma_upper=INF, sigma_lower=INF))
    c["n_iter_0"] = (t, y, None, dict(window_length=0.5, n_iter=0))
    return c


CASES = _cases()
# the cases a plain-Python run of which takes long are left to the numpy form
PLAIN = sorted(k for k, v in CASES.items() if v[1].shape[1] <= 300)

_expected = {}


def expected(name):
    """(rows, flags, record) of clean_spec.clean for the case, formed once."""
    if name not in _expected:
        t, y, bad, kw = CASES[name]
        _expected[name] = clean_spec.clean(t, y, bad, **kw)
    return _expected[name]


def same(a, b):
    """Bit for bit: equal bytes (NaN equals the same NaN)."""
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the measured curves: the project's usual one (spline_cases.rotator: 90 d at 48 points a day with a 3-day gap, noise 3e-4,
# a 0.5 % box of 0.2 d every 7 d, a star of 1 % at 3.1 d) with twelve flares of 1 % decaying over six samples, 2 % of the points
# NaN and five single samples lowered by 3e-3; flares and low samples keep clear of the transits, as the usual curve's flares do
NOISE = 3e-4


def survey_curve(seed, rotator=False):
    """A dict: t, y (the star divided out unless rotator), in_transit, flare (the six samples of every flare), nan, low (the
    five samples)."""
    import spline_cases
    base = spline_cases.rotator(seed)
    t, in_transit = base["t"], base["in_transit"]
    n = len(t)
    star = 1.0 + 0.01 * numpy.sin(2.0 * numpy.pi * t / 3.1) + 0.004 * numpy.sin(2.0 * numpy.pi * t / 5.7)
    y = base["flux"] / star
    rng = numpy.random.default_rng(1000 + seed)
    near = numpy.abs((t - 2.3 + 0.5 * spline_cases.PERIOD) % spline_cases.PERIOD - 0.5 * spline_cases.PERIOD) <= 0.6
    flare = numpy.zeros(n, dtype=bool)
    for a in rng.choice(numpy.flatnonzero(~near[:n - 6]), size=12, replace=False):
        y[a:a + 6] += 0.01 * numpy.exp(-numpy.arange(6) / 2.0)
        flare[a:a + 6] = True
    low = numpy.zeros(n, dtype=bool)
    low[rng.choice(numpy.flatnonzero(~near & ~(numpy.convolve(flare.astype(float), numpy.ones(5), mode="same") > 0)), size=5,
                   replace=False)] = True
    y[low] -= 3e-3
    nan = numpy.zeros(n, dtype=bool)
    nan[rng.choice(numpy.flatnonzero(~low), size=int(0.02 * n), replace=False)] = True
    if rotator:
        y = y * star
    y[nan] = numpy.nan
    return dict(t=t, y=y, in_transit=in_transit, flare=flare, nan=nan, low=low)
