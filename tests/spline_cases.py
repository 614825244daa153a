"""The inputs test_spline_host.py and test_spline.py share: the rotating star of DESIGN.md "Spline detrending" and the small
shapes at which tls_spline_detrend's kernels can go wrong.  GPU-free."""
import numpy

import spline_spec as spec

CADENCE = 1.0 / 48.0
NOISE = 3e-4
DEPTH, DURATION, PERIOD = 0.005, 0.2, 7.0
LADDER = (0.3, 0.5, 0.75, 1.0, 1.5, 2.5)


def rotator(seed, flares=0):
    """90 d at 48 points a day with a 3-day gap; a star with 1 % at 3.1 d plus 0.4 % at 5.7 d; a 0.5 % box of 0.2 d every 7 d;
    white noise of 3e-4; `flares` exponential flares of 1 % (decay 0.04 d) outside the transits.  The seed draws the noise
    and the flares' times; the star and the transits are the same for every seed.  A dict."""
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(4320) * CADENCE
    t = t[(t < 40.0) | (t >= 43.0)]
    star = 1.0 + 0.01 * numpy.sin(2.0 * numpy.pi * t / 3.1) + 0.004 * numpy.sin(2.0 * numpy.pi * t / 5.7)
    T0 = 2.3
    in_transit = numpy.abs((t - T0 + 0.5 * PERIOD) % PERIOD - 0.5 * PERIOD) <= 0.5 * DURATION
    box = numpy.where(in_transit, 1.0 - DEPTH, 1.0)
    noise = NOISE * rng.standard_normal(len(t))
    flare, peaks = numpy.zeros(len(t)), numpy.zeros(0, dtype=numpy.int64)
    if flares:
        near = numpy.abs((t - T0 + 0.5 * PERIOD) % PERIOD - 0.5 * PERIOD) <= 0.6
        peaks = numpy.sort(rng.choice(numpy.flatnonzero(~near), flares, replace=False))
        for t_f in t[peaks]:
            flare += numpy.where(t >= t_f, 0.01 * numpy.exp(-numpy.maximum(t - t_f, 0.0) / 0.04), 0.0)
    flared = flare > NOISE
    return {"t": t, "flux": star * (box + noise + flare), "in_transit": in_transit, "flared": flared, "flare_peaks": peaks,
            "mask": in_transit_mask(t, T0, 1.5)}


def in_transit_mask(t, T0, factor):
    return (numpy.abs((t - T0 + 0.5 * PERIOD) % PERIOD - 0.5 * PERIOD) <= 0.5 * factor * DURATION).astype(numpy.uint8)


def rms_and_depth(flat, star):
    """(the rms of the flat row outside the transits and the flares, 1 - the in-transit mean over the mean outside)."""
    out = ~star["in_transit"] & ~star["flared"]
    level = flat[out].mean()
    return float(numpy.sqrt(numpy.mean((flat[out] / level - 1.0) ** 2))), float(1.0 - flat[star["in_transit"]].mean() / level)


def rows(t, n_curves=1, dy=False, seed=0, outliers=True):
    """n_curves rows over t: a slow sinusoid of 1 %, white noise of 1e-3, where there is room a few outliers of 1 %."""
    n = len(t)
    rng = numpy.random.default_rng(1000 * n + 7 * n_curves + seed)
    phase = rng.uniform(0.0, 6.0, (n_curves, 1))
    y = 1.0 + 0.01 * numpy.sin(2.0 * numpy.pi * t[None, :] / 3.1 + phase) + 1e-3 * rng.standard_normal((n_curves, n))
    if outliers and n > 40:
        for r in range(n_curves):
            y[r, rng.choice(n, 3, replace=False)] += 0.01
    return {"t": numpy.asarray(t, dtype=numpy.float64), "y": y, "dy": rng.uniform(5e-4, 2e-3, (n_curves, n)) if dy else None,
            "mask": None}


def grid(n, start=1.0):
    return start + numpy.arange(n) * CADENCE


def _duplicates():
    t = numpy.repeat(grid(60), 2)[:97]
    return rows(t, 2, dy=True)


def _short_gap():
    """A gap of 0.4 d, below break_tolerance: the intervals of 0.1 d inside it hold no point."""
    t = numpy.concatenate([grid(48), grid(48, 2.4)])
    return rows(t, 2)


def _protected_interval():
    case = rows(grid(192), 2, dy=True)
    case["mask"] = numpy.zeros((2, 192), dtype=numpy.uint8)
    case["mask"][0, 60:110] = 1                              # two whole intervals of 0.5 d (24 points each) and more
    case["mask"][1, 5] = 1
    return case


def _lonely_point():
    """A segment of one point between two ordinary ones; a second curve whose first segment is wholly protected."""
    t = numpy.concatenate([grid(50), [4.0], grid(70, 6.0)])
    case = rows(t, 2)
    case["mask"] = numpy.zeros((2, len(t)), dtype=numpy.uint8)
    case["mask"][1, :50] = 1
    return case


def _two_equal_stamps():
    return {"t": numpy.array([2.0, 2.0]), "y": numpy.array([[1.0, 1.01]]), "dy": None, "mask": None}


def _scaled():
    case = rows(grid(257), 3)
    case["y"] = case["y"] * numpy.array([1e-100, 1.0, 1e100])[:, None]
    return case


def _lds(points):
    case = rows(grid(points), 2, dy=True)
    case["mask"] = (numpy.random.default_rng(4).random((2, points)) < 0.05).astype(numpy.uint8)
    return case


def _widest_band():
    """A segment of 1100 points whose spacing gives q = 509: m = MAX_COEF, two chunks of interval owners."""
    return rows(grid(1100), 1)


WIDEST_SPAN = 1099 * CADENCE
WIDEST_SPACING = WIDEST_SPAN / (spec.MAX_COEF - 3 - 0.5)
ONE_MORE_SPACING = WIDEST_SPAN / (spec.MAX_COEF - 3 + 0.5)


def _picks():
    """Five curves over 30 d whose variability runs from none to a period of 1.5 d: the BIC picks differ."""
    t = grid(1440)
    rng = numpy.random.default_rng(21)
    periods = numpy.array([numpy.inf, 12.0, 6.0, 3.0, 1.5])
    y = 1.0 + 0.01 * numpy.sin(2.0 * numpy.pi * t[None, :] / periods[:, None]) + 5e-4 * rng.standard_normal((5, 1440))
    return {"t": t, "y": y, "dy": None, "mask": None}


# name: (the inputs, the keywords of the statement)
CASES = {
    "n1": (lambda: rows(grid(1), 1), {}),
    "n2_dy": (lambda: rows(grid(2), 1, dy=True), {}),
    "n3_fewer_points_than_coefficients": (lambda: rows(grid(3), 2), {}),
    "two_equal_stamps": (_two_equal_stamps, {}),
    "q1": (lambda: rows(grid(40), 1), {"knot_spacing": 1.0}),
    "q2_dy": (lambda: rows(grid(40), 1, dy=True), {"knot_spacing": 0.5}),
    "on_the_knots": (lambda: rows(grid(97), 2), {"knot_spacing": 0.5}),           # span 2.0: h = 0.5, every 24th point on a knot
    "duplicates": (_duplicates, {"knot_spacing": 0.3}),
    "empty_interval": (_short_gap, {"knot_spacing": 0.1}),
    "empty_interval_no_penalty": (_short_gap, {"knot_spacing": 0.1, "penalty": 0.0}),
    "protected_interval": (_protected_interval, {"knot_spacing": 0.5}),
    "lonely_point": (_lonely_point, {}),
    "n255_5_dy": (lambda: rows(grid(255), 5, dy=True), {"knot_spacing": 0.5}),
    "n256": (lambda: rows(grid(256), 1), {"knot_spacing": 0.5}),
    "n257_5": (lambda: rows(grid(257), 5), {"knot_spacing": 0.5, "sigma_upper": 2.0, "sigma_lower": numpy.inf, "n_iter": 16}),
    "crowded_interval": (lambda: rows(grid(600), 2, dy=True), {"knot_spacing": 7.0}),    # 300 members an interval: more than the threads
    "no_clip_round": (lambda: rows(grid(257), 2, dy=True), {"n_iter": 0}),
    "plain_least_squares": (lambda: rows(grid(257), 2), {"n_iter": 0, "sigma_upper": numpy.inf, "sigma_lower": numpy.inf}),
    "clip_stops_at_two": (lambda: rows(grid(3), 4, outliers=False), {"sigma_upper": 0.3, "sigma_lower": 0.3}),
    "scaled_rows": (_scaled, {"knot_spacing": 0.5}),
    "lds_points": (lambda: _lds(spec.LDS_POINTS), {"n_iter": 2}),
    "lds_points_and_one": (lambda: _lds(spec.LDS_POINTS + 1), {"n_iter": 2}),
    "widest_band": (_widest_band, {"knot_spacing": WIDEST_SPACING, "n_iter": 1}),
    "three_spacings": (_picks, {"knot_spacing": [4.0, 1.0, 0.25]}),
    "two_equal_spacings": (_picks, {"knot_spacing": [1.0, 1.0, 4.0]}),
}
_WANT = {}


def statement(case, **kw):
    return spec.fit(case["t"], case["y"], case.get("dy"), case.get("mask"), **kw)


def want(name):
    """The statement of a case, formed once."""
    if name not in _WANT:
        make, kw = CASES[name]
        _WANT[name] = statement(make(), **kw)
    return _WANT[name]


def equal_bits(got, want, names=("flat", "trend", "segment")):
    """Asserts the fields `names` of the two results equal bit for bit (a NaN equals a NaN)."""
    for k in names:
        a, b = numpy.asarray(got[k]), numpy.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        numpy.testing.assert_array_equal(a, b, err_msg=k)
        assert numpy.array_equal(numpy.signbit(a[a == 0.0]), numpy.signbit(b[b == 0.0])), k


# The BIC is K log(N) + Q', both terms >= 0.  The device's log and the host's are each within 1 ulp of the true value (the
# documented accuracy of both libraries' double log), so they differ by at most 2 ulp of log(N), 2 * 2^-52 of the first term; the
# product and the sum round once each, 2^-53 of the value apiece.  Together that is below 3 * 2^-52 of the value: the bound
# asserted is 2^-50 (4 * 2^-52) of the statement's value.
BIC_ULP = 2.0 ** -50


def equal_curves(got, want_curve, S):
    """The curve records: sigma_pp and the flag bit for bit, every finite BIC within BIC_ULP of the statement's, a non-finite
    one the same, NaN behind S; the choice equal wherever the two lowest BIC values are equal or stand apart by more than both
    their bounds.  Returns the number of curves where they do not."""
    got, want_curve = numpy.asarray(got), numpy.asarray(want_curve)
    assert got.shape == want_curve.shape
    numpy.testing.assert_array_equal(got[:, 1:3], want_curve[:, 1:3])
    unclear = 0
    for g, w in zip(got, want_curve):
        assert numpy.all(numpy.isnan(g[3 + S:])) and numpy.all(numpy.isnan(w[3 + S:]))
        a, b = g[3:3 + S], w[3:3 + S]
        finite = numpy.isfinite(b)
        assert numpy.array_equal(numpy.isfinite(a), finite)
        numpy.testing.assert_array_equal(a[~finite], b[~finite])
        bound = BIC_ULP * numpy.abs(b[finite])
        assert numpy.all(numpy.abs(a[finite] - b[finite]) <= bound), (a, b)
        low = numpy.sort(b[finite])
        if len(low) >= 2 and low[1] != low[0] and low[1] - low[0] <= 2.0 * BIC_ULP * abs(low[1]):
            unclear += 1
        else:
            assert g[0] == w[0], (g, w)
    return unclear
