"""Transit-protected detrending on the device (tls_transit_mask, tls_biweight_detrend_masked, tls_prewhiten_masked and the
survey calls on them) against tests/transit_protect_spec.py: the mask and the masked biweight (trend, flat, status) bit for
bit; masked pre-whitening step by step as tests/test_prewhiten.py compares the unmasked call, every check local to one
(iteration, harmonic) on the device's own row; the survey calls with detrend_mask= byte for byte against the calls on rows
detrended beforehand; power_batch_protected against its two passes; and the three entries behind poisoned LDS and smeared
buffers."""
import warnings

import numpy
import pytest

import biweight_spec
import gls_spec
import prewhiten_cases
import prewhiten_spec
import transit_protect_spec as spec
from test_biweight import CADENCE, _k2_batch, _rows, _same_summary, _times
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
PHASE_TOL = 4 * 2.0 ** -53


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def same(a, b, what):
    assert numpy.array_equal(_bits(a), _bits(b)), what


# ---- the mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 257, 700])
@pytest.mark.parametrize("stamps", ["days", "julian"])
def test_transit_mask_bit_equal(gpu, n, stamps):
    rng = numpy.random.default_rng(n)
    t = (2457000.25 if stamps == "julian" else 3.0) + numpy.cumsum(rng.uniform(0.2, 1.8, n)) / 48.0
    span = max(t[-1] - t[0], 1.0)
    # curves 0 .. 6 in unsorted order: 3 candidates (curve 4), 1 (curves 0, 2, 3, 5, 6), none (curve 1)
    curve = numpy.array([4, 0, 6, 4, 2, 5, 3, 4, 2, 5])
    period = numpy.array([span / 3.7, span / 5.1, numpy.nan, span / 2.3, 0.25, span / 4.4, span / 6.0, span / 9.9, numpy.inf, -1.0])
    T0 = t[0] + numpy.array([0.1, 0.3, 0.2, 0.05, 0.0, 0.4, 0.2 - 1e4 * (span / 6.0), 0.6, 0.1, 0.2])
    duration = numpy.array([0.11, 0.2, 0.1, 0.07, 0.25, 0.0, 0.15, 0.09, 0.1, 0.1])
    for factor in (1.5, 0.75):
        got = gpu.transit_mask(t, period, T0, duration, curve, 7, factor)
        want = spec.transit_mask(t, period, T0, duration, curve, 7, factor)
        assert got.dtype == numpy.uint8 and got.shape == (7, n) and numpy.array_equal(got, want), (n, factor)
    want = spec.transit_mask(t, period, T0, duration, curve, 7, 1.5)
    assert not want[1].any() and not want[6].any() and not want[5].any()     # none; a non-finite period; a zero duration
    assert want[2].all()                                                      # factor * duration >= period: everything
    if n >= 257:
        assert 0 < want[4].sum() < n and 0 < want[3].sum() < n               # (curve 3: T0 1e4 periods before the series)
    same_mask = survey.transit_mask(t, period, T0, duration, curve, 7, context=gpu)
    assert numpy.array_equal(same_mask, want)
    assert gpu.transit_mask(t, period[:3], T0[:3], duration[:3]).shape == (3, n)                    # curve None: k -> curve k
    assert gpu.transit_mask(t, [], [], [], n_curves=2).tobytes() == bytes(2 * n)
    assert gpu.transit_mask(t, [], [], []).shape == (0, n)


def test_transit_mask_argument_errors_of_the_c_entry(gpu):
    lib = _lib.load()
    t = 1000.0 + numpy.arange(40) / 48.0
    p, T0, d = numpy.array([3.0, 2.0]), numpy.array([1000.1, 1000.2]), numpy.array([0.1, 0.1])
    out = numpy.zeros((2, 40), dtype=numpy.uint8)
    dp, ip, u8 = _lib._dp, _lib._ip, out.ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_uint8))

    def c_call(tt=t, n=40, curve=None, m=2, factor=1.5, n_curves=2):
        return lib.tls_transit_mask(gpu._h, dp(tt), n, None if curve is None else ip(curve), dp(p), dp(T0), dp(d), m, factor,
                                    n_curves, u8)

    assert c_call() == 0
    for kw in (dict(n=0), dict(m=-1), dict(n_curves=-1), dict(factor=0.0), dict(factor=numpy.inf), dict(factor=numpy.nan),
               dict(n_curves=1), dict(curve=numpy.array([0, 2])), dict(curve=numpy.array([-1, 0])),
               dict(tt=numpy.where(numpy.arange(40) == 3, numpy.nan, t))):
        assert c_call(**kw) == -1, kw
    assert c_call(n_curves=0, m=0) == 0


# ---- the masked biweight ----------------------------------------------------------------------------------------------------------
def _tile(lo, hi):
    """The outputs a workgroup takes (tls_amd.hip biweight_plan): the whole row up to P0 = about 4 (wmax - 1) slots, at least
    256, otherwise P0 - 2 (wmax - 1)."""
    n, wmax = len(lo), int((hi - lo).max())
    p0 = 64
    while p0 < max(4 * (wmax - 1), 256):
        p0 *= 2
    p0 = min(p0, 8192)
    return n if n <= p0 else p0 - 2 * (wmax - 1)


def _masks(n, t, lo, hi, rng):
    """The masks of the module's docstring, one a row: empty, full, a whole segment (the middle third, which the "gaps" stamps
    make one), runs longer than the longest window in the middle, at the first and at the last point, a run across the first
    tile boundary, random 30 %."""
    run = min(n, int((hi - lo).max()) + 3)
    tile = _tile(lo, hi)
    masks = numpy.zeros((8, n), dtype=numpy.uint8)
    masks[1] = 1
    masks[2, 2 * n // 3: max(5 * n // 6, 2 * n // 3 + 1)] = 1
    masks[3, max(0, n // 2 - run // 2): n // 2 + run // 2 + 1] = 1
    masks[4, :run] = 1
    masks[5, n - run:] = 1
    edge = tile if tile < n else n // 2
    masks[6, max(0, edge - 5): edge + 5] = 3                  # (any byte other than 0 protects)
    masks[7] = rng.random(n) < 0.3
    return masks


def _check_biweight(ctx, t, rows, masks, window_length, min_points, break_tolerance=0.5):
    flat, trend, status = ctx.biweight_detrend_masked(t, rows, masks, window_length, break_tolerance, min_points,
                                                      return_trend=True, return_status=True)
    want = spec.biweight_masked(t, rows, masks, window_length, break_tolerance, min_points)
    what = (rows.shape, window_length, min_points)
    assert status.dtype == numpy.uint8 and numpy.array_equal(status, want[2]), what
    same(trend, want[1], what)
    same(flat, want[0], what)
    same(ctx.biweight_detrend_masked(t, rows, masks, window_length, break_tolerance, min_points), flat, what)   # (no trend, no status)
    assert numpy.all(numpy.isfinite(flat)) and numpy.all(flat > 0)
    return flat, trend, status


@pytest.mark.parametrize("n", [1, 2, 3, 7, 256, 700])
@pytest.mark.parametrize("kind", ["regular", "irregular", "duplicates", "gaps"])
def test_masked_biweight_bit_equal(gpu, n, kind):
    rng = numpy.random.default_rng(1000 + n)
    t = _times(n, kind, rng)
    kinds = _rows(n, rng)
    span = t[-1] - t[0]
    for wl in (0.3 * CADENCE, 0.5, 4.0 * span + 1.0):         # below one cadence, typical, longer than the series
        lo, hi = biweight_spec.windows(t, wl, 0.5)
        masks = _masks(n, t, lo, hi, rng)
        if n == 700 and wl > span:                            # (700-point windows: half the masks keep the statement quick)
            masks = masks[[0, 1, 3, 7]]
        rows = kinds[numpy.arange(len(masks)) % len(kinds)]
        for min_points in (1, 3):
            flat, trend, status = _check_biweight(gpu, t, rows, masks, wl, min_points)
            # the empty mask: the unmasked call's bits on the device; the full one: the same values with status 2
            plain = gpu.biweight_detrend(t, rows[:2], wl, 0.5, return_trend=True)
            same(flat[:2], plain[0], (n, kind, wl))
            same(trend[:2], plain[1], (n, kind, wl))
            assert not status[0].any() and numpy.all(status[1] == 2)
    one = gpu.biweight_detrend_masked(t, kinds[0], masks[-1], 0.5, 0.5, return_status=True)   # one row as [n]
    assert one[0].shape == one[1].shape == (n,)
    same(one[0], spec.biweight_masked(t, kinds[0], masks[-1], 0.5, 0.5)[0], (n, kind, "one row"))


def test_masked_biweight_window_at_the_cap(gpu):
    """Windows of BIWEIGHT_MAX_WINDOW points (the largest span: the LDS is full, the mask lives in spare bits) with every other
    point protected: every window keeps half its points, so every point is fitted; a sample of them against the statement's
    location of the members, the first and the last point among them."""
    n = _lib.BIWEIGHT_MAX_WINDOW + 25
    rng = numpy.random.default_rng(4095)
    t = 1000.0 + CADENCE * numpy.arange(n)
    y = _rows(n, rng)[0]
    wl = (_lib.BIWEIGHT_MAX_WINDOW - 1) * CADENCE
    lo, hi = biweight_spec.windows(t, wl, 0.5)
    assert (hi - lo).max() == _lib.BIWEIGHT_MAX_WINDOW
    mask = (numpy.arange(n) % 2).astype(numpy.uint8)
    flat, trend, status = gpu.biweight_detrend_masked(t, y, mask, wl, 0.5, 3, return_trend=True, return_status=True)
    assert not status.any()
    same(flat, y / trend, "flat")
    sample = numpy.unique(numpy.concatenate([[0, 1, n // 2, n - 2, n - 1], rng.integers(0, n, 27)]))
    for i in sample:
        members = y[lo[i]:hi[i]][mask[lo[i]:hi[i]] == 0]
        same(trend[i], biweight_spec.location(members), i)


@pytest.mark.parametrize("n_rows", [1, 33])
def test_masked_biweight_row_counts(gpu, n_rows):
    """A different mask a row, from nearly empty to nearly full."""
    rng = numpy.random.default_rng(n_rows)
    t = _times(300, "irregular", rng)
    rows = (1.0 + 0.01 * numpy.sin(t[None, :] / rng.uniform(0.5, 3.0, (n_rows, 1)))) * (1.0 + 1e-4 * rng.standard_normal((n_rows, 300)))
    masks = (rng.random((n_rows, 300)) < numpy.linspace(0.05, 0.97, n_rows)[:, None]).astype(numpy.uint8)
    _, _, status = _check_biweight(gpu, t, rows, masks, 0.5, 3)
    if n_rows == 33:
        assert {0, 1} <= set(numpy.unique(status))


def test_masked_biweight_argument_errors_of_the_c_entry(gpu):
    lib = _lib.load()
    t = 1000.0 + CADENCE * numpy.arange(40)
    y, mask = numpy.ones((2, 40)), numpy.zeros((2, 40), dtype=numpy.uint8)
    out = numpy.empty_like(y)
    dp, u8 = _lib._dp, _lib.ctypes.POINTER(_lib.ctypes.c_uint8)

    def c_call(wl=0.5, bt=0.5, low=3, n=40, rows=2, mk=mask):
        return lib.tls_biweight_detrend_masked(gpu._h, dp(t), dp(y), None if mk is None else mk.ctypes.data_as(u8), n, rows, wl,
                                               bt, low, dp(out), None, None)

    assert c_call() == 0
    for kw in (dict(low=0), dict(low=-3), dict(wl=0.0), dict(wl=numpy.nan), dict(bt=0.0), dict(n=0), dict(rows=-1), dict(mk=None)):
        assert c_call(**kw) == -1, kw
    assert c_call(rows=0) == 0 and c_call(low=1) == 0
    with pytest.raises(ValueError, match="min_points"):
        gpu.biweight_detrend_masked(t, y, mask, 0.5, 0.5, 0)
    with pytest.raises(ValueError, match="mask"):
        gpu.biweight_detrend_masked(t, y, mask[:1], 0.5, 0.5)


# ---- masked pre-whitening -------------------------------------------------------------------------------------------------------
def _prewhiten_masks(case):
    """One mask a curve: empty; one run; fewer than 3 points left."""
    n = case.y.shape[1]
    masks = numpy.zeros(case.y.shape, dtype=numpy.uint8)
    masks[1, n // 3: n // 3 + n // 10] = 1
    masks[2] = 1
    masks[2, [n // 4, n // 2]] = 0
    return masks


def _check_prewhiten_curve(case, c, mask, flat, trend, info):
    """Curve c against the statement, step by step on the device's own rows (tests/test_prewhiten.py check_curve with the
    masked weights)."""
    t, f, K, H = case.t, case.f, case.n_terms, case.harmonics
    y = case.y[c]
    n = len(y)
    dy = None if case.dy is None else case.dy[c]
    prot = mask != 0
    want = spec.prewhiten_masked(t, y, f, mask, dy, K, H, case.min_power)
    assert all(g >= prewhiten_cases.MIN_GAP for g in want["gaps"]), (c, want["gaps"])       # (the premise of comparing the pick)
    steps, terms, sums = info["steps"][:, c], info["terms"][c], info["sums"][c]
    ran = int(info["n_iterations"][c])
    what = "curve %d" % c
    assert ran == want["n_iterations"] and info["status"][c] == want["status"], what
    same(steps[0], y, what)
    fitted = int((~prot).sum()) >= 3
    v = spec.inverse_variances(n, dy, prot if fitted else numpy.zeros(n, dtype=bool))
    mean0 = spec.index_prologue(y, v)[2]
    total, slack = numpy.zeros(n), numpy.zeros(n)
    for j in range(K):
        if j >= ran:
            assert numpy.all(terms[j]["status"] == 2.0) and numpy.isnan(terms[j]["frequency"]).all() and numpy.isnan(sums[j]).all()
            continue
        head = terms[j][0]
        w, a, _, YY = spec.index_prologue(steps[j * H], v)
        cs, cs2, ya = (prewhiten_spec._fast_sums(t, w, f), prewhiten_spec._fast_sums(t, w, 2.0 * f), prewhiten_spec._fast_sums(t, a, f))
        power = gls_spec.epilogue(ya[:, 0], ya[:, 1], cs[:, 0], cs[:, 1], cs2[:, 0], cs2[:, 1], YY)[0]
        k = prewhiten_spec.pick(power)
        assert int(head["index"]) == k == int(want["terms"][j][0]["index"]), (what, j)
        fstar = prewhiten_spec.refine(f, k, head["power_left"], head["power_peak"], head["power_right"])
        for h in range(H):
            term, row = terms[j][h], steps[j * H + h]
            tag = (what, j, h)
            fh = numpy.float64(h + 1) * fstar
            same(term["frequency"], fh, tag + ("f*",))
            lw, la, mean, lYY = spec.lane_prologue(row, v)
            assert numpy.all(lw[prot] == 0.0) and numpy.all(la[prot] == 0.0)
            same(term["mean"], mean, tag + ("mean",))
            same(term["variance"], lYY, tag + ("variance",))
            exact = prewhiten_spec.exact_six_sums(t, lw, la, fh)
            reach = numpy.array([fh, 2.0 * fh])
            bound = numpy.repeat([gls_spec.sum_bound(t, la, reach)[0], gls_spec.sum_bound(t, lw, reach)[0]], [2, 4])
            assert numpy.all(numpy.abs(sums[j][h] - exact) <= bound), tag + ("sums", numpy.abs(sums[j][h] - exact) / bound)
            p, amplitude, phase, ca, sa = prewhiten_spec.fit_epilogue(sums[j][h], lYY)
            for name, value in (("power", p), ("amplitude", amplitude), ("ca", ca), ("sa", sa), ("C", sums[j][h][2]), ("S", sums[j][h][3])):
                same(term[name], value, tag + (name,))
            assert term["status"] == 0.0 and abs(term["phase"] - phase) <= PHASE_TOL, tag
            after, q = prewhiten_spec.subtraction(t, row, fh, term["ca"], term["sa"], term["C"], term["S"])
            bound = prewhiten_spec.subtract_bound(row, after, term["ca"], term["sa"])
            off = numpy.abs(steps[j * H + h + 1] - after)
            assert numpy.all(off <= bound), tag + ("subtraction", float(numpy.max(off / bound)))
            if prot.any():                                   # the subtraction reaches the protected points
                assert numpy.any(steps[j * H + h + 1][prot] != row[prot]), tag
            slack = slack + 8.0 * EPS * (abs(term["ca"]) + abs(term["sa"])) + numpy.spacing(numpy.maximum(numpy.abs(total), numpy.abs(total + q)))
            total = total + q
    same(flat[c], y / trend[c], what + " flat")
    if ran == 0:
        same(trend[c], numpy.full(n, mean0), what + " trend")
    else:
        off = numpy.abs(trend[c] - (mean0 + total))
        assert numpy.all(off <= slack + numpy.spacing(numpy.maximum(numpy.abs(trend[c]), numpy.abs(mean0 + total)))), (what, "trend")
        if prot.any():                                       # the trend is defined and differs from the mean at protected points
            assert numpy.all(numpy.isfinite(trend[c][prot])) and numpy.any(trend[c][prot] != mean0), what
    return ran


@pytest.mark.parametrize("n", [300, 1367])
@pytest.mark.parametrize("with_dy", [False, True])
def test_masked_prewhitening_every_step_against_the_statement(gpu, n, with_dy):
    F = 333
    assert F % _lib.GLS_FREQ_TILE
    case = prewhiten_cases.batch(n, 3, F, 70 + n, with_dy, 2, 1)
    masks = _prewhiten_masks(case)
    flat, trend, info = gpu.prewhiten_masked(case.t, case.y, masks, case.f, 2, 1, 0.0, dy=case.dy, return_trend=True, debug=True)
    ran = [_check_prewhiten_curve(case, c, masks[c], flat, trend, info) for c in range(3)]
    assert ran == [2, 2, 0] and list(info["status"]) == [0.0, 0.0, 2.0]
    # the plain call and the survey call return the same rows
    same(gpu.prewhiten_masked(case.t, case.y, masks, case.f, 2, 1, 0.0, dy=case.dy), flat, n)
    got = survey.prewhiten_batch(case.t, case.y, 2, 1, 0.0, frequencies=case.f, dy_batch=case.dy, return_trend=True,
                                 return_terms=True, context=gpu, mask=masks)
    same(got[0], flat, n)
    same(got[1], trend, n)
    assert got[2]["terms"].tobytes() == info["terms"].tobytes()
    # the empty mask: the unmasked call's weights bit for bit, so its picks; the sums of the weights come from another product
    # launch, which may move the last bits of f* and so the trend by far less than the 1e-9 asked here (a sanity check)
    plain = gpu.prewhiten(case.t, case.y[:1], case.f, 2, 1, 0.0, dy=None if case.dy is None else case.dy[:1], return_trend=True,
                          return_terms=True)
    assert numpy.array_equal(plain[2]["terms"]["index"], info["terms"]["index"][:1])
    assert numpy.max(numpy.abs(plain[1][0] - trend[0])) <= 1e-9


# ---- composition ---------------------------------------------------------------------------------------------------------------
def _k2_mask(t, n_curves):
    """A mask a curve: transits of a different ephemeris each, the last curve none."""
    k = numpy.arange(n_curves - 1)
    return survey_mask_spec(t, 3.0 + 0.7 * k, t[0] + 0.3 * (k + 1), 0.15 + 0.02 * k, n_curves)


def survey_mask_spec(t, period, T0, duration, n_curves):
    return spec.transit_mask(t, period, T0, duration, numpy.arange(len(period)), n_curves, 1.5)


def _same_results(got, want):
    _same_summary(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()


def test_detrend_mask_equals_rows_detrended_beforehand(gpu):
    t, raw, kw = _k2_batch(5)
    mask = _k2_mask(t, 5)
    assert mask[:4].any(axis=1).all() and not mask[4].any()
    bw = survey.Biweight(0.5)
    steps = (survey.Prewhiten(2), survey.Biweight(0.5))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flat = survey.biweight_batch(t, raw, 0.5, mask=mask, context=gpu)
        got = survey.power_batch(t, raw, detrend=bw, detrend_mask=mask, with_arrays=True, context=gpu, **kw)
        _same_results(got, survey.power_batch(t, flat, with_arrays=True, context=gpu, **kw))
        assert survey.power_batch(t, raw, detrend=bw, context=gpu, **kw)[0]["SDE"].tobytes() != got[0]["SDE"].tobytes()
        dealt = survey.power_batch(t, raw, detrend=bw, detrend_mask=mask, with_arrays=True, devices=[0, 0], **kw)
        _same_results(dealt, survey.power_batch(t, flat, with_arrays=True, devices=[0, 0], **kw))
        # two steps: the mask goes to both
        grid, k, h, low = survey._prewhiten_step(t, steps[0], len(t))
        first = survey.prewhiten_batch(t, raw, k, h, low, frequencies=grid, mask=mask, context=gpu)
        both = survey.biweight_batch(t, first, 0.5, mask=mask, context=gpu)
        got = survey.power_batch(t, raw, detrend=steps, detrend_mask=mask, context=gpu, **kw)
        _same_results(got, survey.power_batch(t, both, context=gpu, **kw))
        _same_results(survey.power_batch(t, raw, detrend=steps, detrend_mask=mask, devices=[0, 0], **kw),
                      survey.power_batch(t, both, devices=[0, 0], **kw))
        # the other calls that take detrend_mask
        got = survey.search_batch(t, raw, detrend=bw, detrend_mask=mask, context=gpu, **kw)
        for a, b in zip(got, survey.search_batch(t, flat, context=gpu, **kw)):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        got = survey.lomb_scargle(t, raw[:2], detrend=bw, detrend_mask=mask[:2], context=gpu)
        want = survey.lomb_scargle(t, flat[:2], context=gpu)
        assert all(numpy.asarray(got[key]).tobytes() == numpy.asarray(want[key]).tobytes() for key in want)


def test_power_batch_protected_is_its_two_passes(gpu):
    t, raw, kw = _k2_batch(5)
    bw = survey.Biweight(0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = survey.power_batch(t, raw, detrend=bw, peaks=2, peak_fits=True, context=gpu, **kw)
        summary, peaks = first[0], first[-1]["peaks"]
        sde_min = float(numpy.sort(summary["SDE"])[2])                       # (three of the five curves reach it)
        protected = summary["SDE"] >= sde_min
        assert protected.sum() == 3
        use = protected[:, None] & (peaks["status"] == 0)
        assert use.sum() >= 4                                                 # (more than one peak a curve goes into the mask)
        curve = numpy.broadcast_to(numpy.arange(5)[:, None], use.shape)[use]
        mask = survey.transit_mask(t, peaks["period"][use], peaks["T0"][use], peaks["duration_days"][use], curve=curve, n_curves=5,
                                   context=gpu)
        assert mask[protected].any(axis=1).all() and not mask[~protected].any()
        want = survey.power_batch(t, raw, detrend=bw, detrend_mask=mask, statistics=True, context=gpu, **kw)
        got, info = survey.power_batch_protected(t, raw, bw, sde_min, n_peaks=2, statistics=True, context=gpu, **kw)
        _same_results(got, want)
        assert numpy.array_equal(info["protected"], protected) and numpy.array_equal(info["mask"], mask)
        _same_summary(info["summary"], summary)
        # nothing reaches sde_min = inf: plain power_batch(detrend=...), byte for byte
        got, info = survey.power_batch_protected(t, raw, bw, numpy.inf, context=gpu, **kw)
        _same_results(got, survey.power_batch(t, raw, detrend=bw, context=gpu, **kw))
        assert not info["protected"].any() and not info["mask"].any()
        # dealt out over devices: the two passes dealt out the same way
        first = survey.power_batch(t, raw, detrend=bw, peaks=2, peak_fits=True, devices=[0, 0], **kw)
        peaks = first[-1]["peaks"]
        use = (first[0]["SDE"] >= sde_min)[:, None] & (peaks["status"] == 0)
        curve = numpy.broadcast_to(numpy.arange(5)[:, None], use.shape)[use]
        mask = survey.transit_mask(t, peaks["period"][use], peaks["T0"][use], peaks["duration_days"][use], curve=curve, n_curves=5,
                                   context=gpu)
        got, info = survey.power_batch_protected(t, raw, bw, sde_min, n_peaks=2, statistics=True, devices=[0, 0], **kw)
        _same_results(got, survey.power_batch(t, raw, detrend=bw, detrend_mask=mask, statistics=True, devices=[0, 0], **kw))
        assert numpy.array_equal(info["mask"], mask) and numpy.array_equal(info["protected"], first[0]["SDE"] >= sde_min)


# ---- poison ------------------------------------------------------------------------------------------------------------------
def test_poisoned_lds_and_reused_buffers(gpu):
    """The three entries before and after tls_debug_poison_lds (every CU's LDS and the context's device buffers smeared) agree
    byte for byte; a small call behind a larger one reuses the buffers and agrees."""
    rng = numpy.random.default_rng(9)
    n = 700
    t = _times(n, "gaps", rng)
    rows = _rows(n, rng)[[0, 1, 5]]
    lo, hi = biweight_spec.windows(t, 0.5, 0.5)
    masks = _masks(n, t, lo, hi, rng)[[7, 3, 2]]
    case = prewhiten_cases.batch(300, 3, 77, 5, True, 2, 1)
    pmasks = _prewhiten_masks(case)
    cand = (numpy.array([3.1, 2.2, 4.5]), t[0] + numpy.array([0.2, 0.4, 0.1]), numpy.array([0.2, 0.1, 0.3]), numpy.array([1, 0, 1]))

    def calls(small):
        k, m = (1, n // 3) if small else (3, n)
        tt = t[:m]
        out = [gpu.transit_mask(tt, cand[0][:k], cand[1][:k], cand[2][:k], cand[3][:k], 2)]
        out += list(gpu.biweight_detrend_masked(tt, rows[:k, :m], masks[:k, :m], 0.5, 0.5, 3, return_trend=True, return_status=True))
        flat, trend, info = gpu.prewhiten_masked(case.t, case.y[:k], pmasks[:k], case.f, 2, 1, 0.0,
                                                 dy=case.dy[:k], return_trend=True, return_terms=True)
        return out + [flat, trend, info["terms"], info["status"]]

    small = calls(True)
    large = calls(False)
    behind = calls(True)
    gpu.poison_lds(0xFFFFFFFF)
    again = calls(True)
    gpu.poison_lds(0x7FF00000)
    large_again = calls(False)
    for a, b in zip(small + small + large, behind + again + large_again):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    m = n // 3
    want = spec.biweight_masked(t[:m], rows[:1, :m], masks[:1, :m], 0.5, 0.5, 3)
    same(again[1], want[0], "flat")
    assert numpy.array_equal(again[3], want[2]) and numpy.array_equal(again[0], spec.transit_mask(t[:m], *[c[:1] for c in cand], 2))
