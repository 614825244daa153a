"""Regression detrending without a GPU: the two forms of the statement (tests/decorrelate_spec.py) agree bit for bit, the
statement agrees with numpy.linalg.lstsq within the normal equations' own error growth, it is worth what DESIGN.md
"Decorrelation" says on the K2 roll simulation and on an ensemble with known basis vectors, the host helpers return
hand-written values, and every refusal of the host layer carries its message."""
import numpy
import pytest

import biweight_spec
import decorrelate_cases as cases
import decorrelate_spec as spec
import sysrem_spec
from tls_amd import _lib, survey


def _segmented(n=300):
    case = cases.small(n, 2, 3, n_curves=2, dy=True)
    case["segments"] = [0, 1, 4, 150, n]                     # a single point, fewer points than columns, two ordinary ones
    case["mask"] = numpy.zeros((2, n), dtype=numpy.uint8)
    case["mask"][0, 150:] = 1                                # a whole segment protected
    case["mask"][1, 20:30] = 1
    return case


def _degenerate(n=120):
    case = cases.small(n, 1, 4, n_curves=2)
    case["own"][:, 2] = case["own"][:, 0]                    # a duplicate
    case["own"][:, 3] = 0.0                                  # a constant
    return case


LOOP_CASES = {
    "one_point": lambda: cases.small(1, 1, 0),
    "two_points": lambda: cases.small(2, 0, 1),
    "tile_and_one": lambda: cases.small(257, 2, 3, n_curves=2, dy=True),
    "sixteen_columns": lambda: cases.small(97, 6, 10),
    "segments_and_masks": _segmented,
    "duplicate_and_constant": _degenerate,
}


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
@pytest.mark.parametrize("kw", [{}, {"n_iter": 0}, {"ridge": 1e-6, "sigma_upper": 2.0, "sigma_lower": numpy.inf, "n_iter": 16}],
                         ids=["default", "no_clip", "ridge_one_sided"])
def test_the_loops_equal_the_numpy_form(name, kw):
    case = LOOP_CASES[name]()
    args = (case["y"], case.get("dy"), case.get("mask"), case.get("shared"), case.get("own"), case.get("segments"))
    cases.equal_bits(spec.loops(*args, **kw), spec.fit(*args, **kw))


def test_a_mask_of_zeros_changes_no_bit():
    case = cases.small(257, 2, 3, n_curves=2, dy=True)
    want = cases.statement(case)
    case["mask"] = numpy.zeros(case["y"].shape, dtype=numpy.uint8)
    cases.equal_bits(cases.statement(case), want)


def test_the_statuses_and_the_dropped_bits():
    out = cases.statement(_segmented())
    record = out["record"]
    assert record[:, 0, 0].tolist() == [1.0, 1.0] and record[:, 1, 0].tolist() == [1.0, 1.0]      # 1 and 3 points, 5 columns
    assert record[0, 3, 0] == 1.0 and record[0, 3, 2] == 0.0                                      # the protected segment
    assert record[1, 3, 0] == 0.0 and record[1, 2, 0] == 0.0
    assert numpy.all(out["coef"][record[..., 0] == 1.0] == 0.0) and numpy.all(numpy.isnan(record[..., 6][record[..., 0] == 1.0]))
    # status 1 leaves trend = mu: of the segment's own points, the protected ones where nothing else is there
    y = _segmented()["y"]
    assert out["trend"][0, 0] == y[0, 0] and numpy.all(out["trend"][0, 150:] == record[0, 3, 5])
    case = _degenerate()
    out = cases.statement(case)
    assert numpy.all(out["record"][:, 0, 1] == (1 << 3) + (1 << 4)) and numpy.all(out["record"][:, 0, 7] == 3.0)
    # ... and the other coefficients are those of the fit without the two columns
    case["own"] = case["own"][:, :2]
    kept = cases.statement(case)
    cases.equal_bits({"coef": out["coef"][..., :3], "flat": out["flat"]}, {"coef": kept["coef"], "flat": kept["flat"]}, ("coef", "flat"))


def _against_lstsq(y, X):
    """(the largest coefficient difference between the statement and numpy.linalg.lstsq on sqrt(w) u and sqrt(w) z, the
    bound 64 m cond^2 2^-52 of the largest coefficient, cond): no clip, no ridge, uniform weights, every point in F."""
    out = spec.fit(y[None, :], own=X[None], n_iter=0)
    assert out["record"][0, 0, 0] == 0.0 and out["record"][0, 0, 1] == 0.0
    m = len(X)
    u = (X - out["mean"][0, 0][:, None]) / out["scale"][0, 0][:, None]
    z = y / out["record"][0, 0, 5] - 1.0
    c, _, _, sv = numpy.linalg.lstsq(u.T, z, rcond=None)
    cond = sv[0] / sv[-1]
    return float(numpy.max(numpy.abs(out["coef"][0, 0] - c))), 64.0 * m * cond * cond * 2.0 ** -52 * float(numpy.max(numpy.abs(c))), cond


def test_the_statement_against_lstsq_on_the_roll():
    star = cases.roll_star(0)
    error, bound, cond = _against_lstsq(star["flux"], star["own"])
    print("roll: cond %.3g, error %.3g, bound %.3g" % (cond, error, bound))
    assert cond < 10.0 and error <= bound


def test_the_statement_against_lstsq_at_condition_100():
    rng = numpy.random.default_rng(5)
    n = 2000
    x = rng.standard_normal(n)
    X = numpy.stack([x, x + 0.01 * rng.standard_normal(n)])
    y = 1.0 + 0.01 * X[0] - 0.004 * X[1] + 3e-4 * rng.standard_normal(n)
    error, bound, cond = _against_lstsq(y, X)
    print("two near-equal columns: cond %.3g, error %.3g, bound %.3g" % (cond, error, bound))
    assert 50.0 < cond < 400.0 and error <= bound


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("outliers", [0, 24])
def test_what_the_fit_is_worth_on_the_roll(seed, outliers):
    star = cases.roll_star(seed, outliers=outliers)
    raw_rms, _ = cases.rms_and_depth(star["flux"], star)
    mask = star["in_transit"].astype(numpy.uint8)
    out = spec.fit(star["flux"][None, :], mask=mask[None, :], own=star["own"][None])
    rms, depth = cases.rms_and_depth(out["flat"][0], star)
    print("seed %d, %d outliers: rms %.4g -> %.4g, depth kept %.4f, clipped %d" % (seed, outliers, raw_rms, rms, depth / cases.DEPTH,
                                                                               out["record"][0, 0, 3]))
    assert raw_rms > 3.0 * cases.NOISE
    assert abs(rms / cases.NOISE - 1.0) <= 0.05
    assert 0.98 <= depth / cases.DEPTH <= 1.02
    assert out["record"][0, 0, 3] == outliers
    if outliers == 0:
        # unmasked, the transit's points pull on the fit and are clipped as outliers: the figure DESIGN.md records
        open_ = spec.fit(star["flux"][None, :], own=star["own"][None])
        print("    unmasked: depth kept %.4f" % (cases.rms_and_depth(open_["flat"][0], star)[1] / cases.DEPTH))


def test_beside_it_the_biweight_and_sysrem():
    """What the per-row window and the rank-1 ensemble term do to the same star (DESIGN.md "Decorrelation" records the figures;
    nobody had measured them, so they carry no threshold)."""
    star = cases.roll_star(0)
    flat, _ = biweight_spec.detrend(star["t"], star["flux"], 0.5, 0.5)
    print("biweight 0.5 d: rms %.4g, depth kept %.4f" % tuple(v / s for v, s in zip(cases.rms_and_depth(flat, star), (1.0, cases.DEPTH))))
    # an ensemble on the same roll whose stars each follow the centroids in their own way
    rng = numpy.random.default_rng(3)
    x, y = star["cx"], star["cy"]
    rows = [star["flux"]]
    for _ in range(7):
        a, b, c = 0.01 * rng.uniform(-1.5, 1.5), -0.03 * rng.uniform(0.0, 1.5), 0.004 * rng.uniform(-1.5, 1.5)
        rows.append((1.0 + a * x + b * x * x + c * y) * (1.0 + cases.NOISE * rng.standard_normal(len(x))))
    flat = sysrem_spec.fit(numpy.array(rows), 2)[0][0]
    print("SysRem, 2 components of 8 stars: rms %.4g, depth kept %.4f"
          % tuple(v / s for v, s in zip(cases.rms_and_depth(flat, star), (1.0, cases.DEPTH))))


def test_basis_vectors_bring_every_star_to_its_noise():
    flux, profiles, sigma = cases.ensemble()
    out = spec.fit(flux, shared=profiles)
    rms = numpy.sqrt(numpy.mean((out["flat"] - 1.0) ** 2, axis=1))
    raw = numpy.sqrt(numpy.mean((flux / flux.mean(axis=1, keepdims=True) - 1.0) ** 2, axis=1))
    print("raw / noise %.3g .. %.3g, flat / noise %.4f .. %.4f" % ((raw / sigma).min(), (raw / sigma).max(), (rms / sigma).min(),
                                                                    (rms / sigma).max()))
    assert numpy.all(numpy.abs(rms / sigma - 1.0) <= 0.05)
    assert numpy.median(raw / sigma) > 3.0


# ---- the helpers ------------------------------------------------------------------------------------------------------------
def test_centroid_regressors():
    cx, cy = numpy.array([1.0, 2.0, 4.0]), numpy.array([0.0, 3.0, 1.0])      # medians 2 and 1: x = -1 0 2, y = -1 2 0
    x, y = numpy.array([-1.0, 0.0, 2.0]), numpy.array([-1.0, 2.0, 0.0])
    got = survey.centroid_regressors(cx, cy, order=3)
    want = [x, y, x * x, x * y, y * y, x * x * x, x * x * y, x * y * y, y * y * y]
    numpy.testing.assert_array_equal(got, numpy.array(want))
    assert got[3].tolist() == [1.0, 0.0, 0.0] and got[6].tolist() == [-1.0, 0.0, 0.0]
    assert survey.centroid_regressors(cx, cy, 1).shape == (2, 3) and survey.centroid_regressors(cx, cy).shape == (5, 3)
    batch = survey.centroid_regressors(numpy.array([cx, cy]), numpy.array([cy, cx]))
    assert batch.shape == (2, 5, 3)
    numpy.testing.assert_array_equal(batch[0], numpy.array(want[:5]))
    numpy.testing.assert_array_equal(batch[1, 0], y)                         # each row's own medians
    numpy.testing.assert_array_equal(cases.regressors(cx, cy), got[:5])
    for bad in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="centroid regressors: order must be an integer in \\[1, 3\\]"):
            survey.centroid_regressors(cx, cy, bad)
    with pytest.raises(ValueError, match="centroid regressors: cx_batch and cy_batch must share one shape"):
        survey.centroid_regressors(cx, cy[:2])
    with pytest.raises(ValueError, match="centroid regressors: cx_batch and cy_batch must be finite"):
        survey.centroid_regressors(cx, numpy.array([0.0, numpy.nan, 1.0]))


def test_decorrelate_segments():
    t = numpy.array([0.0, 0.1, 0.2, 0.3, 1.0, 1.1, 1.2, 1.3, 1.4, 1.5, 1.6, 1.7, 1.8])
    assert survey.decorrelate_segments(t).tolist() == [0, 4, 13]
    assert survey.decorrelate_segments(t, break_tolerance=1.0).tolist() == [0, 13]
    # the second segment spans 0.8 d: two parts of 0.4 d, the second from the first stamp >= 1.4
    assert survey.decorrelate_segments(t, 0.5, window_length=0.5).tolist() == [0, 4, 8, 13]
    assert survey.decorrelate_segments(t, 0.5, window_length=0.3).tolist() == [0, 4, 7, 10, 13]     # 0.8 / 3: from 1.2667 and 1.5333
    assert survey.decorrelate_segments(t, 0.5, window_length=5.0).tolist() == [0, 4, 13]
    assert survey.decorrelate_segments([3.0]).tolist() == [0, 1]
    assert survey.decorrelate_segments(t).dtype == numpy.int64
    with pytest.raises(ValueError, match="decorrelation segments: t must be finite and non-decreasing"):
        survey.decorrelate_segments(t[::-1])
    with pytest.raises(ValueError, match="decorrelation segments: break_tolerance must be a number > 0"):
        survey.decorrelate_segments(t, 0.0)
    with pytest.raises(ValueError, match="decorrelation segments: window_length must be None or finite and > 0"):
        survey.decorrelate_segments(t, 0.5, numpy.inf)


def test_the_fields_and_the_constants():
    assert survey.decorrelate_fields() == spec.FIELDS == _lib.DECOR_FIELDS
    assert _lib.DECOR_DTYPE.itemsize == 8 * len(spec.FIELDS)
    assert (_lib.DECOR_MAX_TERMS, _lib.DECOR_MAX_ITER, _lib.DECOR_PIVOT, _lib.DECOR_LDS_POINTS) == \
        (spec.MAX_TERMS, spec.MAX_ITER, spec.PIVOT, spec.LDS_POINTS) == (16, 16, 1e-10, 32768)
    header = open(cases.__file__.replace("tests/decorrelate_cases.py", "include/tls_amd.h")).read()
    for line in ("#define TLS_DECOR_MAX_TERMS 16", "#define TLS_DECOR_MAX_ITER 16", "#define TLS_DECOR_PIVOT 1e-10",
                 "#define TLS_DECOR_LDS_POINTS 32768"):
        assert line in header, line


# ---- the refusals: before any device work (no GPU here: a call that got as far as a context would raise RuntimeError) --------
_N = 12
_Y = numpy.linspace(1.0, 1.1, 2 * _N).reshape(2, _N)
_OWN = numpy.arange(2.0 * 3 * _N).reshape(2, 3, _N)
_SHARED = numpy.arange(2.0 * _N).reshape(2, _N)


def _nan(a):
    a = a.copy()
    a.flat[3] = numpy.nan
    return a


REFUSALS = [
    ("no_columns", dict(), "decorrelation: at least one of own and shared must be given"),
    ("flux_shape", dict(flux_batch=numpy.ones((2, 2, _N)), own=_OWN), "decorrelation: flux must be \\[n\\] or \\[n_curves, n\\]"),
    ("dy_shape", dict(own=_OWN, dy_batch=numpy.ones((2, _N + 1))), "decorrelation: flux and dy must be \\[n\\] or \\[n_curves, n\\]"),
    ("flux_nan", dict(flux_batch=_nan(_Y), own=_OWN), "decorrelation: flux has a NaN, infinite or non-positive value: decorrelation needs flux > 0"),
    ("flux_zero", dict(flux_batch=_Y - 1.0, own=_OWN), "decorrelation: flux has a NaN, infinite or non-positive value"),
    ("dy_zero", dict(own=_OWN, dy_batch=numpy.zeros((2, _N))), "decorrelation: dy has a NaN, infinite or non-positive value: decorrelation needs dy > 0"),
    ("dy_inf", dict(own=_OWN, dy_batch=numpy.full((2, _N), numpy.inf)), "decorrelation: dy has a NaN, infinite or non-positive value"),
    ("own_shape", dict(own=_OWN[:1]), "decorrelation: own must be \\[n_curves, n_own, n\\] = \\[2, n_own, 12\\], got \\(1, 3, 12\\)"),
    ("own_length", dict(own=_OWN[:, :, :5]), "decorrelation: own must be \\[n_curves, n_own, n\\]"),
    ("own_two_dimensions", dict(own=_OWN[0]), "decorrelation: own must be \\[n_curves, n_own, n\\]"),
    ("shared_shape", dict(shared=_SHARED[:, :5]), "decorrelation: shared must be \\[n_shared, n\\] with n = 12, got \\(2, 5\\)"),
    ("own_nan", dict(own=_nan(_OWN)), "decorrelation: own and shared must be finite"),
    ("shared_inf", dict(shared=numpy.where(numpy.isnan(_nan(_SHARED)), numpy.inf, _SHARED)), "decorrelation: own and shared must be finite"),
    ("not_numbers", dict(own="abc"), "decorrelation: own and shared must hold numbers"),
    ("too_many", dict(own=numpy.ones((2, 15, _N)), shared=_SHARED), "decorrelation: n_shared \\+ n_own must lie in \\[1, 16\\], got 2 \\+ 15"),
    ("no_term", dict(own=numpy.ones((2, 0, _N))), "decorrelation: n_shared \\+ n_own must lie in \\[1, 16\\], got 0 \\+ 0"),
    ("segments_start", dict(own=_OWN, segments=[1, _N]), "decorrelation: segments must hold integers ascending strictly from 0 to n = 12"),
    ("segments_end", dict(own=_OWN, segments=[0, 5]), "decorrelation: segments must hold integers ascending strictly from 0 to n = 12"),
    ("segments_tie", dict(own=_OWN, segments=[0, 5, 5, _N]), "decorrelation: segments must hold integers ascending strictly"),
    ("segments_float", dict(own=_OWN, segments=[0.0, 12.0]), "decorrelation: segments must hold integers ascending strictly"),
    ("ridge_negative", dict(own=_OWN, ridge=-1e-9), "decorrelation: ridge must be finite and >= 0, got -1e-09"),
    ("ridge_inf", dict(own=_OWN, ridge=numpy.inf), "decorrelation: ridge must be finite and >= 0"),
    ("ridge_nan", dict(own=_OWN, ridge=numpy.nan), "decorrelation: ridge must be finite and >= 0"),
    ("n_iter_high", dict(own=_OWN, n_iter=17), "decorrelation: n_iter must be an integer in \\[0, 16\\], got 17"),
    ("n_iter_negative", dict(own=_OWN, n_iter=-1), "decorrelation: n_iter must be an integer in \\[0, 16\\], got -1"),
    ("n_iter_float", dict(own=_OWN, n_iter=2.0), "decorrelation: n_iter must be an integer in \\[0, 16\\], got 2.0"),
    ("sigma_upper_zero", dict(own=_OWN, sigma_upper=0.0), "decorrelation: sigma_upper must be a number > 0, got 0.0"),
    ("sigma_lower_nan", dict(own=_OWN, sigma_lower=numpy.nan), "decorrelation: sigma_lower must be a number > 0, got nan"),
    ("sigma_lower_negative", dict(own=_OWN, sigma_lower=-5.0), "decorrelation: sigma_lower must be a number > 0"),
    ("mask_dtype", dict(own=_OWN, mask=numpy.zeros((2, _N))), "mask must be a uint8 or bool array, got dtype float64"),
    ("mask_shape", dict(own=_OWN, mask=numpy.zeros((2, _N - 1), dtype=bool)), "mask must have shape \\(2, 12\\)"),
]


@pytest.mark.parametrize("name,kwargs,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, kwargs, message):
    kwargs = dict(kwargs)
    flux = kwargs.pop("flux_batch", _Y)
    with pytest.raises(ValueError, match=message):
        survey.decorrelate_batch(flux, **kwargs)
    with pytest.raises(ValueError, match=message):
        _lib.decorrelate_arguments(flux, kwargs.pop("own", None), kwargs.pop("shared", None), kwargs.pop("dy_batch", None), **kwargs)


def test_what_the_checks_accept():
    a = _lib.decorrelate_arguments(_Y[0], own=_OWN[0], shared=_SHARED[0], sigma_upper=numpy.inf, n_iter=0, segments=numpy.array([0, 3, _N]))
    assert a["single"] and a["y"].shape == (1, _N) and a["own"].shape == (1, 3, _N) and a["shared"].shape == (1, _N)
    assert a["segments"].dtype == numpy.int64 and a["sigma_upper"] == numpy.inf and a["mask"] is None and a["dy"] is None
    a = _lib.decorrelate_arguments(_Y, shared=_SHARED, mask=numpy.zeros((2, _N), dtype=bool), dy=_Y)
    assert a["own"].shape == (2, 0, _N) and a["segments"].tolist() == [0, _N] and a["mask"].dtype == numpy.uint8


def test_the_step_on_the_survey_calls():
    step = survey.Decorrelate(own=_OWN)
    assert step.own is _OWN and step.segments is None
    assert step.n_iter == 3 and step.shared is None and step.ridge == 0.0 and step.sigma_upper == step.sigma_lower == 5.0
    assert survey._detrend_steps(step) == (step,) and survey._detrend_steps((step, 5))[0] is step
    t = numpy.arange(_N) / 48.0
    for call, name in ((survey.injection_recovery, "injection_recovery"), (survey.null_sde, "null_sde")):
        for detrend in (step, (survey.Biweight(0.5), step)):
            with pytest.raises(ValueError, match="%s forms its rows on the device from ONE star and has no columns for them: "
                                                 "detrend=Decorrelate belongs on search_batch, power_batch" % name):
                if call is survey.null_sde:
                    call(t, 4, detrend=detrend, sigma=1e-3)
                else:
                    call(t, numpy.ones(_N), {"T0": [0.1], "period": [0.1], "rp_rs": [0.05], "a": [10.0], "inc": [90.0]},
                         detrend=detrend)
    # a pass of power_batch_multi searches some of the curves: the step follows them
    rows = numpy.array([1])
    assert survey._detrend_of_rows(5, rows) == 5 and survey._detrend_of_rows(None, rows) is None
    biweight = survey.Biweight(0.5)
    assert survey._detrend_of_rows((biweight, 5), rows) == (biweight, 5)
    one = survey._detrend_of_rows(step, rows)
    assert isinstance(one, survey.Decorrelate) and numpy.array_equal(one.own, _OWN[1:]) and one[1:] == step[1:]
    both = survey._detrend_of_rows((survey.Decorrelate(shared=_SHARED), step, biweight), rows)
    assert both[0].own is None and both[0].shared is _SHARED and numpy.array_equal(both[1].own, _OWN[1:]) and both[2] is biweight
    # the messages of the steps before stay
    with pytest.raises(ValueError, match="a step of detrend must be a kernel size, a Biweight or a SysRem"):
        survey._detrend_steps((step, None))
