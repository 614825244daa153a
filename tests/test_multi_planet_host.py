"""The multi-planet search without a GPU: the statement of the removal (tests/remove_transits_spec.py) equals its own loops bit
for bit, leaves untouched what no model touches, applies the candidates of a curve in their order and skips every candidate
that cannot take part; its model is the transit fit's own at the fit's members; the two survey calls refuse bad arguments
before a context is touched; header, binding and version comment name the entry; and the measurement of DESIGN.md
"Multi-planet search" end to end on the statement, with the oracle search injected as tests/test_power_host.py injects it."""
import math
import os
import re
import warnings

import numpy
import pytest

import multi_planet_cases as cases
import remove_transits_spec as spec
import transit_fit_spec as fit_spec
import tls_amd
from conftest import REPO
from tls_amd import _lib, survey


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64))


def both(a):
    """(rows, model, status) of the vectorised form, checked against the loops."""
    fast = spec.remove_transits(**a)
    slow = spec.remove_transits_loops(**a)
    for x, y in zip(fast, slow):
        assert same(x, y)
    return fast


# ---- the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, S, offset, many", [(64, 1, 0.0, False), (64, 5, 0.0, True), (1024, 5, 2457000.0, False)])
def test_the_loops_equal_the_vectorised_form(M, S, offset, many):
    a = cases.layout(257, M, S, offset, many)
    rows, model, status = both(a)
    assert status.tolist() == [0, 0, 0, 0, 1, 0]
    assert same(rows[0], a["y"][0]) and numpy.all(model[0] == 1.0)            # (no candidate: byte for byte)
    for c in (1, 2, 3, 4):
        touched = model[c] != 1.0
        assert 0 < touched.sum() < 0.5 * len(touched)
        assert same(rows[c][~touched], a["y"][c][~touched])                   # (mval == 0: byte for byte)
        assert numpy.all(rows[c][touched] > a["y"][c][touched]) and numpy.all(model[c][touched] < 1.0)
    if many:
        assert (a["t"][-1] - a["t"][0]) / a["P"][0] > 40.0


def test_two_candidates_of_a_curve_are_applied_in_their_order():
    a = cases.layout(257, 64, 5)
    rows, model, status = both(a)
    one = {k: (v[1:2] if k in ("curve", "P", "T0", "row", "A", "b", "T", "c0") else v) for k, v in a.items()}
    first = spec.remove_transits(**one)
    two = {k: (v[2:3] if k in ("curve", "P", "T0", "row", "A", "b", "T", "c0") else v) for k, v in a.items()}
    second = spec.remove_transits(**dict(two, y=first[0]))
    assert same(second[0][2], rows[2])                                        # (f = 1, then f = 2 on its result)
    both_dip = (first[1][2] != 1.0) & (second[1][2] != 1.0)
    assert both_dip.sum() >= 2                                                # (the transits coincide at an epoch)
    assert same(first[1][2] * second[1][2], model[2])
    swapped = {k: (v[[0, 2, 1, 3, 4, 5]] if k in ("curve", "P", "T0", "row", "A", "b", "T", "c0") else v) for k, v in a.items()}
    other = spec.remove_transits(**swapped)
    assert not same(other[0][2], rows[2]) and numpy.allclose(other[0][2], rows[2], rtol=1e-14, atol=0)


@pytest.mark.parametrize("field, value", [
    ("P", numpy.nan), ("P", numpy.inf), ("P", 0.0), ("P", -1.0), ("T0", numpy.nan), ("T0", -numpy.inf), ("A", numpy.nan),
    ("A", 0.0), ("A", -0.5), ("A", 1e3), ("b", numpy.nan), ("b", -0.1), ("b", 1.2), ("T", numpy.nan), ("T", 0.0), ("T", -0.1),
    ("T", numpy.inf), ("c0", numpy.nan), ("c0", numpy.inf)])
def test_every_skip_reason(field, value):
    a = cases.layout(257, 64, 1)
    a[field] = a[field].copy()
    a[field][0] = value                                                       # (curve 1's only candidate)
    rows, model, status = both(a)
    assert status[0] == 1.0 and status[1:].tolist() == [0, 0, 0, 1, 0]
    assert same(rows[1], a["y"][1]) and numpy.all(model[1] == 1.0)


def test_the_grazing_candidate_is_just_inside_and_the_next_value_is_skipped():
    a = cases.layout(257, 64, 1)
    e1 = 1.0 + a["k_rows"][a["row"][3]]
    assert a["b"][3] * a["b"][3] < e1 * e1 and a["b"][3] > e1 * (1.0 - 1e-11)
    a["b"] = a["b"].copy()
    a["b"][3] = e1
    assert both(a)[2][3] == 1.0                                               # (bb == e2)


def test_the_model_is_the_fit_own_at_its_members():
    """model == 1 - A * mval of transit_fit_spec.model_values for the fit's own unit at the fit's members."""
    k_rows, table = cases.profile(64, numpy.geomspace(0.03, 0.15, 9))
    t = cases.T[:500]
    y = cases.curve(5)[:500]
    dy = numpy.full(len(t), numpy.std(y))
    sub = fit_spec.sub_offsets(float(numpy.median(numpy.diff(t))), 5)
    P, T0, d = 2.1, 0.7, 0.1
    impacts, ratios, shifts = [0.0, 0.4, 0.8], [0.8, 1.0, 1.25], [-0.1, 0.0, 0.1]
    rec = dict(zip(fit_spec.FIELDS, fit_spec.transit_fit(t, y, dy, P, T0, d, 6, k_rows, table, impacts, ratios, shifts, sub)))
    assert rec["status"] == 0.0
    j = int(rec["row"])
    rows, model, status = spec.remove_transits(t, y, [0], [P], [T0], [j], [rec["amplitude"]], [rec["b"]], [rec["duration"]],
                                               [rec["shift"]], k_rows, table, sub)
    index, taus = fit_spec.members_of(t, P, T0, 1.0 * d)
    mval, _ = fit_spec.model_values(taus, table[j], k_rows[j], 64, d, impacts, ratios, shifts, sub)
    unit = (int(rec["i_impact"]) * len(ratios) + int(rec["i_duration"])) * len(shifts) + int(rec["i_shift"])
    mine = mval[:, unit]
    assert (mine > 0.0).sum() == rec["n_in"] > 0
    want = numpy.where(mine > 0.0, 1.0 - rec["amplitude"] * mine, 1.0)
    assert status.tolist() == [0.0] and same(model[0][index], want)
    outside = numpy.ones(len(t), dtype=bool)
    outside[index] = False
    assert numpy.all(model[0][outside] == 1.0)                                # (the window holds the whole model)


def test_the_repeat_rule():
    assert spec.is_repeat(2.1028, 2.0994) and survey.is_repeat(2.1028, 2.0994)
    assert spec.is_repeat(4.2, 2.0994) and spec.is_repeat(1.05, 2.0994) and spec.is_repeat(0.7, 2.0994)
    assert not spec.is_repeat(3.7016, 2.0994) and not survey.is_repeat(numpy.nan, 2.0994)
    periods = numpy.linspace(0.5, 8.0, 3001)
    for sep, ratios in ((0.02, survey.HARMONICS), (0.05, ()), (0.01, (0.5, 2.0))):
        want = [spec.is_repeat(p, 2.0994, sep, ratios) for p in periods]
        assert survey.is_repeat(periods, 2.0994, sep, ratios).tolist() == want


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_remove_transits"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "(8: %s)" % name in text.split("#define TLS_AMD_ABI_VERSION")[0]
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_remove_transits.argtypes) == declared.count(",") + 1 == 23
    assert declared.endswith("double *out_rows, double *out_model, double *out_status")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_remove.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_remove.hip.h")).read()
    assert "__syncthreads" not in re.sub(r"//[^\n]*", "", kernel) and "wg_sync();" in kernel
    assert "#pragma clang fp contract(off)" in kernel
    names = [n for n in vars(_lib.Context) if not n.startswith("_")]
    assert names.index("remove_transits") > names.index("prewhiten_masked") > names.index("ephemeris_match")
    assert callable(_lib.remove_transits_arguments) and callable(survey.remove_transits) and callable(survey.power_batch_multi)


GOOD = dict(t=cases.T[:300], y=numpy.ones((2, 300)), period=[2.0, 3.0], T0=[0.5, 0.6], row=[0, 8], amplitude=[1.0, 1.0],
            b=[0.1, 0.2], duration=[0.1, 0.2], shift=[0.0, 0.01], sub=[-0.005, 0.005], curve=[0, 0])


@pytest.mark.parametrize("kw", [
    dict(curve=[0, 2]), dict(curve=[-1, 0]), dict(curve=[0]), dict(curve=[0.0, 1.0]), dict(T0=[1.0]), dict(t=cases.T[:300][::-1]),
    dict(y=numpy.ones((2, 299))), dict(row=[0, 9]), dict(row=[-1, 0]), dict(row=[0]), dict(row=[0.5, 1.0]), dict(row=["a", "b"]),
    dict(sub=[numpy.inf]), dict(sub=numpy.zeros(17)), dict(sub=[]), dict(k_rows=numpy.geomspace(0.03, 0.15, 9)[::-1]),
    dict(k_rows=numpy.geomspace(0.03, 0.15, 8)), dict(profile=numpy.ones((9, 1))), dict(profile=numpy.ones((9, 4098))),
    dict(profile=numpy.full((9, 65), numpy.nan)), dict(period=["x", "y"])])
def test_remove_transits_arguments_refuses(kw):
    k_rows, table = cases.profile(64, numpy.geomspace(0.03, 0.15, 9))
    with pytest.raises(ValueError, match="^remove transits: "):
        _lib.remove_transits_arguments(**dict(dict(GOOD, k_rows=k_rows, profile=table), **kw))


def test_remove_transits_arguments_packs():
    k_rows, table = cases.profile(64, numpy.geomspace(0.03, 0.15, 9))
    one = {k: (v[:1] if k in ("period", "T0", "row", "amplitude", "b", "duration", "shift") else v) for k, v in GOOD.items()}
    a = _lib.remove_transits_arguments(**dict(one, k_rows=k_rows, profile=table, period=[numpy.nan], y=numpy.ones(300), curve=None))
    assert a["y"].shape == (1, 300) and a["curve"] is None and numpy.isnan(a["period"][0])
    a = _lib.remove_transits_arguments(**dict(GOOD, k_rows=k_rows, profile=table, row=numpy.array([numpy.nan, 8.0])))
    assert a["row"].tolist() == [0, 8] and a["row"].dtype == numpy.int64 and numpy.isnan(a["amplitude"][0]) and a["amplitude"][1] == 1.0
    assert a["curve"].tolist() == [0, 0] and a["profile"].shape == (9, 65) and a["sub"].tolist() == [-0.005, 0.005]


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


def _planets(n, **fields):
    out = numpy.zeros(n, dtype=[(k, "f8") for k in _lib.REMOVE_TRANSITS_FIELDS])
    for k, v in dict(dict(period=2.0, T0=0.5, fit_row=3.0, fit_amplitude=1.0, fit_b=0.1, fit_duration=0.1, fit_shift=0.0),
                     **fields).items():
        out[k] = v
    return out


@pytest.mark.parametrize("kw, match", [
    (dict(planets=numpy.zeros(2)), "structured"), (dict(planets=_planets(2)[["period", "T0"]]), "structured"),
    (dict(planets=_planets(3)), "planets must be"), (dict(curve=[0, 2]), "curve"), (dict(curve=[0]), "curve"),
    (dict(planets=_planets(2, fit_row=81.0)), "row"), (dict(planets=_planets(2, fit_row=0.5)), "row"),
    (dict(n_sub=0), "n_sub"), (dict(n_sub=17), "n_sub"), (dict(exposure=-1.0), "exposure"), (dict(profile=3), "profile"),
    (dict(t=cases.T[:300][::-1]), "non-decreasing"), (dict(flux_batch=numpy.ones((2, 299))), "flux_batch")])
def test_remove_transits_refuses_before_any_device_work(no_device, kw, match):
    args = dict(dict(t=cases.T[:300], flux_batch=numpy.ones((2, 300)), planets=_planets(2), profile=cases.profile()), **kw)
    with pytest.raises(ValueError, match=match):
        survey.remove_transits(**args)
    with pytest.raises(AssertionError, match="a context was created"):       # (a good call reaches the device)
        survey.remove_transits(cases.T[:300], numpy.ones((2, 300)), _planets(2, period=[numpy.nan, 2.0]), profile=cases.profile())


@pytest.mark.parametrize("kw, match", [
    (dict(sde_min=numpy.nan), "sde_min"), (dict(sde_min="9"), "sde_min"), (dict(sde_min=True), "sde_min"),
    (dict(n_planets=0), "n_planets"), (dict(n_planets=9), "n_planets"), (dict(n_planets=2.0), "n_planets"),
    (dict(protect_factor=0.0), "protect_factor"), (dict(protect_factor=numpy.inf), "protect_factor"),
    (dict(protect_factor=1.5, detrend=25), "median filter"), (dict(transit_fit=False), "transit_fit"),
    (dict(transit_fit=dict(windows=1.0)), "keys"), (dict(transit_fit=dict(n_sub=0)), "n_sub"), (dict(peaks=3), "peaks"),
    (dict(statistics=True), "statistics"), (dict(detrend_mask=numpy.zeros((2, 300), dtype=bool)), "detrend_mask"),
    (dict(peak_separation=-1.0), "separation"), (dict(flux_batch=numpy.ones(300)), "flux_batch"),
    (dict(dy_batch=numpy.ones((3, 300))), "dy_batch")])
def test_power_batch_multi_refuses_before_any_device_work(no_device, kw, match):
    args = dict(dict(t=cases.T[:300], flux_batch=numpy.ones((2, 300)), sde_min=9.0, transit_fit=dict(profile=cases.profile())), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch_multi(**args)


def test_sde_min_has_no_default():
    with pytest.raises(TypeError):
        survey.power_batch_multi(cases.T[:300], numpy.ones((2, 300)))


def test_the_fields_of_the_planets_array():
    summary = numpy.dtype([("SDE", "f8"), ("period", "f8"), ("T0", "f8"), ("index_best", "i8"), ("duration", "f8")])
    peaks = numpy.dtype([("period", "f8"), ("T0", "f8"), ("status", "f8"), ("fit_status", "f8")])
    names = [k for k, _ in survey.multi_planet_fields(summary, peaks)]
    assert names == ["pass_status", "SDE", "summary_period", "summary_T0", "index_best", "summary_duration", "period", "T0",
                     "status", "fit_status"]
    assert (survey.PLANET_ACCEPTED, survey.PLANET_NOT_REACHED, survey.PLANET_BELOW_SDE, survey.PLANET_NO_FIT,
            survey.PLANET_REPEAT) == (0, 1, 2, 3, 4)


# ---- the measurement, end to end on the statement ---------------------------------------------------------------------------
@pytest.fixture()
def make_model(monkeypatch, oracle_lib):
    def oracle_search_periods(t, y, dy, periods, table, transit_depth_min, R_star_min, R_star_max,
                              M_star_min, M_star_max, T0_fit_margin, **_unused):
        chi2, row, depth, _ = oracle_lib.search(t, y, dy, periods, table, transit_depth_min,
                                                R_star_min, R_star_max, M_star_min, M_star_max,
                                                T0_fit_margin)
        return chi2, row, depth

    def host_t0_fit_residuals(t, y, period, signal, T0_array, roll, **_unused):
        return oracle_lib.t0_residuals(t, y, period, signal, T0_array, roll)

    def oracle_spectra(chi2, oversampling_factor, **_unused):
        return oracle_lib.spectra(chi2, int(oversampling_factor * 30))

    monkeypatch.setattr(tls_amd.search, "spectra", oracle_spectra)
    monkeypatch.setattr(tls_amd.search, "search_periods", oracle_search_periods)
    monkeypatch.setattr(tls_amd.search, "t0_fit_residuals", host_t0_fit_residuals)
    return lambda t, y, dy: tls_amd.transitleastsquares(t, y, dy, verbose=False)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_second_planet_appears_once_the_first_is_divided_out(make_model, seed):
    """Three passes of power() on the statement's quotients: 2.1 d, then 3.7 d (absent from pass 1's periodogram), then
    nothing above 9."""
    t, raw = cases.T, cases.curve(seed)
    k_rows, table = cases.profile()
    sub = fit_spec.sub_offsets(float(numpy.median(numpy.diff(t))), 5)
    y, found, passes = raw, [], []
    for _ in range(3):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = make_model(t, y, None).power(verbose=False, show_progress_bar=False, **cases.SEARCH)
        passes.append(r)
        dy = numpy.full(len(t), numpy.std(y))
        j0 = fit_spec.nearest_row(k_rows, math.sqrt(max(1.0 - r.depth, 0.0)))
        rec = dict(zip(fit_spec.FIELDS, fit_spec.transit_fit(
            t, y, dy, r.period, r.T0, r.duration, j0, k_rows, table, fit_spec.DEFAULT_IMPACTS, fit_spec.DEFAULT_RATIOS,
            fit_spec.DEFAULT_SHIFTS, sub)))
        assert rec["status"] == 0.0
        found.append((r.period, r.T0, int(rec["row"]), rec["amplitude"], rec["b"], rec["duration"], rec["shift"]))
        P, T0, row, A, b, T, c0 = zip(*found)
        rows, model, status = spec.remove_transits(t, raw, numpy.zeros(len(found), dtype=numpy.int64), P, T0, row, A, b, T, c0,
                                                   k_rows, table, sub)                # (from the raw row every time)
        assert numpy.all(status == 0.0)
        y = rows[0]
    print("seed %d:" % seed, ["%.4f d SDE %.2f" % (r.period, r.SDE) for r in passes])
    first, second, third = passes
    near = numpy.fabs(first.periods - 3.7) <= 0.02 * 3.7
    print("   power within 2 %% of 3.7 d in pass 1: %.3f" % first.power[near].max())
    assert abs(first.period - 2.1) <= 0.01 * 2.1
    assert first.power[near].max() < 1.0
    assert abs(second.period - 3.7) <= 0.01 * 3.7 and second.SDE > 9.0
    assert third.SDE < 9.0
    assert not spec.is_repeat(second.period, first.period)
    if seed in (0, 2):                               # (what is left of the first planet: a repeat, and below 9 anyway)
        assert spec.is_repeat(third.period, first.period)
