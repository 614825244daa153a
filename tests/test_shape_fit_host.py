"""The shape fit without a GPU: the statement (tests/shape_fit_spec.py) equals its own loops bit for bit -- gaps, exact ties,
constant flux, bad ephemerides --; it tells a planet from a grazing binary and recovers the contacts of a uniform disc;
transit_geometry inverts the contact times of Seager & Mallen-Ornelas (2003); the argument checks of the Python layer, all
raised before any device work; the field lists; and the header, the binding and the version comment name tls_shape_fit."""
import ctypes
import math
import os
import re
import warnings

import numpy
import pytest

import shape_fit_spec as spec
from conftest import REPO
from tls_amd import _lib, survey, transit_model

T = 1.0 + numpy.arange(300) / 64.0
RATIOS, INGRESS, SHIFTS = [0.5, 0.75, 1.0, 1.5, 2.0], [0.0, 0.125, 0.25, 0.5], [-0.25, 0.0, 0.25]


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64))


def both(t, y, dy, P, T0, d, ratios=RATIOS, ingress=INGRESS, shifts=SHIFTS, **kw):
    """The record of the vectorised form, checked against the loops."""
    fast = spec.shape_fit(t, y, dy, P, T0, d, ratios, ingress, shifts, **kw)
    slow = spec.shape_fit_loops(t, y, dy, P, T0, d, ratios, ingress, shifts, **kw)
    assert same(fast, slow), (fast, slow)
    return dict(zip(spec.FIELDS, fast))


def gapped(seed, points=600):
    """30 min cadence on multiples of 1/64 d with two gaps, a transit of period 1.75 d, noise and per-point errors."""
    rng = numpy.random.RandomState(seed)
    t = numpy.delete(1.0 + numpy.arange(points) / 64.0, numpy.r_[100:180, 400:431])
    dy = 1e-3 * (1.0 + 0.5 * rng.uniform(size=len(t)))
    y = transit_model.light_curve(t, 1.5, 1.75, 0.08, 6.0, 88.0, 0, 90, [0.4, 0.4], "quadratic") + rng.normal(0, 1.0, len(t)) * dy
    return t, y, dy


# ---- the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_loops_equal_the_vectorised_form(seed):
    t, y, dy = gapped(seed)
    r = both(t, y, dy, 1.75, 1.5 + 0.01 * seed, 0.11)
    assert r["status"] == 0.0 and r["n_in"] >= 3 and r["ses"] > 10 and r["ses"] >= max(r["ses_box"], r["ses_vee"])
    assert r["depth_err"] > 0 and r["duration"] == 0.11 * RATIOS[int(r["i_duration"])]
    assert r["ingress"] == INGRESS[int(r["i_ingress"])] and r["shift"] == 0.11 * SHIFTS[int(r["i_shift"])]
    r = both(t, y, dy, 1.75, 1.5, 0.11, min_count=40, depth_min=1e-3)       # (the narrow units have too few points)
    assert r["status"] == 0.0 and r["n_in"] >= 40


def test_exact_ties_go_to_the_first_unit():
    t, y, dy = gapped(3)
    r = both(t, y, dy, 1.75, 1.5, 0.11, shifts=[0.0, 0.0, 0.0])             # (three equal shifts: three equal units each)
    assert r["status"] == 0.0 and r["i_shift"] == 0.0
    # a curve symmetric about the epochs: shifts -c and +c see mirrored members; with one transit and equal weights the sums
    # run over the same values in opposite order -- equal where the additions are exact, as here (dyadic values)
    t1 = numpy.arange(-32, 33) / 64.0
    y1 = 1.0 - numpy.where(numpy.fabs(t1) <= 4 / 64.0, 1 / 64.0, 0.0)
    r = both(t1, y1, numpy.full(len(t1), 0.5), 4.0, 0.0, 0.125, ratios=[1.0, 2.0], ingress=[0.0, 0.5], shifts=[-0.25, 0.25])
    assert r["status"] == 0.0 and r["i_shift"] == 0.0 and r["shift"] == -0.03125
    r = both(t1, y1, numpy.full(len(t1), 0.5), 4.0, 0.0, 0.125, ratios=[1.0, 1.0], ingress=[0.0, 0.0, 0.5, 0.5], shifts=[0.0])
    assert (r["i_duration"], r["i_ingress"]) == (0.0, 0.0) and r["ses_box"] == r["ses"] and r["ses_vee"] < r["ses_box"]


def test_constant_flux_has_no_valid_unit():
    t, y, dy = gapped(4)
    r = both(t, numpy.ones(len(t)), dy, 1.75, 1.5, 0.11)
    assert r["status"] == 2.0 and r["n_points"] > 50
    assert all(math.isnan(r[k]) for k in spec.FIELDS[2:])
    r = both(t, 2.0 - y, dy, 1.75, 1.5, 0.11, depth_min=1e-3)             # (a brightening is no dip)
    assert r["status"] == 2.0
    r = both(t, y, dy, 1.75, 1.5, 0.11, min_count=10 ** 6)
    assert r["status"] == 2.0
    r = both(t, y, dy, 1.75, 1.5 + 100 / 64.0 + 0.6, 0.02, ratios=[0.5, 1.0], shifts=[0.0])   # (every epoch in a gap or thin)
    assert r["status"] in (0.0, 2.0)


@pytest.mark.parametrize("P, T0, d", [(numpy.nan, 1.5, 0.1), (1.75, numpy.inf, 0.1), (1.75, 1.5, numpy.nan), (0.0, 1.5, 0.1),
                                      (-1.75, 1.5, 0.1), (1.75, 1.5, 0.0), (1.75, 1.5, -0.1), (1.75, 1.5, numpy.inf),
                                      (0.4, 1.5, 0.1), (0.5, 1.5, 0.125)])
def test_no_such_candidate(P, T0, d):
    """Status 1: a bad ephemeris, and a window of half a period or more (window * d >= P / 2; 2 * 0.125 is 0.5 * 0.5)."""
    t, y, dy = gapped(5)
    r = both(t, y, dy, P, T0, d)
    assert r["status"] == 1.0 and all(math.isnan(r[k]) for k in spec.FIELDS[1:])


def test_the_window_just_below_half_a_period_is_fitted():
    t, y, dy = gapped(5)
    assert both(t, y, dy, 0.5 + 2.0 ** -40, 1.5, 0.125)["status"] != 1.0


# ---- what the fit is for ----------------------------------------------------------------------------------------------------
def contacts(P, k, a, b):
    """(T14, T23) of Seager & Mallen-Ornelas (2003), equations 3 and 4, circular orbit (T23 NaN for a grazing transit)."""
    sin_i = math.sqrt(1.0 - (b / a) ** 2)
    flat = (1 - k) ** 2 - b * b
    return (P / math.pi * math.asin(math.sqrt((1 + k) ** 2 - b * b) / (a * sin_i)),
            P / math.pi * math.asin(math.sqrt(flat) / (a * sin_i)) if flat >= 0 else math.nan)


CASES = [(3.7, 0.07, 12, 0.1), (10, 0.1, 20, 0.5), (1.2, 0.03, 4, 0.8), (365.25, 0.00916, 215, 0.3)]


@pytest.mark.parametrize("P, k, a, b", CASES)
def test_transit_geometry_inverts_the_contact_times(P, k, a, b):
    """The formulas are exact inverses: only rounding separates them (3e-14 at worst in a prototype; asked: 1e-9)."""
    t14, t23 = contacts(P, k, a, b)
    impact, a_rs, rho = survey.transit_geometry(P, k * k, t14, (1.0 - t23 / t14) / 2.0)
    print("b %.3e a/R* %.3e rho %.6f" % (abs(impact / b - 1), abs(a_rs / a - 1), rho))
    assert abs(impact / b - 1) <= 1e-9 and abs(a_rs / a - 1) <= 1e-9
    if P == 365.25:
        assert abs(rho - 1.0) <= 0.01            # (the Earth's orbit around the Sun)


def test_transit_geometry_broadcasts_and_refuses_with_nan():
    P, k, a, b = zip(*CASES)
    c = [contacts(*case) for case in CASES]
    t14, t23 = numpy.array([v[0] for v in c]), numpy.array([v[1] for v in c])
    impact, a_rs, rho = survey.transit_geometry(P, numpy.square(k), t14, (1.0 - t23 / t14) / 2.0)
    assert numpy.allclose(impact, b, rtol=1e-9) and numpy.allclose(a_rs, a, rtol=1e-9) and rho.shape == (4,)
    for bad in ((numpy.nan, 0.01, 0.1, 0.1), (3.0, numpy.nan, 0.1, 0.1), (3.0, 0.01, numpy.inf, 0.1), (3.0, 0.01, 0.1, numpy.nan),
                (3.0, 0.01, 0.1, 0.0), (3.0, 0.01, 0.1, 0.01)):               # (the last two: b^2 < 0, sharper than a central transit)
        assert all(numpy.isnan(v) for v in survey.transit_geometry(*bad)), bad
    impact, a_rs, rho = survey.transit_geometry(3.0, 0.01, 0.1, 0.5)           # (a V is the grazing b = 1 - k)
    assert abs(impact - 0.9) < 1e-12 and a_rs > 0 and rho > 0


def observed(seed, rp, inc):
    """The record of the default tables on 90 d at 48 a day, sigma 3e-4, P 3.7, a 12, quadratic (0.4, 0.4): the fit is handed
    T0 + 0.01 and 0.9 of the true T14."""
    n, P, a, T0 = 90 * 48, 3.7, 12.0, 3.14 + 1.234
    t = numpy.linspace(3.14, 3.14 + 90, n)
    flux = transit_model.light_curve(t, T0, P, rp, a, inc, 0, 90, [0.4, 0.4], "quadratic") \
        + numpy.random.RandomState(seed).normal(0, 3e-4, n)
    t14 = contacts(P, rp, a, a * math.cos(math.radians(inc)))[0]
    r = spec.shape_fit(t, flux, numpy.full(n, 3e-4), P, T0 + 0.01, 0.9 * t14, spec.DEFAULT_RATIOS, spec.DEFAULT_INGRESS,
                       spec.DEFAULT_SHIFTS)
    return dict(zip(spec.FIELDS, r))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_shape_separates_a_planet_from_a_grazing_binary(seed):
    """Seeds 0 to 2 of a prototype: the planet has ses_box 188.2 against ses_vee 186.7 and ingress 0.13 to 0.20, the binary
    ses_vee 290.2 against ses_box 277.2 and ingress 0.37.  No threshold on ingress itself."""
    planet, binary = observed(seed, 0.07, 89.5), observed(seed, 0.35, 84.4)
    for name, r in (("planet", planet), ("binary", binary)):
        print("%s seed %d: ses_box %.1f ses_vee %.1f ses %.1f ingress %.3f duration %.4f"
              % (name, seed, r["ses_box"], r["ses_vee"], r["ses"], r["ingress"], r["duration"]))
    assert planet["status"] == 0.0 and binary["status"] == 0.0
    assert planet["ses_box"] > planet["ses_vee"]
    assert binary["ses_vee"] > binary["ses_box"]
    assert planet["ingress"] < binary["ingress"]


def test_a_noise_free_uniform_disc_gives_its_contacts_back():
    """27 d at 720 a day, rp 0.1, a 15, inc 90, no limb darkening: the geometric T12/T14 is 0.0909 and the grids resolve 1/30
    in ingress and 2^(1/8) in duration (a prototype gave ingress 0.067)."""
    n, P, T0 = 27 * 720, 3.7, 3.14 + 1.234
    t = numpy.linspace(3.14, 3.14 + 27, n)
    flux = transit_model.light_curve(t, T0, P, 0.1, 15.0, 90.0, 0, 90, [0.0, 0.0], "quadratic")
    t14, t23 = contacts(P, 0.1, 15.0, 0.0)
    geometric = (1.0 - t23 / t14) / 2.0
    assert abs(geometric - 0.0909) < 5e-4        # (0.09103; k / (1 + k) is 0.0909)
    r = dict(zip(spec.FIELDS, spec.shape_fit(t, flux, numpy.full(n, 1e-4), P, T0, t14, spec.DEFAULT_RATIOS,
                                             spec.DEFAULT_INGRESS, spec.DEFAULT_SHIFTS)))
    print("ingress %.4f (geometric %.4f) duration %.5f (T14 %.5f)" % (r["ingress"], geometric, r["duration"], t14))
    assert r["status"] == 0.0
    assert abs(r["ingress"] - geometric) <= 1 / 30.0
    assert t14 / 2 ** 0.125 <= r["duration"] <= t14 * 2 ** 0.125
    assert r["ses_box"] > r["ses_vee"]


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_field_lists_and_defaults():
    assert spec.FIELDS == _lib.SHAPE_FIELDS == _lib.SHAPE_DTYPE.names and len(spec.FIELDS) == 16
    assert survey.shape_fit_fields() == tuple("shape_" + k for k in spec.FIELDS) + ("shape_delta_chi2", "shape_impact",
                                                                                      "shape_a_rs", "shape_rho_star")
    assert survey.shape_fit_fields()[0] == "shape_status"
    assert ctypes.sizeof(_lib.ShapeRecord) == 128 == _lib.SHAPE_DTYPE.itemsize
    assert spec.MAX_UNITS == _lib.SHAPE_MAX_UNITS == 65536
    for mine, theirs, want in ((survey.SHAPE_FIT_RATIOS, spec.DEFAULT_RATIOS, numpy.geomspace(0.5, 2.0, 17)),
                               (survey.SHAPE_FIT_INGRESS, spec.DEFAULT_INGRESS, numpy.linspace(0.0, 0.5, 16)),
                               (survey.SHAPE_FIT_SHIFTS, spec.DEFAULT_SHIFTS, numpy.linspace(-0.25, 0.25, 9))):
        assert same(mine, want) and same(theirs, want)
    assert len(survey.SHAPE_FIT_RATIOS) * len(survey.SHAPE_FIT_INGRESS) * len(survey.SHAPE_FIT_SHIFTS) == 2448
    assert survey.SHAPE_FIT_INGRESS[0] == 0.0 and survey.SHAPE_FIT_INGRESS[-1] == 0.5


def test_the_record_of_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct tls_shape_record \{(.*?)\} tls_shape_record;", code, flags=re.S).group(1)
    declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
    assert tuple(declared) == _lib.SHAPE_FIELDS
    assert "#define TLS_SHAPE_MAX_UNITS 65536" in text
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_shape.hip.h")).read()
    assert "constexpr int kShapeMaxUnits = 65536;" in kernel and "constexpr int kShapeWords = 16;" in kernel
    assert "constexpr int kShapeLdsMembers = %d;" % _lib.SHAPE_LDS_MEMBERS in kernel
    assert "constexpr int kShapeMaxPoints = 1 << 22;" in kernel and _lib.SHAPE_MAX_POINTS == 1 << 22
    assert "__syncthreads" not in re.sub(r"//[^\n]*", "", kernel) and "wg_sync();" in kernel
    assert "#pragma clang fp contract(off)" in kernel and "kChkShape" in kernel


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_shape_fit"
    assert re.search(r"\bint\s+%s\s*\(" % name, code)
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "(7: %s)" % name in text.split("#define TLS_AMD_ABI_VERSION")[0]     # (the version comment lists the entries it gained)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert len(lib.tls_shape_fit.argtypes) == declared.count(",") + 1 == 21
    assert declared.endswith("double window, int64_t min_count, double depth_min, tls_shape_record *out")
    makefile = open(os.path.join(REPO, "tls_amd", "csrc", "Makefile")).read()
    assert "tls_shape.hip.h" in re.search(r"^HDR = (.*)$", makefile, flags=re.M).group(1)
    assert hasattr(_lib.Context, "shape_fit") and callable(_lib.shape_fit_arguments)


BAD = [
    (dict(ratios=[1.0, 0.5]), "ratios"), (dict(ratios=[1.0, numpy.nan]), "ratios"), (dict(ratios=[0.0, 1.0]), "ratio"),
    (dict(ratios=[]), "ratios"), (dict(ratios=[[1.0]]), "ratios"), (dict(ratios="x"), "ratios"),
    (dict(ingress=[0.0, 0.3, 0.2, 0.5]), "ingress"), (dict(ingress=[0.1, 0.5]), "ingress must run"),
    (dict(ingress=[0.0, 0.4]), "ingress must run"), (dict(ingress=[0.0]), "ingress must run"),
    (dict(ingress=[0.0, numpy.inf]), "ingress"), (dict(shifts=[0.1, 0.0]), "shifts"), (dict(shifts=[numpy.nan]), "shifts"),
    (dict(ratios=numpy.linspace(0.5, 2.0, 64), ingress=numpy.linspace(0.0, 0.5, 64), shifts=numpy.linspace(-0.25, 0.25, 17)),
     "units"),
    (dict(window=numpy.nan), "window"), (dict(window=numpy.inf), "window"), (dict(window="2"), "window"),
    (dict(window=1.2), "window"), (dict(window=1.0, ratios=[1.0], shifts=[-0.6, 0.0]), "window"),
    (dict(min_count=0), "min_count"), (dict(min_count=2.5), "min_count"), (dict(min_count=True), "min_count"),
    (dict(transit_depth_min=-1e-6), "depth_min"), (dict(transit_depth_min=numpy.nan), "depth_min"),
    (dict(period=[1.0]), "n_fits"), (dict(period=[[1.0, 1.5]]), "n_fits"), (dict(T0=["a", "b"]), "numbers"),
    (dict(curve=[0, 2]), "curve"), (dict(curve=[0.0, 1.0]), "curve"), (dict(curve=[0]), "curve")]


@pytest.mark.parametrize("kw, match", BAD)
def test_survey_call_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    args = dict(dict(period=[1.0, 1.5], T0=[1.2, 1.3], duration=[0.1, 0.1]), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.shape_fit(T, flux, **args)
        with pytest.raises(ValueError, match=match):              # (nor is anything detrended first)
            survey.shape_fit(T, flux, detrend=25, **args)


def test_survey_call_checks_the_rows_and_reaches_the_device(no_device):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="flux_batch must be"):
            survey.shape_fit(T, flux[:, :-1], [1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
        with pytest.raises(ValueError, match="one candidate a light curve"):
            survey.shape_fit(T, flux, [1.0], [1.2], [0.1])
        with pytest.raises(ValueError, match="non-decreasing"):
            survey.shape_fit(T[::-1], flux, [1.0, 1.5], [1.2, 1.3], [0.1, 0.1])
        with pytest.raises(AssertionError, match="a context was created"):     # (a good call reaches the device)
            survey.shape_fit(T, flux, [1.0, numpy.nan], [1.2, 1.3], [0.1, -1.0])
        with pytest.raises(AssertionError, match="a context was created"):     # (a window that just holds the model)
            survey.shape_fit(T, flux, [1.0, 1.5], [1.2, 1.3], [0.1, 0.1], window=1.25)


@pytest.mark.parametrize("kw, match", [
    (dict(shape_fit=True), "needs peak_fits"), (dict(shape_fit=True, peaks=3), "needs peak_fits"),
    (dict(shape_fit=True, peaks=3, peak_fits=True, shape_fit_window=1.0), "window"),
    (dict(shape_fit=True, peaks=3, peak_fits=True, shape_fit_window=numpy.nan), "window"),
    (dict(shape_fit=True, peaks=3, peak_fits=True, shape_fit_min_count=0), "min_count")])
def test_power_batch_refuses_before_any_device_work(no_device, kw, match):
    flux = 1 + numpy.random.RandomState(0).normal(0, 1e-3, (2, len(T)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, **kw)
        with pytest.raises(ValueError, match=match):
            survey.power_batch(T, flux, detrend=25, **kw)


GOOD = dict(t=T, y=numpy.ones(300), dy=numpy.ones(300), period=[1.0, 2.0], T0=[1.1, 1.2], duration=[0.1, 0.2], ratios=[0.5, 1.0],
            ingress=[0.0, 0.5], shifts=[0.0], curve=[0, 0])


@pytest.mark.parametrize("kw", [
    dict(curve=[0, 1]), dict(curve=[-1, 0]), dict(curve=None), dict(T0=[1.0]), dict(duration=[[0.1, 0.2]]), dict(t=T[::-1]),
    dict(t=numpy.where(numpy.arange(300) == 7, numpy.nan, T)), dict(dy=numpy.zeros(300)), dict(y=numpy.full(300, numpy.nan)),
    dict(y=numpy.ones(299)), dict(ingress=[0.0, 0.25]), dict(window=0.4), dict(min_count=0), dict(depth_min=-1.0)])
def test_shape_fit_arguments_refuses(kw):
    with pytest.raises(ValueError, match="^shape fit: "):
        _lib.shape_fit_arguments(**dict(GOOD, **kw))


def test_shape_fit_arguments_packs():
    a = _lib.shape_fit_arguments(**dict(GOOD, period=[numpy.nan, -2.0]))      # (any candidate value: the device says status 1)
    assert a["y"].shape == a["dy"].shape == (1, 300) and a["curve"].dtype == numpy.int64 and a["curve"].tolist() == [0, 0]
    assert a["ratio"].tolist() == [0.5, 1.0] and a["ingress"].tolist() == [0.0, 0.5] and a["shift"].tolist() == [0.0]
    assert (a["window"], a["min_count"], a["depth_min"]) == (2.0, 3, 0.0)
    assert all(a[k].flags.c_contiguous and a[k].dtype == numpy.float64 for k in ("t", "y", "dy", "period", "T0", "duration"))
    one = _lib.shape_fit_arguments(T, numpy.ones((2, 300)), numpy.ones((2, 300)), [1.0, 2.0], [1.1, 1.2], [0.1, 0.2], [1.0],
                                   [0.0, 0.5], [0.0])
    assert one["curve"].tolist() == [0, 1]


def test_the_host_formed_fields():
    raw = numpy.zeros(3, dtype=_lib.SHAPE_DTYPE)
    raw["status"] = [0.0, 0.0, 1.0]
    raw["ses"], raw["ses_vee"] = [10.0, 8.0, numpy.nan], [6.0, numpy.nan, numpy.nan]
    t14, t23 = contacts(3.7, 0.07, 12, 0.1)
    raw["depth"], raw["duration"], raw["ingress"] = 0.07 ** 2, t14, (1.0 - t23 / t14) / 2.0
    out = survey._with_shapes(None, raw, numpy.array([3.7, 3.7, numpy.nan]))
    assert out.dtype.names == survey.shape_fit_fields()
    assert out["shape_delta_chi2"][0] == 64.0 and numpy.isnan(out["shape_delta_chi2"][1:]).all()
    assert abs(out["shape_impact"][0] - 0.1) < 1e-9 and abs(out["shape_a_rs"][1] - 12) < 1e-8
    assert numpy.isnan(out["shape_rho_star"][2]) and same(out["shape_ses"], raw["ses"])
