"""Injection-recovery without a GPU: the tls_inject_transits declaration against its binding, a numpy mirror of the device's
per-point sequence against transit_model.light_curve (bit for bit), the recovery classification, T14, injection_grid,
completeness and the argument errors."""
import ctypes
import os
import re

import numpy
import pytest

from tls_amd import _lib, constants as C, survey, transit_model
from conftest import REPO

PI = numpy.pi


def _header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---- header and binding

def test_declaration_matches_argtypes():
    text = _header()
    m = re.search(r"int\s+tls_inject_transits\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "tls_inject_transits is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    c_types = {"tls_ctx *": ctypes.c_void_p, "double": ctypes.c_double, "int64_t": ctypes.c_int64,
               "const double *": _lib._c_double_p, "double *": _lib._c_double_p, "int64_t *": _lib._c_int64_p,
               "const tls_injection *": ctypes.POINTER(_lib.Injection)}
    want = []
    for p in params:
        ctype = re.match(r"(.*?)\s*\**\s*\w+$", p.replace("*", " * ")).group(0)
        ctype = " ".join(ctype.replace("*", " * ").split()[:-1]).replace(" *", " *")
        want.append(c_types[ctype.replace(" * ", " *").replace("* ", "*")])
    got = _lib.load().tls_inject_transits.argtypes
    assert len(got) == len(want) == 11
    assert list(got) == want
    assert _lib.load().tls_inject_transits.restype == ctypes.c_int


def test_injection_struct_matches_header():
    text = _header()
    m = re.search(r"typedef struct tls_injection\s*\{(.*?)\}\s*tls_injection;", text, flags=re.S)
    assert m
    names = [n.strip() for n in m.group(1).replace("double", "").replace(";", ",").split(",") if n.strip()]
    assert names == [k for k, _ in _lib.Injection._fields_] == list(_lib.INJECTION_FIELDS)
    assert all(t is ctypes.c_double for _, t in _lib.Injection._fields_)
    assert ctypes.sizeof(_lib.Injection) == 48 == _lib.INJECTION_DTYPE.itemsize


def test_abi_version_is_8():
    assert _lib.ABI_VERSION == 8
    assert _lib.load().tls_abi_version() == 8
    assert re.search(r"#define TLS_AMD_ABI_VERSION 8\b", open(os.path.join(REPO, "include", "tls_amd.h")).read())


# ---- a numpy mirror of the device's per-point sequence (tls_inject.hip.h), fed the host-formed constants

def _ek(k):
    return transit_model.ellip_k(k), transit_model.ellip_e(k)


def mirror_flux(z, p, u1, u2):
    """inj_quadratic_flux element by element (as masks): the device's case order and operation order."""
    z = numpy.abs(numpy.array(z, dtype=float))
    flux = numpy.ones_like(z)
    omega = 1.0 - u1 / 3.0 - u2 / 6.0
    c2 = u1 + 2.0 * u2
    z = numpy.where(numpy.abs(p - z) < 1e-14, p, z)
    z = numpy.where(numpy.abs(p - 1.0 - z) < 1e-14, p - 1.0, z)
    z = numpy.where(numpy.abs(1.0 - p - z) < 1e-14, 1.0 - p, z)
    z = numpy.where(z < 1e-14, 0.0, z)
    x1, x2, pp = (p - z) * (p - z), (p + z) * (p + z), p * p
    x3 = pp - z * z
    todo = z < 1.0 + p
    lam_e, lam_d, eta_d, kap0, kap1 = (numpy.zeros_like(z) for _ in range(5))
    with numpy.errstate(all="ignore"):
        if p >= 1.0:
            m = todo & (z <= p - 1.0)
            flux[m] = 1.0 - ((1.0 - c2) + c2 * (2.0 / 3.0) + u2 * 0.5) / omega
            todo &= ~m
        m = todo & (z >= abs(1.0 - p)) & (z <= 1.0 + p)
        zz = z[m]
        kap1[m] = numpy.arccos(numpy.minimum((1.0 - pp + zz * zz) / 2.0 / zz, 1.0))
        kap0[m] = numpy.arccos(numpy.minimum((pp + zz * zz - 1.0) / 2.0 / p / zz, 1.0))
        r = 1.0 + zz * zz - pp
        lam_e[m] = (pp * kap0[m] + kap1[m] - 0.5 * numpy.sqrt(numpy.maximum(4.0 * zz * zz - r * r, 0.0))) / PI
        m = todo & (z == p)
        if m.any():
            zz = z[m]
            if p < 0.5:
                q = 2.0 * p
                E, K = transit_model.ellip_e(q), transit_model.ellip_k(q)
                lam_d[m] = 1.0 / 3.0 + 2.0 / 9.0 / PI * (4.0 * (2.0 * p * p - 1.0) * E + (1.0 - 4.0 * p * p) * K)
                eta_d[m] = pp / 2.0 * (pp + 2.0 * zz * zz)
                lam_e[m] = pp
            elif p > 0.5:
                q = 0.5 / p
                E, K = transit_model.ellip_e(q), transit_model.ellip_k(q)
                lam_d[m] = 1.0 / 3.0 + 16.0 * p / 9.0 / PI * (2.0 * p * p - 1.0) * E \
                    - (32.0 * p ** 4 - 20.0 * p * p + 3.0) / 9.0 / PI / p * K
                zsq = zz * zz
                eta_d[m] = 0.5 / PI * (kap1[m] + pp * (pp + 2.0 * zsq) * kap0[m]
                                       - (1.0 + 5.0 * p * p + zsq) / 4.0 * numpy.sqrt((1.0 - x1[m]) * (x2[m] - 1.0)))
            else:
                lam_d[m] = 1.0 / 3.0 - 4.0 / PI / 9.0
                eta_d[m] = 3.0 / 32.0
            flux[m] = 1.0 - ((1.0 - c2) * lam_e[m] + c2 * lam_d[m] + u2 * eta_d[m]) / omega
            todo &= ~m
        m = todo & (((z > 0.5 + abs(p - 0.5)) & (z < 1.0 + p)) | ((p > 0.5) & (z > abs(1.0 - p) * 1.0001) & (z < p)))
        if m.any():
            zz, a1, a2, a3 = z[m], x1[m], x2[m], x3[m]
            q = numpy.sqrt((1.0 - a1) / (a2 - a1))
            K, E = _ek(q)
            P = transit_model.ellip_pi(1.0 / a1 - 1.0, q)
            ld = 1.0 / 9.0 / PI / numpy.sqrt(p * zz) * (((1.0 - a2) * (2.0 * a2 + a1 - 3.0) - 3.0 * a3 * (a2 - 2.0)) * K
                                                       + 4.0 * p * zz * (zz * zz + 7.0 * p * p - 4.0) * E - 3.0 * a3 / a1 * P)
            eta = 1.0 / 2.0 / PI * (kap1[m] + pp * (pp + 2.0 * zz * zz) * kap0[m]
                                    - (1.0 + 5.0 * p * p + zz * zz) / 4.0 * numpy.sqrt((1.0 - a1) * (a2 - 1.0)))
            ld = ld + numpy.where(p > zz, 2.0 / 3.0, 0.0)
            flux[m] = 1.0 - ((1.0 - c2) * lam_e[m] + c2 * ld + u2 * eta) / omega
            todo &= ~m
        if p <= 1.0:
            m = todo & (z <= 1.0 - p)
            zz, a1, a2, a3 = z[m], x1[m], x2[m], x3[m]
            eta = pp / 2.0 * (pp + 2.0 * zz * zz)
            q = numpy.sqrt((a2 - a1) / (1.0 - a1))
            K, E = _ek(q)
            P = transit_model.ellip_pi(a2 / a1 - 1.0, q)
            ld = 2.0 / 9.0 / PI / numpy.sqrt(1.0 - a1) * ((1.0 - 5.0 * zz * zz + pp + a3 * a3) * K
                                                          + (1.0 - a1) * (zz * zz + 7.0 * p * p - 4.0) * E - 3.0 * a3 / a1 * P)
            touch = numpy.abs(p + zz - 1.0) <= 1e-14
            ld = numpy.where(touch, 2.0 / 3.0 / PI * numpy.arccos(1.0 - 2.0 * p)
                             - 4.0 / 9.0 / PI * numpy.sqrt(p * (1.0 - p)) * (3.0 + 2.0 * p - 8.0 * p * p), ld)
            ld = numpy.where(zz == 0.0, -2.0 / 3.0 * (1.0 - pp) ** 1.5, ld)
            flux[m] = 1.0 - ((1.0 - c2) * p * p + c2 * (ld + numpy.where(p > zz, 2.0 / 3.0, 0.0)) + u2 * eta) / omega
    return flux


def mirror_inject(t, flux, c, u1, u2):
    """tls_inject_transits on the host: (rows, n_in_transit) from INJECTION_DTYPE constants."""
    rows = numpy.empty((len(c), len(t)))
    count = numpy.zeros(len(c), dtype=numpy.int64)
    for k in range(len(c)):
        tp, per, p, a, sin_inc, omega = (float(c[f][k]) for f in _lib.INJECTION_FIELDS)
        x = (t - tp) / per
        f = (x - numpy.trunc(x)) * 2.0 * PI
        s = numpy.sin(f + omega) * sin_inc
        z = numpy.where(s <= 0.0, 1e10, a * numpy.sqrt(numpy.maximum(1.0 - s * s, 0.0)))
        zs = numpy.where(numpy.abs(p - z) < 1e-14, p, z)
        zs = numpy.where(numpy.abs(p - 1.0 - zs) < 1e-14, p - 1.0, zs)
        zs = numpy.where(numpy.abs(1.0 - p - zs) < 1e-14, 1.0 - p, zs)
        zs = numpy.where(zs < 1e-14, 0.0, zs)
        contact = zs < 1.0 + p
        count[k] = int(contact.sum())
        base = flux if flux.ndim == 1 else flux[k]
        row = base.copy()
        row[contact] = base[contact] * mirror_flux(z[contact], p, u1, u2)
        rows[k] = row
    return rows, count


def random_injections(rng, t, n_inj, rp_lo=0.002, rp_hi=0.3):
    """Random circular injections: rp in [rp_lo, rp_hi], b in [0, 1 + rp + 0.1] (grazing and non-transiting ones)."""
    P = rng.uniform(0.7, 25.0, n_inj)
    rp = rng.uniform(rp_lo, rp_hi, n_inj)
    a = rng.uniform(3.0, 40.0, n_inj)
    b = rng.uniform(0.0, 1.0 + rp + 0.1)
    inc = numpy.degrees(numpy.arccos(numpy.minimum(b / a, 1.0)))
    T0 = numpy.min(t) + rng.uniform(-1.0, 1.0, n_inj) * P
    return dict(T0=T0, period=P, rp_rs=rp, a=a, inc=inc)


def host_rows(t, flux, inj, u, law):
    out = numpy.empty((len(inj["T0"]), len(t)))
    for k in range(len(out)):
        base = flux if flux.ndim == 1 else flux[k]
        out[k] = base * transit_model.light_curve(t, float(inj["T0"][k]), float(inj["period"][k]), float(inj["rp_rs"][k]),
                                                  float(inj["a"][k]), float(inj["inc"][k]), 0, 90, u, law)
    return out


@pytest.mark.parametrize("law,u", [("quadratic", [0.4804, 0.1867]), ("linear", [0.55]), ("uniform", [])])
def test_mirror_equals_light_curve_bit_for_bit(law, u):
    rng = numpy.random.RandomState(11)
    t = numpy.sort(numpy.concatenate([numpy.linspace(3.0, 40.0, 1500), rng.uniform(3.0, 40.0, 300)]))
    flux = 1.0 + rng.normal(0.0, 1e-4, len(t))
    inj = random_injections(rng, t, 60)
    # dense in-transit sampling of a few long transits too
    _, u1, u2 = survey._injection_law(u, law, {})
    c = survey.injection_constants(inj)
    rows, count = mirror_inject(t, flux, c, u1, u2)
    want = host_rows(t, flux, inj, u if law != "uniform" else None, law)
    numpy.testing.assert_array_equal(rows, want)
    assert numpy.any(count > 0) and numpy.any(count == 0)


def test_mirror_reaches_every_case():
    """Separations placed on z = 0, p, 1 - p, 1 + p and in between, p = 0.5 and the fully covered p = 1.2."""
    for p in (0.05, 0.3, 0.5, 0.7, 1.0, 1.2):
        z = numpy.unique(numpy.concatenate([[0.0, p, abs(1.0 - p), 1.0 + p, max(p - 1.0, 0.0)],
                                            numpy.linspace(0.0, 1.0 + p + 0.05, 501)]))
        got = mirror_flux(z, p, 0.4, 0.25)
        want = transit_model.quadratic_ld_flux(z, p, 0.4, 0.25)
        numpy.testing.assert_array_equal(got, want)


# ---- classification

def _summary(period, T0, SDE, no_fit=0):
    s = numpy.zeros(len(numpy.atleast_1d(period)), dtype=[("period", "f8"), ("T0", "f8"), ("SDE", "f8"), ("no_fit", "i8")])
    s["period"], s["T0"], s["SDE"], s["no_fit"] = period, T0, SDE, no_fit
    return s


INJ = dict(T0=[10.0], period=[5.0], rp_rs=[0.05], a=[15.0], inc=[90.0])


def _classify(period, T0, SDE=20.0, no_fit=0, **kw):
    return survey.classify_recovery(INJ, _summary(period, T0, SDE, no_fit), [100], **kw)[0]


def test_classification_exact_match():
    r = _classify(5.0, 10.0)
    assert r["recovered"] and r["period_match"] == 1.0 and r["epoch_offset"] == 0.0 and r["n_in_transit"] == 100


def test_classification_double_period_alias_only_when_listed():
    r = _classify(10.0, 15.0)
    assert not r["recovered"] and r["period_match"] == 0.0 and numpy.isnan(r["epoch_offset"])
    r = _classify(10.0, 15.0, aliases=(1.0, 2.0))
    assert r["recovered"] and r["period_match"] == 2.0 and r["epoch_offset"] == 0.0


def test_classification_half_period_alias_with_half_period_epoch():
    r = _classify(2.5, 12.5, aliases=(1.0, 0.5))
    assert r["recovered"] and r["period_match"] == 0.5 and r["epoch_offset"] == 0.0
    assert not _classify(2.5, 12.5)["recovered"]


def test_classification_epoch_one_period_later_and_earlier():
    for T0 in (15.0, 5.0, 35.0):
        r = _classify(5.0, T0)
        assert r["recovered"] and abs(r["epoch_offset"]) < 1e-12


def test_classification_tolerance_edges():
    T14 = survey.injected_duration(INJ)[0]
    assert _classify(5.0 * 1.01, 10.0)["period_match"] == 1.0          # |dP| == 0.01 P: inside
    assert _classify(5.0 * 1.0101, 10.0)["period_match"] == 0.0
    assert _classify(5.0, 10.0 + 0.5 * T14)["recovered"]
    assert not _classify(5.0, 10.0 + 0.5 * T14 * 1.001)["recovered"]
    assert not _classify(5.0, 10.0 - 0.5 * T14 * 1.001)["recovered"]
    assert _classify(5.0, 10.2, epoch_tolerance=0.2)["recovered"]
    assert not _classify(5.0, 10.2001, epoch_tolerance=0.2)["recovered"]
    assert _classify(5.1, 10.0, period_tolerance=0.02)["recovered"]


def test_classification_sde_threshold_and_no_fit():
    assert _classify(5.0, 10.0, SDE=7.0)["recovered"]
    assert not _classify(5.0, 10.0, SDE=numpy.nextafter(7.0, 0.0))["recovered"]
    assert _classify(5.0, 10.0, SDE=6.0, sde_threshold=5.0)["recovered"]
    r = _classify(numpy.nan, numpy.nan, SDE=0.0, no_fit=1)
    assert not r["recovered"] and r["period_match"] == 0.0
    assert not _classify(5.0, 10.0, SDE=50.0, no_fit=1)["recovered"]


def test_t14_against_dense_host_model():
    for rp, a, inc in ((0.05, 15.0, 90.0), (0.1, 20.0, 88.0), (0.02, 8.0, 85.0), (0.2, 12.0, 85.5)):
        P = 7.0
        t = numpy.linspace(-0.5, 0.5, 400001)
        f = transit_model.light_curve(t, 0.0, P, rp, a, inc, 0, 90, [0.4, 0.2], "quadratic")
        dt = t[1] - t[0]
        inside = t[f < 1.0]
        width = inside[-1] - inside[0] + dt
        T14 = survey.injected_duration(dict(T0=[0.0], period=[P], rp_rs=[rp], a=[a], inc=[inc]))[0]
        assert abs(width - T14) <= 2 * dt, (rp, a, inc, width, T14)
    # no transit at all: T14 = 0
    assert survey.injected_duration(dict(T0=[0.0], period=[5.0], rp_rs=[0.1], a=[10.0], inc=[80.0]))[0] == 0.0


# ---- injection_grid and completeness

def test_injection_grid_deterministic_and_kepler():
    t = numpy.linspace(2.0, 92.0, 4320)
    state = numpy.random.get_state()
    g1 = survey.injection_grid(t, [3.0, 10.0], [0.02, 0.05, 0.1], per_cell=4, b_max=0.6, seed=5)
    g2 = survey.injection_grid(t, [3.0, 10.0], [0.02, 0.05, 0.1], per_cell=4, b_max=0.6, seed=5)
    g3 = survey.injection_grid(t, [3.0, 10.0], [0.02, 0.05, 0.1], per_cell=4, b_max=0.6, seed=6)
    after = numpy.random.get_state()
    assert after[0] == state[0] and numpy.array_equal(after[1], state[1]) and after[2:] == state[2:]
    assert numpy.array_equal(g1, g2) and not numpy.array_equal(g1["T0"], g3["T0"])
    assert len(g1) == 2 * 3 * 4
    assert list(g1["period"][:12]) == [3.0] * 12 and list(g1["rp_rs"][:4]) == [0.02] * 4
    assert numpy.all((g1["T0"] >= 2.0) & (g1["T0"] < 2.0 + g1["period"]))
    P_s = g1["period"] * C.SECONDS_PER_DAY
    a = (C.G * C.M_sun * P_s ** 2 / (4 * numpy.pi ** 2)) ** (1 / 3) / C.R_sun
    numpy.testing.assert_allclose(g1["a"], a, rtol=1e-14)
    assert 19.4 < g1["a"][-1] < 19.7           # 10 d around a Sun: a/R* ~ 19.5
    b = g1["a"] * numpy.cos(numpy.radians(g1["inc"]))
    assert numpy.all((b >= -1e-12) & (b <= 0.6 + 1e-12)) and b.max() > 0.3
    flat = survey.injection_grid(t, [5.0], [0.1], per_cell=3)
    assert numpy.all(flat["inc"] == 90.0)
    big = survey.injection_grid(t, [5.0], [0.1], R_star=2.0, M_star=0.5)
    assert abs(big["a"][0] / survey.injection_grid(t, [5.0], [0.1])["a"][0] - 0.5 ** (1 / 3) / 2.0) < 1e-12


def test_completeness_counts():
    rec = numpy.zeros(6, dtype=[("period", "f8"), ("rp_rs", "f8"), ("n_in_transit", "i8"), ("recovered", "?")])
    rec["period"] = [2.0, 2.5, 2.2, 8.0, 8.0, 9.0]
    rec["rp_rs"] = [0.05, 0.05, 0.05, 0.15, 0.15, 0.05]
    rec["n_in_transit"] = [10, 10, 0, 5, 5, 7]
    rec["recovered"] = [True, False, True, True, True, False]
    frac, hit, total = survey.completeness(rec, [1.0, 5.0, 10.0], [0.0, 0.1, 0.2])
    assert total.tolist() == [[2, 0], [1, 2]] and hit.tolist() == [[1, 0], [0, 2]]
    assert frac[0, 0] == 0.5 and numpy.isnan(frac[0, 1]) and frac[1, 1] == 1.0 and frac[1, 0] == 0.0
    frac, hit, total = survey.completeness(rec, [1.0, 5.0, 10.0], [0.0, 0.1, 0.2], exclude_untransiting=False)
    assert total.tolist() == [[3, 0], [1, 2]] and hit.tolist() == [[2, 0], [0, 2]]


# ---- argument errors (raised before any device work)

def test_argument_errors():
    t = numpy.linspace(0.0, 30.0, 500)
    f = numpy.ones(500)
    good = dict(T0=[1.0], period=[3.0], rp_rs=[0.05], a=[10.0], inc=[90.0])
    ctx = object()   # (never reached)
    with pytest.raises(ValueError, match="closed form"):
        survey.injection_recovery(t, f, good, inject_limb_dark="nonlinear", context=ctx)
    with pytest.raises(ValueError, match="closed form"):
        survey.injection_recovery(t, f, good, limb_dark="squareroot", context=ctx)
    with pytest.raises(ValueError, match="circular"):
        survey.injection_recovery(t, f, dict(good, ecc=[0.1]), context=ctx)
    with pytest.raises(ValueError, match="circular"):
        survey.injection_recovery(t, f, dict(good, w=[80.0]), context=ctx)
    with pytest.raises(ValueError, match="shape"):
        survey.injection_recovery(t, numpy.ones(499), good, context=ctx)
    with pytest.raises(ValueError, match="shape"):
        survey.injection_recovery(t, numpy.ones((2, 500)), good, context=ctx)
    with pytest.raises(ValueError, match="dy"):
        survey.injection_recovery(t, f, good, dy=numpy.ones(3), context=ctx)
    with pytest.raises(ValueError, match="rp_rs"):
        survey.injection_recovery(t, f, dict(good, rp_rs=[-0.01]), context=ctx)
    with pytest.raises(ValueError, match="period"):
        survey.injection_recovery(t, f, dict(good, period=[0.0]), context=ctx)
    with pytest.raises(ValueError, match="period"):
        survey.injection_recovery(t, f, dict(good, period=[-2.0]), context=ctx)
    with pytest.raises(ValueError, match="lack"):
        survey.injection_recovery(t, f, dict(T0=[1.0], period=[3.0]), context=ctx)
    with pytest.raises(ValueError, match="coefficients"):
        survey.injection_recovery(t, f, good, inject_u=[0.3], inject_limb_dark="quadratic", context=ctx)
    with pytest.raises(ValueError, match="aliases"):
        survey.injection_recovery(t, f, good, aliases=(0.0,), context=ctx)
