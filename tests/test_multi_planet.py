"""The multi-planet search on the device: tls_remove_transits equals its statement (tests/remove_transits_spec.py) bit for bit
-- rows, model and status -- on every path of the kernel (no candidate, one, two that coincide, a grazing one, a skipped one
in front of a valid one; one and five sub-exposures; a profile row of 65 and of 1025 doubles; 40 epochs; Julian dates; a row
of two tiles and of six), behind poisoned LDS and a larger call; every pass of power_batch_multi is power_batch on the
remove_transits rows; and the two planets of the measured set-up come back, the single one alone, and nothing from noise."""
import numpy
import pytest

import multi_planet_cases as cases
import remove_transits_spec as spec
from conftest import oracle_search
from tls_amd import survey
from tls_amd.planning import search_inputs

pytestmark = pytest.mark.gpu


def same(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.uint64), b.view(numpy.uint64))


def device(gpu, a):
    return gpu.remove_transits(a["t"], a["y"], a["P"], a["T0"], a["row"], a["A"], a["b"], a["T"], a["c0"], a["k_rows"],
                               a["profile"], a["sub"], curve=a["curve"], return_model=True, return_status=True)


def check(gpu, a):
    want = spec.remove_transits(**a)
    got = device(gpu, a)
    assert want[2].tolist() == [0, 0, 0, 0, 1, 0]
    for c in (1, 2, 3, 4):
        assert 0 < (want[1][c] != 1.0).sum() < a["y"].shape[1]
    for name, g, w in zip(("rows", "model", "status"), got, want):
        assert same(g, w), (name, numpy.argwhere(numpy.asarray(g) != numpy.asarray(w))[:5])
    assert same(got[0][0], a["y"][0])
    assert gpu.last_kernel() == "tls_remove_transits"


@pytest.mark.parametrize("n, M, S, offset, many", [
    (257, 64, 1, 0.0, False), (257, 64, 5, 2457000.0, True), (257, 1024, 1, 0.0, True), (257, 1024, 5, 0.0, False),
    (1440, 64, 1, 2457000.0, False), (1440, 64, 5, 0.0, True), (1440, 1024, 1, 0.0, True), (1440, 1024, 5, 2457000.0, False)])
def test_remove_transits_equals_the_statement(gpu, n, M, S, offset, many):
    check(gpu, cases.layout(n, M, S, offset, many))


def test_behind_poisoned_lds_and_a_larger_call(gpu):
    check(gpu, cases.layout(1440, 1024, 5))
    gpu.poison_lds()
    check(gpu, cases.layout(257, 64, 1))
    check(gpu, cases.layout(257, 64, 5, many_epochs=True))


def test_no_candidate_and_all_skipped_copy_the_rows(gpu):
    a = cases.layout(257, 64, 1)
    none = {k: (v[:0] if k in ("curve", "P", "T0", "row", "A", "b", "T", "c0") else v) for k, v in a.items()}
    rows, model, status = device(gpu, none)
    assert same(rows, a["y"]) and numpy.all(model == 1.0) and len(status) == 0
    skipped = dict(a, A=numpy.full(len(a["A"]), numpy.nan))
    rows, model, status = device(gpu, skipped)
    assert same(rows, a["y"]) and numpy.all(model == 1.0) and numpy.all(status == 1.0)


def test_the_survey_call_takes_a_peaks_array(gpu):
    """survey.remove_transits on planets [n_curves, K] equals the statement on the flattened candidates."""
    a = cases.layout(257, 1024, 5)
    k_rows, table = cases.profile()
    planets = numpy.zeros((5, 2), dtype=[(k, "f8") for k in ("period", "T0", "fit_row", "fit_amplitude", "fit_b", "fit_duration",
                                                              "fit_shift")])
    for k in planets.dtype.names:
        planets[k] = numpy.nan
    slots = [(1, 0), (2, 0), (2, 1), (3, 0), (4, 0), (4, 1)]
    for f, at in enumerate(slots):
        for k, v in zip(planets.dtype.names, (a["P"][f], a["T0"][f], 40.0 + f, a["A"][f], 0.2 * f, a["T"][f], a["c0"][f])):
            planets[k][at] = v
    flat = planets.reshape(-1)
    with numpy.errstate(all="ignore"):
        row = numpy.where(numpy.isfinite(flat["fit_row"]), flat["fit_row"], 0).astype(numpy.int64)
    sub = survey._transit_fit_setup(a["t"], None, None, None, None, 5, 1.0, 3, 1.0, (k_rows, table), {})["sub"]
    want = spec.remove_transits(a["t"], a["y"], numpy.repeat(numpy.arange(5), 2), flat["period"], flat["T0"], row,
                                flat["fit_amplitude"], flat["fit_b"], flat["fit_duration"], flat["fit_shift"], k_rows, table, sub)
    got = survey.remove_transits(a["t"], a["y"], planets, profile=(k_rows, table), return_model=True, return_status=True,
                                 context=gpu)
    assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2].reshape(-1), want[2])
    assert want[2].reshape(5, 2).tolist() == [[1, 1], [0, 1], [0, 0], [0, 1], [1, 0]]


def test_c_entry_arguments(gpu):
    """Every TLS_E_ARG case returns before any device work with the outputs untouched; n_fits == 0 copies the rows; curve NULL
    takes candidate f for curve f; out_model may be NULL; out_rows may be y itself."""
    from tls_amd import _lib
    lib, dp, ip = gpu._lib, _lib._dp, _lib._ip
    a = cases.layout(257, 64, 5)
    n, k_rows, table = 257, a["k_rows"], a["profile"]
    good = dict(t=a["t"], y=a["y"], n_curves=5, curve=a["curve"], period=a["P"], T0=a["T0"], row=a["row"], amplitude=a["A"],
                b=a["b"], duration=a["T"], shift=a["c0"], n_fits=6, k_rows=k_rows, profile=table, M=64, sub=a["sub"])
    rows, model, status = numpy.full((5, n), -7.0), numpy.full((5, n), -7.0), numpy.full(6, -7.0)

    def call(with_model=True, out=None, **kw):
        c = dict(good, **kw)
        f8 = {k: _lib._f8(c[k]) for k in ("t", "y", "period", "T0", "amplitude", "b", "duration", "shift", "k_rows", "profile", "sub")}
        curve, row = None if c["curve"] is None else _lib._i8(c["curve"]), _lib._i8(c["row"])
        return lib.tls_remove_transits(
            gpu._h, dp(f8["t"]), dp(f8["y"]) if out is None else dp(out), len(f8["t"]), c["n_curves"],
            None if curve is None else ip(curve), dp(f8["period"]), dp(f8["T0"]), ip(row), dp(f8["amplitude"]), dp(f8["b"]),
            dp(f8["duration"]), dp(f8["shift"]), c["n_fits"], dp(f8["k_rows"]), dp(f8["profile"]), len(f8["k_rows"]), c["M"],
            dp(f8["sub"]), len(f8["sub"]), dp(rows) if out is None else dp(out), dp(model) if with_model else None, dp(status))

    def untouched():
        return bool((rows == -7.0).all() and (model == -7.0).all() and (status == -7.0).all())

    late, nan = a["t"].copy(), numpy.nan
    late[100] = late[99] - 0.01
    bad_t = a["t"].copy()
    bad_t[5] = nan
    bad_profile = table.copy()
    bad_profile[3, 4] = nan
    row_of = lambda f, v: numpy.where(numpy.arange(6) == f, v, a["row"])
    curve_of = lambda f, v: numpy.where(numpy.arange(6) == f, v, a["curve"])
    for kw in (dict(curve=curve_of(2, 5)), dict(curve=curve_of(0, -1)), dict(row=row_of(1, -1)), dict(row=row_of(5, len(k_rows))),
               dict(curve=None), dict(sub=[nan]), dict(sub=[]), dict(sub=numpy.zeros(17)), dict(M=0), dict(M=4097),
               dict(k_rows=-k_rows[::-1]), dict(k_rows=k_rows[::-1]), dict(profile=bad_profile), dict(t=late), dict(t=bad_t),
               dict(n_fits=-1), dict(n_curves=-1)):
        assert call(**kw) == -1, kw                  # TLS_E_ARG
        assert untouched(), kw
        assert b"remove transits" in lib.tls_last_error(gpu._h), kw
    want = spec.remove_transits(**a)
    assert call(n_fits=0) == 0 and same(rows, a["y"]) and numpy.all(model == 1.0) and numpy.all(status == -7.0)
    assert call() == 0 and same(rows, want[0]) and same(model, want[1]) and same(status, want[2])
    model[:] = -7.0
    assert call(with_model=False) == 0 and same(rows, want[0]) and numpy.all(model == -7.0)
    in_place = a["y"].copy()
    assert call(out=in_place) == 0 and same(in_place, want[0])
    first = {k: (v[:1] if k in ("curve", "P", "T0", "row", "A", "b", "T", "c0") else v) for k, v in a.items()}
    one = spec.remove_transits(**dict(first, curve=None))                     # (curve NULL: candidate 0 on curve 0)
    assert call(curve=None, n_fits=1) == 0 and same(rows, one[0]) and not same(rows[0], a["y"][0])


# ---- the flow ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def curves():
    return cases.batch()


def _records_equal(planets, idx, j, out):
    summary, peaks = out[0], out[-1]["peaks"][:, 0]
    for k in summary.dtype.names:
        name = "summary_" + k if k in ("period", "T0", "depth", "duration") else k
        assert planets[name][idx, j].tobytes() == summary[k].tobytes(), (j, k)
    for k in peaks.dtype.names:
        assert planets[k][idx, j].tobytes() == numpy.ascontiguousarray(peaks[k]).tobytes(), (j, k)


@pytest.mark.parametrize("devices", [None, [0]])
def test_every_pass_is_power_batch_on_the_removed_rows(curves, devices):
    """n = 1440: the time stamps start at day 1 (a time stamp 0 is no valid point of a batched search)."""
    t, raw = 1.0 + cases.T, curves[:6]
    planets, info = survey.power_batch_multi(t, raw, 9.0, n_planets=3, devices=devices, return_rows=True, **cases.SEARCH)
    assert planets.shape == (6, 3) and len(info["searched"]) == 3
    assert info["searched"][0].tolist() == [0, 1, 2, 3, 4, 5]
    for j in (0, 1):                                 # (only the curves with an accepted pick go on)
        idx = info["searched"][j]
        assert info["searched"][j + 1].tolist() == idx[planets["pass_status"][idx, j] == survey.PLANET_ACCEPTED].tolist()
    assert len(info["searched"][1]) >= 3 and len(info["searched"][2]) >= 3
    for j, idx in enumerate(info["searched"]):
        rows = raw[idx] if j == 0 else survey.remove_transits(t, raw[idx], planets[idx, :j])
        out = survey.power_batch(t, rows, peaks=1, peak_fits=True, transit_fit=True, **cases.SEARCH)
        _records_equal(planets, idx, j, out)
        rest = numpy.setdiff1d(numpy.arange(6), idx)
        assert numpy.all(planets["pass_status"][rest, j] == survey.PLANET_NOT_REACHED)
        assert numpy.all(numpy.isnan(planets["SDE"][rest, j])) and numpy.all(planets["index"][rest, j] == -1)
    assert info["n_found"].tolist() == [2, 2, 2, 1, 0, 0]
    accepted = planets.copy()
    accepted["fit_amplitude"][planets["pass_status"] != 0] = numpy.nan
    assert same(info["rows"], survey.remove_transits(t, raw, accepted))
    assert same(info["rows"][4:], raw[4:]) and not same(info["rows"][3], raw[3])


def test_protect_factor_masks_the_planets_found_in_the_detrending(curves):
    """With a detrender and protect_factor, pass j + 1 is power_batch(detrend=, detrend_mask=transit_mask of the accepted
    planets) on the remove_transits rows; pass 0 has no mask."""
    t, raw, detrend = 1.0 + cases.T, curves[:4], survey.Biweight(0.75)
    planets, info = survey.power_batch_multi(t, raw, 9.0, n_planets=2, detrend=detrend, protect_factor=1.5, **cases.SEARCH)
    assert info["searched"][0].tolist() == [0, 1, 2, 3] and len(info["searched"][1]) >= 3
    idx = info["searched"][1]
    assert idx.tolist() == numpy.nonzero(planets["pass_status"][:, 0] == survey.PLANET_ACCEPTED)[0].tolist()
    out = survey.power_batch(t, raw, detrend=detrend, peaks=1, peak_fits=True, transit_fit=True, **cases.SEARCH)
    _records_equal(planets, numpy.arange(4), 0, out)
    found = planets[idx, :1]
    mask = survey.transit_mask(t, found["period"][:, 0], found["T0"][:, 0], found["duration_days"][:, 0], factor=1.5)
    assert mask.shape == (len(idx), len(t)) and 0 < mask.mean() < 0.2
    rows = survey.remove_transits(t, raw[idx], found)
    out = survey.power_batch(t, rows, detrend=detrend, detrend_mask=mask, peaks=1, peak_fits=True, transit_fit=True, **cases.SEARCH)
    _records_equal(planets, idx, 1, out)
    with pytest.raises(ValueError, match="median filter"):
        survey.power_batch_multi(t, raw, 9.0, detrend=25, protect_factor=1.5, **cases.SEARCH)


def test_recovery(curves, oracle_lib):
    """The measured set-up on the 1439 points power() keeps of it (it drops the time stamp 0)."""
    t, curves = cases.T[1:], curves[:, 1:]
    planets, info = survey.power_batch_multi(t, curves, sde_min=9, n_planets=3, **cases.SEARCH)
    print("SDE by pass:\n", numpy.round(planets["SDE"], 2), "\nperiod by pass:\n", numpy.round(planets["period"], 4))
    assert info["n_found"].tolist() == [2, 2, 2, 1, 0, 0, 0, 0]
    for c in (0, 1, 2):
        assert planets["pass_status"][c].tolist() in ([0, 0, 2], [0, 0, 4])
        assert abs(planets["period"][c, 0] - 2.1) <= 0.01 * 2.1 and abs(planets["period"][c, 1] - 3.7) <= 0.01 * 3.7
    assert planets["pass_status"][3].tolist() in ([0, 2, 1], [0, 4, 1]) and abs(planets["period"][3, 0] - 2.1) <= 0.01 * 2.1
    assert numpy.all(planets["pass_status"][4:, 0] == survey.PLANET_BELOW_SDE)
    assert numpy.all(planets["pass_status"][4:, 1:] == survey.PLANET_NOT_REACHED)
    # the device search agrees with the oracle to 1e-10 in chi^2 (the SDE nearest to the threshold 9 are 7.14 and 16.97)
    inp = search_inputs(t, curves[0], None, **cases.SEARCH)
    want = oracle_search(oracle_lib, inp)[0]
    got = survey.power_batch(t, curves[:1], with_arrays=True, **cases.SEARCH)[2][0]
    numpy.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
