"""The drop-in API end to end on the GPU: tls_amd.transitleastsquares(...).power(...)
against golden results of the unmodified reference and the reference's own
known-answer tests (same checks as test_power_host.py, real HIP search)."""
import os
import warnings

import numpy
import pytest

import tls_amd
import pins
from tls_amd import synthetic, transit_model

pytestmark = pytest.mark.gpu


def make_model(t, y, dy):
    return tls_amd.transitleastsquares(t, y, dy, verbose=False)


@pytest.mark.parametrize("name", ["small", "weights", "nofit", "grazing", "box", "ecc"])
def test_power_matches_reference_golden(name):
    pins.check_power_golden(make_model, name)


def test_reference_pin_synthetic():
    pins.check_synthetic(make_model)


def test_reference_pin_transit_depth_min():
    pins.check_transit_depth_min(make_model)


def test_reference_pin_uncertainties():
    pins.check_uncertainties(make_model)


def test_reference_pin_stats_gap():
    pins.check_stats_gap(make_model)


def test_reference_pin_multi_planet():
    pins.check_multi_planet(make_model)


def test_reference_pin_shapes():
    pins.check_shapes(make_model)


def test_k2_90d_anchor_values():
    """SURVEY.md Appendix D, config 2 (shimmed reference + C inner loops)."""
    from tls_amd import synthetic
    t, f, kw = synthetic.config("k2_90d")
    r = make_model(t, f, None).power(verbose=False, show_progress_bar=False, **kw)
    assert len(r.periods) == 9679
    assert int(numpy.argmin(r.chi2)) == 7738 == int(numpy.argmax(r.power))
    numpy.testing.assert_allclose(r.chi2_min, 4101.6439079674, rtol=1e-10)
    numpy.testing.assert_allclose(numpy.sum(r.chi2), 41768414.394605, rtol=1e-10)
    numpy.testing.assert_allclose(r.period, 10.12452360, rtol=1e-8)
    numpy.testing.assert_allclose(r.T0, 13.25983524, rtol=1e-8)
    numpy.testing.assert_allclose(r.duration, 0.18549107, rtol=1e-7)
    numpy.testing.assert_allclose(r.depth, 0.99989805, rtol=1e-7)
    numpy.testing.assert_allclose(r.SDE, 25.71647715, rtol=1e-7)
    numpy.testing.assert_allclose(r.SDE_raw, 22.94488813, rtol=1e-7)
    numpy.testing.assert_allclose(r.rp_rs, 0.00908039, rtol=1e-6)
    numpy.testing.assert_allclose(r.snr, 14.324393, rtol=1e-6)
    assert len(r.transit_times) == 8


def _extra_seeds():   # TLS_FUZZ_SEEDS="100-140" adds seeds for a one-off longer sweep
    out = []
    for part in filter(None, os.environ.get("TLS_FUZZ_SEEDS", "").split(",")):
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3, 4] + _extra_seeds())
def test_power_gpu_equals_power_with_oracle_search(monkeypatch, oracle_lib, seed):
    """End to end on random small light curves: the drop-in with the HIP search and the device T0
    fit must return the same results object as the same host code fed by the CPU oracle's search
    and T0-fit loops (the combination that the reference's own known answers pin)."""
    from tls_amd import transit_model
    import warnings
    rng = numpy.random.RandomState(seed)
    span = float(rng.choice([15.0, 30.0, 60.0]))
    n = int(span * rng.choice([24, 48]))
    t = numpy.linspace(2.0, 2.0 + span, n)
    per = float(rng.uniform(2.0, span / 4))
    y = transit_model.light_curve(t, 2.5, per, float(rng.uniform(0.02, 0.07)), 12, 89.8, 0, 90,
                                  [0.4, 0.3], "quadratic") + rng.normal(0, 3e-4, n)
    dy = rng.uniform(0.8, 1.3, n) * 3e-4 if seed % 2 else None
    kwargs = dict(period_min=1.0, period_max=span / 3, oversampling_factor=2,
                  T0_fit_margin=float(rng.choice([0.01, 0.05])), verbose=False, show_progress_bar=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = make_model(t, y, dy).power(**kwargs)

        def oracle_search_periods(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                  M_star_min, M_star_max, T0_fit_margin, **_unused):
            return oracle_lib.search(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                     M_star_min, M_star_max, T0_fit_margin)[:3]

        monkeypatch.setattr(tls_amd.search, "spectra",
                            lambda chi2_, osf_, **kw: oracle_lib.spectra(chi2_, int(osf_ * 30)))
        monkeypatch.setattr(tls_amd.search, "search_periods", oracle_search_periods)
        monkeypatch.setattr(tls_amd.search, "t0_fit_residuals",
                            lambda t_, y_, p_, s_, e_, r_, **kw: oracle_lib.t0_residuals(t_, y_, p_, s_, e_, r_))
        want = make_model(t, y, dy).power(**kwargs)
    assert list(got.keys()) == list(want.keys())
    for key in pins.SCALARS:
        numpy.testing.assert_allclose(float(got[key]), float(want[key]), rtol=1e-9, atol=1e-12, err_msg=key)
    for key in pins.ARRAYS:
        # The spectra are (SR - mean SR) / std SR with std SR ~ 1e-3: a 1e-12 relative difference of chi^2 -- the
        # LDS-resident kernel's fast prefix-sum mode moves the depth scale of a cell by <= 2^-52 * N (DESIGN.md
        # section 3) -- arrives 1e3 times larger.  chi^2 itself is held to 1e-9 here and to 1e-9 against the oracle
        # on every configuration (tests/test_gpu_parity.py).
        atol = 2e-9 if key in ("power", "power_raw", "SR") else 1e-11
        numpy.testing.assert_allclose(numpy.asarray(got[key], dtype=float), numpy.asarray(want[key], dtype=float),
                                      rtol=1e-9, atol=atol, err_msg=key)
    assert int(numpy.argmin(got.chi2)) == int(numpy.argmin(want.chi2))


@pytest.mark.parametrize("weights", [False, True])
def test_power_batch_equals_power_per_curve_and_the_oracle(oracle_lib, weights):
    """Survey-mode power() (tls_power_batch: search + spectra + final T0 fit on the device, 80 bytes back per light
    curve) against (i) the drop-in power() of every light curve on its own -- which is pinned to the reference -- for
    12 seeds from three different 32-curve launch groups, (ii) the oracle: its search, its spectra and its T0-fit
    residuals fed the same way (main.py:198-283, stats.py:105-204)."""
    import tls_amd
    from tls_amd import survey, _lib
    ctx = _lib.Context(0)
    n_curves = 70
    t = numpy.linspace(3.0, 33.0, 720)
    rng = numpy.random.RandomState(11)
    fluxes, dys = [], []
    for s in range(n_curves):
        per = float(rng.uniform(2.0, 7.0))
        f = transit_model.light_curve(t, 3.2 + rng.uniform(0, 1), per, float(rng.uniform(0.03, 0.08)), 12, 89.8, 0, 90,
                                      [0.4, 0.3], "quadratic") + rng.normal(0, 4e-4, len(t))
        if s == 5:
            f = 1 + rng.normal(0, 1e-9, len(t)) * 0 + 0.0        # flat: nothing passes transit_depth_min
            f[::7] += 1e-7
        fluxes.append(f)
        dys.append(rng.uniform(0.8, 1.3, len(t)) * 4e-4)
    fluxes = numpy.array(fluxes)
    dy_batch = numpy.array(dys) if weights else None
    kw = dict(period_min=1.5, period_max=9.0, oversampling_factor=2, T0_fit_margin=0.02)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        summary, periods, chi2, row, depth, power = survey.power_batch(t, fluxes, dy_batch, context=ctx, with_arrays=True, **kw)
        assert len(summary) == n_curves
        for s in (0, 1, 5, 17, 31, 32, 33, 47, 63, 64, 65, 69):
            one = tls_amd.transitleastsquares(t, fluxes[s], None if dy_batch is None else dy_batch[s], verbose=False).power(
                context=ctx, verbose=False, show_progress_bar=False, **kw)
            rec = summary[s]
            numpy.testing.assert_array_equal(chi2[s], one.chi2)          # same kernel, same launch-group invariance
            assert rec["chi2_min"] == one.chi2_min
            if rec["no_fit"]:
                assert one.SDE == 0 and numpy.isnan(one.period) and one.depth == 1 and one.T0 == 0
                assert rec["SDE"] == 0 and numpy.isnan(rec["period"]) and rec["depth"] == 1 and rec["T0"] == 0
                continue
            assert rec["period"] == one.period and rec["depth"] == one.depth
            assert rec["T0"] == one.T0, (s, rec["T0"], one.T0)
            numpy.testing.assert_allclose([rec["SDE"], rec["SDE_raw"]], [one.SDE, one.SDE_raw], rtol=1e-12)
            numpy.testing.assert_allclose(power[s], one.power, rtol=1e-12, atol=1e-13)
            assert rec["index_best"] == int(numpy.argmin(one.chi2)) and rec["index_power"] == int(numpy.argmax(one.power))
            # the oracle, fed the way main.py:198-283 feeds its own pieces
            inp = synthetic.search_inputs(t, fluxes[s], None if dy_batch is None else dy_batch[s], **kw)
            p = inp["params"]
            o_chi2, o_row, o_depth, _ = oracle_lib.search(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"],
                                                          p["transit_depth_min"], p["R_star_min"], p["R_star_max"],
                                                          p["M_star_min"], p["M_star_max"], p["T0_fit_margin"])
            o_SR, o_praw, o_power, o_sde_raw, o_sde = oracle_lib.spectra(o_chi2, 60)
            assert int(numpy.argmin(o_chi2)) == rec["index_best"] and int(numpy.argmax(o_power)) == rec["index_power"]
            assert o_row[rec["index_best"]] == rec["best_row"]
            numpy.testing.assert_allclose([rec["SDE"], rec["SDE_raw"], rec["chi2_min"]], [o_sde, o_sde_raw, o_chi2.min()], rtol=1e-8)
            assert abs(rec["depth"] - o_depth[rec["index_power"]]) < 1e-11
            assert rec["duration"] == inp["overview"]["duration"][rec["best_row"]]
    ctx.close()


def test_power_at_tess_size_gpu_equals_power_with_oracle_search(oracle_lib, monkeypatch):
    """One whole power() call at the size of BASELINE config 4 (N = 19 440, 2459 periods: the HBM-slab kernel, the
    non-resident T0 fit): every result of the drop-in on the GPU against the same host layer fed by the oracle's
    search, spectra and T0-fit residuals."""
    t, f, kw = synthetic.config("tess_27d")
    kwargs = dict(kw, verbose=False, show_progress_bar=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = make_model(t, f, None).power(**kwargs)

        def oracle_search_periods(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                  M_star_min, M_star_max, T0_fit_margin, **_unused):
            return oracle_lib.search(t_, y_, dy_, periods, table, transit_depth_min, R_star_min, R_star_max,
                                     M_star_min, M_star_max, T0_fit_margin)[:3]

        monkeypatch.setattr(tls_amd.search, "spectra",
                            lambda chi2_, osf_, **kw_: oracle_lib.spectra(chi2_, int(osf_ * 30)))
        monkeypatch.setattr(tls_amd.search, "search_periods", oracle_search_periods)
        monkeypatch.setattr(tls_amd.search, "t0_fit_residuals",
                            lambda t_, y_, p_, s_, e_, r_, **kw_: oracle_lib.t0_residuals(t_, y_, p_, s_, e_, r_))
        want = make_model(t, f, None).power(**kwargs)
    assert list(got.keys()) == list(want.keys())
    for key in pins.SCALARS:
        numpy.testing.assert_allclose(float(got[key]), float(want[key]), rtol=1e-9, atol=1e-12, err_msg=key)
    for key in pins.ARRAYS:
        # (the spectra divide by std(SR) ~ 2e-3; the slab kernel's fast prefix-sum mode moves chi^2 by up to 1e-10 relative
        # at this N -- DESIGN.md section 3 -- against 1e-12 typical in the LDS-resident kernel)
        atol = 8e-9 if key in ("power", "power_raw", "SR") else 1e-11
        numpy.testing.assert_allclose(numpy.asarray(got[key], dtype=float), numpy.asarray(want[key], dtype=float),
                                      rtol=1e-9, atol=atol, err_msg=key)
    assert int(numpy.argmin(got.chi2)) == int(numpy.argmin(want.chi2))
    assert abs(got.period - 10.123) < 0.05


@pytest.mark.parametrize("name,devices", [("k2_90d", [0, 0]), ("tess_27d", [0, 0]), ("tess_27d", [0, 0, 0])])
def test_devices_list_shards_the_period_grid_bit_for_bit(name, devices):
    """power(devices=[...]) / DeviceGroup (reference: the use_threads pool over periods, main.py:140-163): one context and
    one host thread per listed device, period blocks by modelled time, the blocks' results brought together -- here two and
    three contexts on the one GPU of the box (the host-copy collective; the RCCL branch of distinct devices is exercised
    with stand-in contexts in test_device_group.py).  A period's result does not depend on the partition: chi2, row and
    depth of the sharded search are the BITS of the one-context search, on the LDS-resident and on the HBM-slab path
    (whose prefix-sum mode is decided per period from the light curve and the period alone)."""
    from tls_amd import _lib, search as tsearch
    t, f, kw = synthetic.config(name)
    inp = synthetic.search_inputs(t, f, **kw)
    one = _lib.Context(0)
    want = one.search(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    one.close()
    group = tsearch.DeviceGroup(devices)
    try:
        got = group.search(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
        assert group.last_collective == "host_concatenate"
        blocks = numpy.asarray(group.last_blocks)   # periods per context: the grid dealt out cyclically
        assert len(blocks) == len(devices) and blocks.sum() == len(inp["periods"]) and blocks.max() - blocks.min() <= 1
        for a, b in zip(got, want[:3]):
            numpy.testing.assert_array_equal(a, b)
        assert int(numpy.argmin(got[0])) == int(numpy.argmin(want[0]))
    finally:
        group.close()


def test_power_with_a_devices_list_returns_the_one_device_results():
    """The drop-in call itself: every field of the results object of power(devices=[0, 0]) equals power()'s."""
    t, f = synthetic.light_curve(30.0, 48, 2e-4, per=4.321, rp=0.05, a=12)
    kw = dict(period_min=1.0, period_max=9.0, oversampling_factor=2, show_progress_bar=False, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = tls_amd.transitleastsquares(t, f, verbose=False).power(**kw)
        sharded = tls_amd.transitleastsquares(t, f, verbose=False).power(devices=[0, 0], **kw)
        single = tls_amd.transitleastsquares(t, f, verbose=False).power(devices=[0], **kw)
    for other in (sharded, single):
        assert list(other.keys()) == list(plain.keys())
        for k in plain.keys():
            numpy.testing.assert_array_equal(numpy.asarray(other[k], dtype=float), numpy.asarray(plain[k], dtype=float), err_msg=k)


def test_survey_of_1024_light_curves_has_no_stalled_group():
    """one profile run of round 5 held a tls_power_batch call of 25.8 s for 1024 light curves among calls
    of 0.9 s.  The library now times every group of 32 (tls_debug_batch_group_ms): the whole call within 3 s and no group
    beyond 0.5 s (a group takes ~28 ms) -- a stall of that kind fails here with the group it happened in."""
    import time
    from tls_amd import survey, search as tsearch
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    fluxes = numpy.stack([synthetic.config("k2_90d", seed=s)[1] for s in range(1024)])
    ctx = tsearch.default_context(None)
    survey.power_batch(t, fluxes[:64], context=ctx, **kw)      # plan, pinned staging, device buffers
    t0 = time.perf_counter()
    summary, _ = survey.power_batch(t, fluxes, context=ctx, **kw)
    wall = time.perf_counter() - t0
    groups = ctx.batch_group_ms()
    assert len(groups) == 32 and len(summary) == 1024
    assert wall < 3.0, (wall, groups.max(), int(groups.argmax()))
    assert groups.max() < 500.0, (groups.max(), int(groups.argmax()), float(numpy.median(groups)))
    assert int(numpy.sum(numpy.abs(summary["period"] - 10.123) < 0.05)) == 1024


def test_auto_devices_on_a_one_gpu_box_is_the_one_device_search():
    """power()'s default devices="auto" (reference: use_threads = cpu_count(), validate.py:81): with one visible GPU it is the
    plain one-device call -- same context, same bits -- and an explicit device= or devices=[0] changes nothing."""
    from tls_amd import _lib, search as tsearch
    t, f = synthetic.light_curve(30.0, 48, 2e-4, per=4.321, rp=0.05, a=12)
    kw = dict(period_min=1.0, period_max=9.0, oversampling_factor=2, show_progress_bar=False, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auto = tls_amd.transitleastsquares(t, f, verbose=False).power(**kw)
        named = tls_amd.transitleastsquares(t, f, verbose=False).power(devices="auto", **kw)
        single = tls_amd.transitleastsquares(t, f, verbose=False).power(device=0, **kw)
    for other in (named, single):
        for k in auto.keys():
            numpy.testing.assert_array_equal(numpy.asarray(other[k], dtype=float), numpy.asarray(auto[k], dtype=float), err_msg=k)
    if _lib.device_count() == 1:
        inp = synthetic.search_inputs(t, f, period_min=1.0, period_max=9.0, oversampling_factor=2)
        assert tsearch.auto_devices(inp["t"], inp["y"], inp["periods"], inp["table"], inp["params"]) is None
        used = {}
        tsearch.search_periods(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], devices="auto", used=used, **inp["params"])
        assert used["context"] is tsearch.default_context(None) and used["devices"] == [0]


def test_survey_batches_over_a_devices_list_equal_the_one_device_batch():
    """BASELINE config 5 inside one process: survey.search_batch / power_batch with devices=[...] deal contiguous slices
    of the light curves to the contexts of a DeviceGroup (one host thread each, no collective); every light curve's
    results are those of the one-device batch, bit for bit (two contexts on the one GPU of the box)."""
    from tls_amd import survey
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    fluxes = numpy.stack([synthetic.config("k2_90d", seed=s, sigma=(1 + s % 3) * 50e-6)[1] for s in range(70)])
    kw = dict(kw, period_min=5.0, period_max=20.0)
    one = survey.search_batch(t, fluxes, **kw)
    two = survey.search_batch(t, fluxes, devices=[0, 0], **kw)
    for a, b in zip(one, two):
        numpy.testing.assert_array_equal(a, b)
    s1, p1 = survey.power_batch(t, fluxes[:40], **kw)
    s2, p2 = survey.power_batch(t, fluxes[:40], devices=[0, 0, 0], **kw)
    numpy.testing.assert_array_equal(p1, p2)
    for name in s1.dtype.names:
        numpy.testing.assert_array_equal(s1[name], s2[name], err_msg=name)


@pytest.mark.gpu
def test_pink_noise_on_the_device_returns_the_bits_of_the_reference_loop():
    """tls_pink_noise (stats.py:72-77 on the device: numpy's pairwise association inside every window, the terms added from
    the left by the exact sequential prefix sum) against the reference's own loop over numpy.std on small inputs and against
    the vectorised numpy form (tls_amd.stats.pink_noise, itself pinned to that loop) at every branch of the pairwise sum:
    widths below 8, up to 128, beyond (halved runs), one window, width = n."""
    from tls_amd import _lib, stats, search
    ctx = _lib.Context(0)
    rng = numpy.random.RandomState(5)

    def reference(data, width):   # stats.py:72-77, verbatim arithmetic
        std = 0
        datapoints = len(data) - width + 1
        for i in range(datapoints):
            std += numpy.std(data[i: i + width]) / width ** 0.5
        return std / datapoints

    for n, widths in ((40, (1, 3, 7, 8, 9, 40)), (700, (1, 8, 16, 127, 128, 129, 300, 700)), (19000, (5, 92, 257, 1000, 4097))):
        data = 1 + rng.normal(0, 3e-4, n)
        for width in widths:
            got = ctx.pink_noise(data, width)
            assert got == stats.pink_noise(data, width), (n, width)
            if n <= 700:
                assert got == reference(data, width), (n, width)
    # what power() calls: small inputs stay with numpy, large ones go to the device; the same number either way
    data = 1 + rng.normal(0, 1e-3, 30000)
    assert search.pink_noise(data, 100, context=ctx) == stats.pink_noise(data, 100)
    assert search.pink_noise(data[:500], 10, context=ctx) == stats.pink_noise(data[:500], 10)
    with pytest.raises(RuntimeError):
        ctx.pink_noise(data[:10], 11)


def test_a_failed_batch_leaves_the_context_as_a_fresh_one():
    """The failure exit of both batch entries: curve 35 (the second launch group) has per-point dy and every other curve
    uniform dy, so tls_search_batch and tls_power_batch stop with the mixed-weights error -- tls_power_batch while group 0
    is still in flight (group g + 1 is formed before group g is consumed).  The same context then gives for a valid batch
    bit for bit what a fresh context gives, for both calls."""
    from tls_amd import _lib
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    inp = synthetic.search_inputs(t, f0, None, **dict(kw, period_min=5.0, period_max=20.0))
    y = numpy.stack([inp["y"]] + [synthetic.config("k2_90d", seed=s)[1] for s in range(1, 40)])
    dy = numpy.tile(inp["dy"], (40, 1))
    mixed = dy.copy()
    mixed[35] *= 1.0 + 0.1 * numpy.sin(numpy.arange(len(t)))
    args = (inp["periods"], inp["table"], inp["params"])
    ctx, fresh = _lib.Context(0), None
    try:
        with pytest.raises(RuntimeError, match="must all have uniform or all have per-point dy"):
            ctx.search_batch(inp["t"], y, mixed, *args)
        with pytest.raises(RuntimeError, match="must all have uniform or all have per-point dy"):
            ctx.power_batch(inp["t"], y, mixed, *args, 30, with_arrays=True, with_power=True)
        got = ctx.search_batch(inp["t"], y, dy, *args)
        got_power = ctx.power_batch(inp["t"], y, dy, *args, 30, with_arrays=True, with_power=True, with_spectra=True)
        fresh = _lib.Context(0)
        want = fresh.search_batch(inp["t"], y, dy, *args)
        want_power = fresh.power_batch(inp["t"], y, dy, *args, 30, with_arrays=True, with_power=True, with_spectra=True)
    finally:
        ctx.close()
        if fresh is not None:
            fresh.close()
    for a, b in zip(got + got_power, want + want_power):
        assert a.tobytes() == b.tobytes()
