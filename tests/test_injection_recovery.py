"""Survey-mode injection-recovery on the device (tls_inject_transits, survey.injection_recovery): the injected rows against
flux * transit_model.light_curve on the host -- bit for bit out of contact, within the model's own sensitivity to a few ulp
of z in contact -- on every case of the model, and the end-to-end call against power_batch on the same rows."""
import json
import os
import warnings

import numpy
import pytest

from tls_amd import survey, synthetic, transit_model
from test_injection_recovery_host import host_rows, random_injections

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LAWS = (("quadratic", [0.4804, 0.1867]), ("linear", [0.55]), ("uniform", None))
WORST = {}   # largest deviation in contact, per series (printed, and written where TLS_INJECT_REPORT names a file)


def _separation(t, inj, k):
    return transit_model.projected_separation(t, float(inj["T0"][k]), float(inj["period"][k]), float(inj["a"][k]),
                                              float(inj["inc"][k]), 0, 90)


def _check_rows(name, t, base, inj, rows, count, u, law):
    """Device rows and counts against the host model of every injection."""
    _, u1, u2 = survey._injection_law(u, law, {})
    want = host_rows(t, base, inj, u, law)
    worst = (0.0, None)
    for k in range(len(rows)):
        b = base if base.ndim == 1 else base[k]
        p = float(inj["rp_rs"][k])
        z = _separation(t, inj, k)
        contact = z < 1.0 + p
        edge = numpy.abs(z - (1.0 + p)) <= 1e-12
        assert abs(int(count[k]) - int(contact.sum())) <= int(edge.sum()), (name, k)
        out = ~contact & ~edge
        numpy.testing.assert_array_equal(rows[k][out], b[out], err_msg="%s: injection %d out of contact" % (name, k))
        if not contact.any() and not edge.any():
            assert count[k] == 0
            numpy.testing.assert_array_equal(rows[k], b)
            continue
        m = contact | edge
        zc, bc = z[m], b[m]
        f0 = transit_model.quadratic_ld_flux(zc, p, u1, u2)
        sens = numpy.zeros_like(zc)
        for j in (-3, -2, -1, 1, 2, 3):
            sens = numpy.maximum(sens, numpy.abs(bc * transit_model.quadratic_ld_flux(zc * (1.0 + j * EPS), p, u1, u2) - bc * f0))
        err = numpy.abs(rows[k][m] - want[k][m])
        bound = 1e-13 + 4.0 * sens
        bad = err > bound
        assert not bad.any(), ("%s: injection %d: %d points over the bound, worst %.3g at z=%.17g (p=%.17g, bound %.3g)"
                               % (name, k, bad.sum(), err[bad].max(), zc[bad][numpy.argmax(err[bad])], p,
                                  bound[bad][numpy.argmax(err[bad])]))
        assert err.max() <= 1e-7
        if err.max() > worst[0]:
            i = int(numpy.argmax(err))
            worst = (float(err[i]), dict(injection=k, law=law, z=float(zc[i]), p=p, z_minus_p=float(zc[i] - p),
                                         bound=float(bound[i])))
    prev = WORST.get(name, (0.0, None))
    if worst[0] >= prev[0]:
        WORST[name] = worst


def _series():
    t_k2 = synthetic.config("k2_90d", seed=0)[0]
    t_gap = numpy.linspace(3.0, 60.0, 2736)
    t_gap = t_gap[((t_gap < 14.0) | (t_gap > 21.5)) & ((t_gap < 40.0) | (t_gap > 41.2))]
    t_tess = synthetic.config("tess_27d", seed=0)[0]
    assert len(t_k2) == 4320 and len(t_tess) == 19440
    return (("k2_90d", t_k2), ("gapped", t_gap), ("tess_19440", t_tess))


@pytest.mark.parametrize("name,t", _series(), ids=lambda v: v if isinstance(v, str) else "")
def test_device_model_against_host(gpu, name, t):
    rng = numpy.random.RandomState(len(t))
    base = 1.0 + rng.normal(0.0, 1e-4, len(t))
    for law, u in LAWS:
        inj = random_injections(rng, t, 67)
        rows, count = gpu.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(u, law, {})[1:])
        assert rows.shape == (67, len(t)) and count.dtype == numpy.int64
        _check_rows(name, t, base, inj, rows, count, u, law)
    report = {k: dict(max_abs_err=v[0], where=v[1]) for k, v in WORST.items()}
    print("\ninjection model, largest deviation in contact:", json.dumps(report))
    if os.environ.get("TLS_INJECT_REPORT"):
        with open(os.environ["TLS_INJECT_REPORT"], "w") as fh:
            json.dump(report, fh, indent=1)


def _times_at(z_targets, T0, P, a):
    """Time stamps at which a planet on an edge-on circular orbit (inc = 90) sits at the separations z_targets, on the
    ingress side of the transit at T0 and one period later on the egress side."""
    f = numpy.arcsin(numpy.asarray(z_targets) / a)
    dt = f / (2.0 * numpy.pi) * P
    return numpy.sort(numpy.concatenate([T0 - dt, T0 + P + dt]))


def test_every_branch(gpu):
    """Points at z = 0, p, 1 - p, 1 + p and around them, for p = 0.1, 0.5, 0.7 and the fully covered p = 1.2."""
    P, a, T0 = 4.0, 3.0, 0.25   # (small t and a: the host's z lands within the snap distance of every target)
    for p in (0.1, 0.5, 0.7, 1.2):
        targets = numpy.array([0.0, p, abs(1.0 - p), 1.0 + p, max(p - 1.0, 0.0)])
        around = numpy.concatenate([targets * (1.0 + d) for d in (-1e-6, -1e-9, 1e-9, 1e-6)] + [numpy.linspace(0, 1 + p + 0.1, 97)])
        t = _times_at(numpy.unique(numpy.concatenate([targets, numpy.abs(around)])), T0, P, a)
        inj = dict(T0=[T0], period=[P], rp_rs=[p], a=[a], inc=[90.0])
        z = _separation(t, inj, 0)
        for target in targets[:3]:   # the host reaches the case: its snap takes the computed z onto the boundary
            assert numpy.min(numpy.abs(z - target)) < 1e-14, (p, target)
        assert numpy.min(numpy.abs(z - (1.0 + p))) < 1e-12
        base = numpy.ones(len(t))
        for law, u in LAWS:
            rows, count = gpu.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(u, law, {})[1:])
            _check_rows("branches", t, base, inj, rows, count, u, law)
        if p >= 1.0:   # the fully covered case: the flux of a star without light
            q = transit_model.quadratic_ld_flux(numpy.array([0.0]), p, 0.4804, 0.1867)[0]
            rows, _ = gpu.inject_transits(t, base, survey.injection_constants(inj), 0.4804, 0.1867)
            assert numpy.any(rows[0] == q)


def test_argument_errors_on_device(gpu):
    t = numpy.linspace(0.0, 10.0, 100)
    c = survey.injection_constants(dict(T0=[1.0, 2.0], period=[3.0, 3.0], rp_rs=[0.1, 0.1], a=[10.0, 10.0], inc=[90.0, 90.0]))
    with pytest.raises(RuntimeError, match="flux_rows"):
        gpu.inject_transits(t, numpy.ones((3, 100)), c, 0.4, 0.2)
    for field, value in (("period", 0.0), ("a", -1.0), ("rp", -0.1), ("tp", numpy.nan), ("sin_inc", numpy.inf)):
        bad = c.copy()
        bad[field][1] = value
        with pytest.raises(RuntimeError, match="inject"):
            gpu.inject_transits(t, numpy.ones(100), bad, 0.4, 0.2)
    with pytest.raises(RuntimeError, match="n out of range"):
        gpu.inject_transits(t[:0], numpy.ones(0), c, 0.4, 0.2)
    rows, count = gpu.inject_transits(t, numpy.ones(100), c[:0], 0.4, 0.2)
    assert rows.shape == (0, 100) and count.shape == (0,)


def _noise_curve(seed=3):
    t = synthetic.config("k2_90d", seed=0)[0]
    rng = numpy.random.RandomState(seed)
    return t, 1.0 + rng.normal(0.0, 1e-4, len(t))


def _e2e_injections(t):
    """70 injections: 20 deep ones with >= 3 transits, 10 that never transit (b > 1 + rp), 40 random ones."""
    rng = numpy.random.RandomState(21)
    deep = dict(T0=numpy.min(t) + rng.uniform(0, 1, 20) * 0, period=rng.uniform(3.0, 12.0, 20), rp_rs=rng.uniform(0.06, 0.12, 20),
                a=rng.uniform(10.0, 25.0, 20), inc=numpy.full(20, 90.0))
    deep["T0"] = numpy.min(t) + rng.uniform(0.1, 0.9, 20) * deep["period"]
    a_none = rng.uniform(10.0, 25.0, 10)
    none = dict(T0=numpy.min(t) + rng.uniform(0, 5, 10), period=rng.uniform(2.0, 15.0, 10), rp_rs=numpy.full(10, 0.05),
                a=a_none, inc=numpy.degrees(numpy.arccos(1.3 / a_none)))
    rnd = random_injections(rng, t, 40, rp_lo=0.005, rp_hi=0.05)
    rnd["period"] = rng.uniform(1.0, 20.0, 40)
    inj = {k: numpy.concatenate([deep[k], none[k], rnd[k]]) for k in survey.INJECTION_FIELDS}
    return inj, numpy.arange(20), numpy.arange(20, 30)


def _assert_summary_equal(a, b):
    assert a.dtype == b.dtype
    for k in a.dtype.names:
        numpy.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_end_to_end_against_power_batch(gpu):
    t, base = _noise_curve()
    inj, deep, none = _e2e_injections(t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        recovery, summary, rows = survey.injection_recovery(t, base, inj, chunk=40, return_rows=True, context=gpu,
                                                            aliases=(1.0, 2.0, 0.5))
        ref, _ = survey.power_batch(t, rows, context=gpu)
    assert len(recovery) == len(summary) == 70 and rows.shape == (70, len(t))
    _assert_summary_equal(summary, ref)
    counts = recovery["n_in_transit"]
    want = survey.classify_recovery(inj, ref, counts, aliases=(1.0, 2.0, 0.5))
    assert recovery.dtype == want.dtype
    for k in want.dtype.names:
        numpy.testing.assert_array_equal(recovery[k], want[k], err_msg=k)
    # the rows themselves are the device model of each injection
    _check_rows("end_to_end", t, base, inj, rows, counts, [0.4804, 0.1867], "quadratic")
    assert numpy.all(recovery["recovered"][deep]), recovery[deep]
    assert numpy.all(recovery["period_match"][deep] == 1.0)
    assert numpy.all(counts[none] == 0) and numpy.all(counts[deep] > 0)
    for k in none:
        numpy.testing.assert_array_equal(rows[k], base)
    frac, hit, total = survey.completeness(recovery, [0.5, 12.5, 25.0], [0.0, 0.06, 0.2])
    assert total.sum() == numpy.sum(counts != 0)


def test_pass_through_options(gpu):
    t, _ = _noise_curve()
    rng = numpy.random.RandomState(8)
    n_inj = 36
    bases = 1.0 + rng.normal(0.0, 1e-4, (n_inj, len(t)))
    dy = rng.uniform(0.8, 1.2, (n_inj, len(t))) * 1e-4
    inj = random_injections(rng, t, n_inj, rp_lo=0.01, rp_hi=0.1)
    inj["period"] = rng.uniform(1.5, 15.0, n_inj)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # per-injection base rows with per-point dy, and the linear law for the injection only
        rec, summ, rows = survey.injection_recovery(t, bases, inj, dy=dy, inject_u=[0.5], inject_limb_dark="linear",
                                                    return_rows=True, chunk=20, context=gpu)
        _assert_summary_equal(summ, survey.power_batch(t, rows, dy, context=gpu)[0])
        _check_rows("pass_through", t, bases, inj, rows, rec["n_in_transit"], [0.5], "linear")
        # statistics=True equals power_batch(statistics=True)
        rec_s, summ_s, rows_s = survey.injection_recovery(t, bases[0], inj, statistics=True, return_rows=True, context=gpu)
        _assert_summary_equal(summ_s, survey.power_batch(t, rows_s, context=gpu, statistics=True)[0])
        assert "snr" in summ_s.dtype.names
        # a shared per-point dy
        rec_d, summ_d, rows_d = survey.injection_recovery(t, bases[0], inj, dy=dy[0], return_rows=True, context=gpu)
        _assert_summary_equal(summ_d, survey.power_batch(t, rows_d, numpy.broadcast_to(dy[0], rows_d.shape), context=gpu)[0])
        # two slices of the batch over devices=[0, 0] equal one device
        rec_2, summ_2 = survey.injection_recovery(t, bases[0], inj, statistics=True, devices=[0, 0])
    _assert_summary_equal(summ_2, summ_s)
    for k in rec_s.dtype.names:
        numpy.testing.assert_array_equal(rec_2[k], rec_s[k], err_msg=k)
