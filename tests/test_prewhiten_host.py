"""Pre-whitening without a GPU: the statement (tests/prewhiten_spec.py) on a pulsator with a transit, the premise the GPU
tests rest on, survey.gls_power_threshold, and the arguments of survey.Prewhiten / prewhiten_batch.

The pulsator is the one the feature was specified on: 1367 points over 30 d with a gap of 1.5 d, noise 3e-4, pulsations of
5e-3, 3e-3 and 2e-3 at 5.37, 7.91 and 11.13 cycles a day, and a 0.5 % box transit of 0.12 d every 3.3 d.  Measured here on
the seeds 0-4 (the figures README.md and DESIGN.md "Pre-whitening" quote; run with -s to see them):

    rms before 4.45e-3 .. 4.46e-3; after three terms 9.4e-4 .. 9.6e-4 (the transit included; out of transit 2.96e-4 .. 3.06e-4)
    depth kept (1 = the whole transit): K = 3: 0.986 .. 1.009;  K = 4: 0.914 .. 0.937 (the fourth term lands on 1 / P or 2 / P);
    K = 4 on the grid above 3.1 cycles a day (the transit's tenth harmonic is at 3.03): 0.945 .. 0.967 -- the cut helps, but a
    box has harmonics beyond the tenth, and the fourth term finds one
    white noise of 3e-4 on these time stamps: highest power 0.0098 .. 0.0177 on ten seeds, the default min_power 0.0196
"""
import numpy
import pytest

import gls_spec
import prewhiten_cases
import prewhiten_spec as spec
from tls_amd import _lib, survey

SIGNALS = ((5.37, 5e-3), (7.91, 3e-3), (11.13, 2e-3))
PERIOD, DURATION, DEPTH = 3.3, 0.12, 5e-3


def pulsator(seed, signals=SIGNALS, depth=DEPTH):
    """(t, y, in_transit) of the module's docstring."""
    rng = numpy.random.default_rng(seed)
    t = numpy.arange(1440) * (30.0 / 1440)
    t = t[(t < 13.0) | (t >= 14.5)][:1367] + 2458000.0
    assert len(t) == 1367
    y = numpy.ones(len(t))
    for f, amp in signals:
        y += amp * numpy.sin(2.0 * numpy.pi * (f * (t - t[0]) + rng.uniform()))
    phase = ((t - t[0] - 1.0) / PERIOD + 0.5) % 1.0 - 0.5
    inside = numpy.abs(phase) * PERIOD <= 0.5 * DURATION
    y = y * numpy.where(inside, 1.0 - depth, 1.0)
    return t, y + 3e-4 * rng.standard_normal(len(t)), inside


def depth_kept(flat, inside):
    return (1.0 - flat[inside].mean() / flat[~inside].mean()) / DEPTH


@pytest.fixture(scope="module")
def runs():
    """seed -> (t, y, inside, f, {label: the statement's run})."""
    out = {}
    for seed in range(5):
        t, y, inside = pulsator(seed)
        f = survey.variability_frequencies(t)
        cut = survey._prewhiten_grid(t, f_min=3.1)
        out[seed] = (t, y, inside, f, dict(k3=spec.prewhiten(t, y, f, n_terms=3), k4=spec.prewhiten(t, y, f, n_terms=4),
                                           k4_cut=spec.prewhiten(t, y, cut, n_terms=4)))
    return out


def test_three_terms_recover_the_three_pulsations(runs):
    for seed, (t, y, inside, f, run) in runs.items():
        k3 = run["k3"]
        step = f[1] - f[0]
        assert k3["status"] == 0.0 and k3["n_iterations"] == 3
        found = sorted(terms[0]["frequency"] for terms in k3["terms"])
        for got, (want, _) in zip(found, SIGNALS):
            assert abs(got - want) <= step, (seed, got, want)
        before, after = numpy.std(y), numpy.std(k3["r"])
        out = numpy.std(k3["r"][~inside])
        print("seed %d: rms before %.3e, after three terms %.3e (out of transit %.3e)" % (seed, before, after, out))
        assert after < 0.3 * before
        numpy.testing.assert_array_equal(k3["flat"], y / k3["trend"])


def test_a_fourth_term_eats_into_the_transit(runs):
    """The depth kept, measured (the module's docstring); the one thing fixed: three terms keep more than four."""
    for seed, (t, y, inside, f, run) in runs.items():
        kept = {label: depth_kept(r["flat"], inside) for label, r in run.items()}
        fourth = run["k4"]["terms"][3][0]["frequency"]
        print("seed %d: depth kept K=3 %.3f, K=4 %.3f (fourth term at %.4f = %.2f / P), K=4 with f_min=3.1 %.3f"
              % (seed, kept["k3"], kept["k4"], fourth, fourth * PERIOD, kept["k4_cut"]))
        assert kept["k3"] > kept["k4"], (seed, kept)


@pytest.mark.parametrize("name", sorted(prewhiten_cases.cases()))
def test_the_highest_power_stands_clear_in_every_gpu_input(name):
    """The premise of tests/test_prewhiten.py's comparison of the pick: a condition on the inputs, not a tolerance."""
    gaps = [g for run in prewhiten_cases.statement(name) for g in run["gaps"]]
    finite = [g for g in gaps if numpy.isfinite(g)]
    print(name, "iterations", len(gaps), "smallest relative gap %.3e" % (min(finite) if finite else numpy.inf))
    assert gaps or name == "edges"
    assert all(g >= prewhiten_cases.MIN_GAP for g in gaps), (name, min(gaps))


def test_the_cases_are_what_they_say():
    c = prewhiten_cases.cases()
    stops = prewhiten_cases.statement("one_stops")
    assert [r["n_iterations"] for r in stops] == [3, 1, 3] and [r["status"] for r in stops] == [0.0, 1.0, 0.0]
    edges = prewhiten_cases.statement("edges")
    assert edges[0]["status"] == 2.0 and edges[0]["n_iterations"] == 0
    numpy.testing.assert_array_equal(edges[0]["flat"], c["edges"].y[0] / edges[0]["mean0"])
    F = len(c["edges"].f)
    assert edges[1]["terms"][0][0]["index"] == 0 and edges[1]["terms"][0][0]["frequency"] == c["edges"].f[0]
    assert edges[2]["terms"][0][0]["index"] == F - 1 and edges[2]["terms"][0][0]["frequency"] == c["edges"].f[-1]
    assert 0 < edges[3]["terms"][0][0]["index"] < F - 1 and edges[3]["terms"][0][0]["frequency"] != edges[3]["terms"][0][0]["frequency_grid"]
    assert len(c["two_slabs"].y) == 4097 and c["lds_side"].y.shape[1] == _lib.PREWHITEN_LDS_POINTS == c["global_side"].y.shape[1] - 1
    assert all(len(case.f) <= 128 for case in (c["lds_side"], c["global_side"]))


def test_gls_power_threshold_is_its_formula():
    for n, F, fap, over in ((1367, 3400, 1e-3, 5), (100, 50, 0.01, 1), (4320, 9000, 1e-6, 5.0)):
        want = 1.0 - (fap / (F / over)) ** (2.0 / (n - 3))
        assert survey.gls_power_threshold(n, F, fap, over) == pytest.approx(want, rel=1e-14)
    assert 0.0 < survey.gls_power_threshold(1367, 3400, 1e-3) < 0.03
    for bad in ((3, 10, 0.1), (10, 0, 0.1), (10, 10, 0.0), (10, 10, 5.0), (10.5, 10, 0.1), (10, 10, numpy.nan)):
        with pytest.raises(ValueError):
            survey.gls_power_threshold(*bad)
    with pytest.raises(ValueError):
        survey.gls_power_threshold(10, 10, 0.1, oversampling=0)


def test_white_noise_has_nothing_removed():
    """At the default min_power (false-alarm probability 1e-3) ten white-noise curves keep every point."""
    t = pulsator(0)[0]
    f = survey.variability_frequencies(t)
    low = survey.gls_power_threshold(len(t), len(f), survey.PREWHITEN_FAP)
    for seed in range(10):
        y = 1.0 + 3e-4 * numpy.random.default_rng(100 + seed).standard_normal(len(t))
        run = spec.prewhiten(t, y, f, n_terms=3, min_power=low)
        print("seed %d: highest power %.4f, min_power %.4f" % (seed, run["powers"][0].max(), low))
        assert run["status"] == 1.0 and run["n_iterations"] == 0
        numpy.testing.assert_array_equal(run["flat"], y / gls_spec.prologue(y)[2])


def test_prewhiten_steps_parse():
    step = survey.Prewhiten()
    assert step == (3, 1, None, None, None) and survey.Prewhiten(2, 2, 0.1, 1.0, 9.0).f_max == 9.0
    assert survey._detrend_steps(step) == (step,)
    both = (survey.Biweight(0.75), survey.Prewhiten(2))
    assert survey._detrend_steps(both) == both and survey._detrend_steps([25, step]) == (25, step)
    survey._no_ensemble_step(both, "injection_recovery")
    with pytest.raises(ValueError, match="a step of detrend must be a kernel size, a Biweight or a SysRem"):
        survey._detrend_steps((step, None))
    assert survey.prewhiten_term_fields() == spec.TERM_FIELDS == _lib.PREWHITEN_FIELDS
    assert _lib.PREWHITEN_DTYPE.itemsize == 8 * len(spec.TERM_FIELDS)
    t = pulsator(0)[0]
    f = survey.variability_frequencies(t)
    grid, k, h, low = survey._prewhiten_step(t, survey.Prewhiten(2, 3, f_min=3.1, f_max=10.0), len(t))
    assert (k, h) == (2, 3) and grid[0] >= 3.1 and grid[-1] <= 10.0 and numpy.all(numpy.isin(grid, f))
    assert low == survey.gls_power_threshold(len(t), len(grid), 1e-3)
    assert survey._prewhiten_step(t, survey.Prewhiten(min_power=0.25), len(t))[3] == 0.25


def test_bad_arguments_raise():
    t, y, _ = pulsator(0)
    f = survey.variability_frequencies(t)
    good = _lib.prewhiten_arguments(t, y, None, f, 3, 1, 0.0)
    assert good["y"].shape == (1, len(t)) and good["n_terms"] == 3 and good["dy"] is None
    for kw in (dict(n_terms=0), dict(n_terms=33), dict(n_terms=2.0), dict(n_terms=True), dict(harmonics=0), dict(harmonics=9),
               dict(min_power=-0.1), dict(min_power=1.5), dict(min_power=numpy.nan), dict(min_power="x")):
        args = dict(n_terms=3, harmonics=1, min_power=0.0)
        args.update(kw)
        with pytest.raises(ValueError, match="prewhiten"):
            _lib.prewhiten_arguments(t, y, None, f, **args)
    with pytest.raises(ValueError):
        _lib.prewhiten_arguments(t, y[:-1], None, f)
    with pytest.raises(ValueError):
        _lib.prewhiten_arguments(t, numpy.where(numpy.arange(len(y)) == 5, numpy.nan, y), None, f)
    with pytest.raises(ValueError):
        _lib.prewhiten_arguments(t, y, numpy.zeros(len(y)), f)
    with pytest.raises(ValueError):
        _lib.prewhiten_arguments(t[::-1], y, None, f)
    with pytest.raises(ValueError):
        _lib.prewhiten_arguments(t, y, None, -f)
    for kw in (dict(f_min=0.0), dict(f_max=numpy.inf), dict(f_min="1"), dict(f_min=50.0), dict(f_min=5.0, f_max=4.0)):
        with pytest.raises(ValueError, match="prewhiten"):
            survey._prewhiten_grid(t, **kw)
    # the survey calls refuse a bad step before any device work (no GPU here: nothing else could raise a ValueError)
    with pytest.raises(ValueError, match="prewhiten"):
        survey.prewhiten_batch(t, y, n_terms=0)
