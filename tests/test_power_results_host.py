"""Survey-mode results objects (survey.power_results, tls_power_batch_models), the parts that need no GPU: the binding against
the header, the assembly of the 41-key objects from the device's arrays, and the argument checks."""
import os
import re

import numpy
import pytest

from tls_amd import _lib, search, survey, synthetic
from tls_amd.api import transitleastsquares
from tls_amd.results import RESULT_KEYS
from conftest import REPO


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "tls_amd.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_binding_matches_the_header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    assert int(re.search(r"#define TLS_AMD_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 8
    lib = _lib.load()
    for name in ("tls_power_batch_models", "tls_debug_transit_models"):
        assert name in _lib.SYMBOLS
        assert len(getattr(lib, name).argtypes) == len(declaration(name)), name
    # the models entries are the statistics entries plus the same eleven model arguments
    assert declaration("tls_power_batch_models")[:-11] == declaration("tls_power_batch_stats")
    assert declaration("tls_debug_transit_models")[:-11] == declaration("tls_debug_transit_stats")
    assert declaration("tls_power_batch_models")[-11:] == declaration("tls_debug_transit_models")[-11:]


def test_lc_cap_covers_every_epoch_count():
    n, max_epochs = 4320, 50
    cap = survey._lc_cap(n, max_epochs)
    for E in range(1, max_epochs + 1):
        s = int(n / E) * 5
        assert cap >= (E + 1) * s + 1
    assert cap <= 15 * n


def fake_batch(n_curves, t, n_periods=40, no_fit=()):
    """What _power_batch returns with models and spectra, filled with recognisable values."""
    from tls_amd._lib import POWER_SUMMARY_DTYPE, TRANSIT_STATS_DTYPE
    n, max_e, cap = len(t), 6, 50
    rng = numpy.random.RandomState(3)
    fields = [(k, POWER_SUMMARY_DTYPE[k]) for k in POWER_SUMMARY_DTYPE.names] + [("duration", "f8")]
    fields += [(k, "f8") for k in TRANSIT_STATS_DTYPE.names] + [("rp_rs", "f8"), ("FAP", "f8"), ("chi2red_min", "f8")]
    summary = numpy.zeros(n_curves, dtype=fields)
    for k in summary.dtype.names:
        summary[k] = rng.uniform(1, 5, n_curves) if summary.dtype[k].kind == "f" else 3
    summary["transit_count"] = 4
    summary["no_fit"] = [1 if k in no_fit else 0 for k in range(n_curves)]
    periods = numpy.linspace(1.0, 5.0, n_periods)
    arrays = [rng.uniform(1, 2, (n_curves, n_periods)) for _ in range(6)]   # chi2 row depth power SR power_raw
    pt = {k: rng.uniform(0, 1, (n_curves, max_e)) for k in _lib.PER_TRANSIT_FIELDS}
    pt["n_epochs"] = numpy.full(n_curves, 4)
    m = {k: rng.uniform(0, 1, (n_curves, n)) for k in ("folded_phase", "folded_y", "folded_dy", "model_folded_model")}
    m.update({k: rng.uniform(0, 1, (n_curves, cap)) for k in _lib.LIGHTCURVE_FIELDS})
    m["lc_len"] = numpy.full(n_curves, 17)
    m["model_folded_phase"] = numpy.linspace(0 + 1 / n / 2, 1 + 1 / n / 2, n)
    chi2, row, depth, power, SR, power_raw = arrays
    return summary, periods, chi2, row, depth, power, pt, m, SR, power_raw


def test_results_objects_are_assembled_key_for_key(monkeypatch):
    t = numpy.linspace(0.0, 10.0, 300)
    fake = fake_batch(3, t, no_fit=(1,))
    monkeypatch.setattr(survey, "_power_batch", lambda *a, **k: fake)
    summary, periods, chi2, row, depth, power, pt, m, SR, power_raw = fake
    got = survey.power_results(t, numpy.ones((3, len(t))))
    assert len(got) == 3
    for r in got:
        assert tuple(r.keys()) == RESULT_KEYS
    # the curve without a fit: exactly power()'s object for it
    chi2red = chi2[1] / (len(t) - 4)
    want = transitleastsquares._results_without_fit(None, periods, chi2[1], chi2red, numpy.min(chi2[1]), numpy.min(chi2red))
    assert tuple(want.keys()) == tuple(got[1].keys())
    for key in want:
        numpy.testing.assert_array_equal(numpy.asarray(got[1][key], dtype=float), numpy.asarray(want[key], dtype=float), key)
    # a curve with a fit: tuples from the _std fields, rows cut to the epochs and to the model light curve's length
    r, rec = got[2], summary[2]
    assert r.depth_mean == (rec["depth_mean"], rec["depth_mean_std"])
    assert r.depth_mean_odd == (rec["depth_mean_odd"], rec["depth_mean_odd_std"])
    assert r.depth_mean_even == (rec["depth_mean_even"], rec["depth_mean_even_std"])
    assert r.period == periods[rec["index_power"]] and r.depth == depth[2][rec["index_power"]]
    assert r.transit_times == list(pt["transit_times"][2, :4]) and r.transit_count == 4
    numpy.testing.assert_array_equal(r.chi2red, chi2[2] / (len(t) - 4))
    assert r.chi2red_min == numpy.min(chi2[2] / (len(t) - 4))
    assert r.periods is periods
    assert len(r.model_lightcurve_time) == len(r.model_lightcurve_model) == 17
    numpy.testing.assert_array_equal(r.folded_dy, m["folded_dy"][2])
    numpy.testing.assert_array_equal(r.SR, SR[2])
    numpy.testing.assert_array_equal(r.power_raw, power_raw[2])


def test_argument_errors_come_before_any_device_work(monkeypatch):
    def no_device(*args, **kwargs):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(search, "default_context", no_device)
    monkeypatch.setattr(search, "device_group", no_device)
    monkeypatch.setattr(_lib, "Context", no_device)
    t, f = synthetic.light_curve(20.0, 24, 2e-4, per=3.3, rp=0.05, a=10)
    kw = dict(period_min=1.0, period_max=6.0)
    with pytest.raises(ValueError, match="shape"):
        survey.power_results(t, f, **kw)
    with pytest.raises(ValueError, match="shape"):
        survey.power_results(t, numpy.stack([f, f])[:, :-1], **kw)
    with pytest.raises(ValueError):
        survey.power_results(t, numpy.stack([f, f]), dy_batch=numpy.ones((2, len(t) - 1)), **kw)
    unsorted = t.copy()
    unsorted[[10, 11]] = unsorted[[11, 10]]
    with pytest.raises(ValueError, match="ascending"):
        survey.power_results(unsorted, numpy.stack([f, f]), **kw)
    with pytest.raises(ValueError, match="ascending"):
        survey.power_batch(unsorted, numpy.stack([f, f]), models=True, **kw)
