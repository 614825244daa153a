"""power_batch's peak stages on the host: the whole chain on the stand-in context of tests/peak_stages_fake.py, pinned byte
for byte to tests/golden/peak_stages_host.npz, which tools/gen_peak_stages_golden.py made from the commit before survey.py
got its stage table (_PEAK_STAGES).  No device and no built library."""
import inspect
import json
import os

import numpy
import pytest

import peak_stages_fake as fake
from tls_amd import survey

GOLDEN = numpy.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "peak_stages_host.npz"))


def _equals_golden(prefix, got):
    names = sorted(k for k in GOLDEN.files if k.startswith(prefix) and not k.endswith(".log"))
    assert names == sorted(got)
    for k in names:
        assert got[k].dtype == GOLDEN[k].dtype and got[k].shape == GOLDEN[k].shape, k
        assert got[k].tobytes() == GOLDEN[k].tobytes(), k


def _same(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def all_on():
    return fake.run(survey, 3, fake.ALL)


def test_every_stage_on_equals_the_parent_commit(all_on):
    summary, found, log = all_on
    _equals_golden("one.", fake.flatten("one.", summary, found))
    assert log == json.loads(str(GOLDEN["one.log"]))
    assert len(found["peaks"].dtype.names) == 163
    status = found["peaks"]["status"]
    assert (status == 0).sum() >= 3 and ((status != 0).sum(axis=1) >= 1).all()      # (fitted peaks, and unfitted ones in every curve)


@pytest.mark.parametrize("name", fake.STAGES)
def test_a_stage_alone_adds_its_own_fields_and_nothing_else(all_on, name):
    # (the views read the phase scan's secondary_phase, as they do with every stage on: that stage runs behind the scan)
    before = ("phase_scan",) if name == "views" else ()
    _, base, _ = fake.run(survey, 3, before)
    summary, alone, log = fake.run(survey, 3, before + (name,))
    assert summary.tobytes() == all_on[0].tobytes()
    own = [k for k in alone["peaks"].dtype.names if k not in base["peaks"].dtype.names]
    assert own and alone["peaks"].dtype.names == base["peaks"].dtype.names + tuple(own)
    for k in own:
        assert alone["peaks"].dtype[k] == all_on[1]["peaks"].dtype[k] and _same(alone["peaks"][k], all_on[1]["peaks"][k]), k
    for k in base["peaks"].dtype.names:
        assert _same(alone["peaks"][k], base["peaks"][k]), k
    extras = sorted(set(alone) - set(base))
    assert extras == sorted(k for k in {"transit_times": ["transit_times"], "views": ["views"], "event_vetting": ["events"],
                                        "noise": ["noise"]}.get(name, []))
    for k in extras:
        for sub in (alone[k] if isinstance(alone[k], dict) else [None]):
            a, b = (alone[k], all_on[1][k]) if sub is None else (alone[k][sub], all_on[1][k][sub])
            assert _same(a, b), (k, sub)
    assert _same(alone["n_peaks"], base["n_peaks"])
    assert [c[1] for c in log][0] == "_power_batch" and len(log) == 2


def test_two_slices_equal_one_context_and_the_match_runs_once_behind_them(monkeypatch):
    group = fake.FakeGroup()
    t, flux, dy, cx, cy = fake.batch(5)
    kw = dict(fake.stage_keywords(fake.ALL, cx, cy), peaks=fake.N_PEAKS, peak_fits=True, **fake.KW)
    one = survey.power_batch(t, flux, dy, context=fake.FakeContext(), **kw)
    monkeypatch.setattr(survey, "_resolve", lambda devices, device, context, n_curves: ("group", group))
    two = survey.power_batch(t, flux, dy, devices=[0, 1], **kw)
    _equals_golden("two.", fake.flatten("two.", two[0], two[-1]))
    assert group.log == json.loads(str(GOLDEN["two.log"]))
    assert one[0].tobytes() == two[0].tobytes()
    assert one[-1]["peaks"].dtype == two[-1]["peaks"].dtype
    for k in one[-1]["peaks"].dtype.names:
        if not k.startswith("match_"):
            assert _same(one[-1]["peaks"][k], two[-1]["peaks"][k]), k
    a, b = fake.flatten("", one[0], one[-1]), fake.flatten("", two[0], two[-1])
    assert sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a if k != "peaks")
    calls = [(c[0], c[1], c[2]) for c in group.log]
    assert [c[:2] for c in calls if c[1] == "_power_batch"] == [("ctx0", "_power_batch"), ("ctx1", "_power_batch")]
    assert sorted(c[2] for c in calls if c[1] == "_power_batch") == [2, 3]
    assert [c[:2] for c in calls].count(("ctx0", "ephemeris_match")) == 1 and calls[-1][:2] == ("ctx0", "ephemeris_match")
    assert not any(c[1] == "ephemeris_match" for c in calls[:-1])


def test_the_sine_test_gets_no_weights_without_a_dy_batch():
    _, found, log = fake.run(survey, 3, ("sine_test",), dy=False)
    names = [k for k in found["peaks"].dtype.names if k.startswith("sine_")]
    assert fake.field_bytes(found["peaks"], names).tobytes() == GOLDEN["nody.sine"].tobytes()
    assert [c for c in log if c[1] == "sine_test"] == json.loads(str(GOLDEN["nody.log"]))
    assert log[-1][4]["weighted"] == 0


def test_power_batch_keeps_its_signature():
    sig = inspect.signature(survey.power_batch)
    assert [[k, repr(p.default), str(p.kind)] for k, p in sig.parameters.items()] == json.loads(str(GOLDEN["signature"]))


def test_the_pipeline_names_no_stage():
    source = inspect.getsource(survey._power_batch)
    assert tuple(stage.name for stage in survey._PEAK_STAGES) == fake.STAGES
    assert [name for name in fake.STAGES if name in source] == []
    assert [s.scope for s in survey._PEAK_STAGES].count("batch") == 1
    assert "stages" in inspect.signature(survey._power_batch).parameters
    assert not set(fake.STAGES) & set(inspect.signature(survey._power_batch).parameters)


def test_joined_keeps_every_dtype_and_allocates_nothing_for_one_part():
    a = numpy.zeros((2, 3), dtype=[("x", "f8"), ("i", "i8")])
    a["x"], a["i"] = numpy.arange(6.0).reshape(2, 3), -1
    b = numpy.ones((2, 3), dtype=[("h", "f8", (4,))])
    out = survey._joined(a, b, None)
    assert out.dtype.descr == a.dtype.descr + b.dtype.descr and out.shape == (2, 3)
    assert _same(out["x"], a["x"]) and _same(out["i"], a["i"]) and _same(out["h"], b["h"])
    assert survey._joined(None, b) is b and survey._joined(a) is a


def test_peak_candidates():
    from tls_amd import _lib
    peaks, fits = numpy.zeros((2, 2), dtype=_lib.PEAK_DTYPE), numpy.zeros((2, 2), dtype=_lib.PEAK_FIT_DTYPE)
    peaks["period"], fits["T0"], fits["duration_days"] = [[2.0, 3.0], [4.0, 5.0]], [[0.1, 0.2], [0.3, 0.4]], 0.25
    fits["status"] = [[0, 1], [2, 0]]
    period, T0, duration, curve, fitted = survey._peak_candidates(peaks, fits)
    assert fitted.tolist() == [True, False, False, True] and curve.tolist() == [0, 0, 1, 1]
    assert numpy.array_equal(period, [2.0, numpy.nan, numpy.nan, 5.0], equal_nan=True)
    assert numpy.array_equal(T0, [0.1, numpy.nan, numpy.nan, 0.4], equal_nan=True)
    assert numpy.array_equal(duration, [0.25, numpy.nan, numpy.nan, 0.25], equal_nan=True)
    period, _, _, _, fitted = survey._peak_candidates(peaks, fits, keep=numpy.array([False, True, True, True]))
    assert fitted.tolist() == [False, False, False, True] and numpy.isnan(period[:3]).all() and period[3] == 5.0
