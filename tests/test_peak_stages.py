"""Every peak stage of power_batch at once, on the device: one call with the phase scan and all nine follow-ups of
survey._PEAK_STAGES against one call per stage alone, byte for byte, on the batch of tests/test_centroid.py (8 curves of 600
points, peaks=4: fitted peaks and peaks without a fit).  What each stage computes is pinned in its own test module."""
import warnings

import numpy
import pytest

import test_centroid as base
from tls_amd import _lib, survey

pytestmark = pytest.mark.gpu

# the keywords that ask for a stage (the smallest views that still have an empty and a full bin), and its fields in `peaks`
STAGES = dict(
    transit_times=(dict(transit_times=True), lambda: tuple(k for k, _ in survey.TRANSIT_TIMES_PEAK_FIELDS)),
    shape_fit=(dict(shape_fit=True), survey.shape_fit_fields),
    sine_test=(dict(sine_test=True), survey.sine_test_fields),
    ephemeris_match=(dict(ephemeris_match=True), survey.ephemeris_match_peak_fields),
    views=(dict(views=True, views_global_bins=201, views_local_bins=51),
           lambda: ("views_status",) + tuple("views_" + k for k in survey.folded_view_fields()[2:])),
    event_vetting=(dict(event_vetting=True), lambda: tuple("ev_" + k for k in survey.event_summary_fields())),
    centroids=(dict(), survey.centroid_fields),
    noise=(dict(noise=True), lambda: ("noise_width", "noise_sigma", "noise_mes")),
    transit_fit=(dict(transit_fit=True), survey.transit_fit_fields),
)
EXTRAS = dict(transit_times="transit_times", views="views", event_vetting="events", noise="noise")


def _same(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_every_stage_at_once():
    assert tuple(STAGES) == tuple(stage.name for stage in survey._PEAK_STAGES)
    rows = [base.curve_of(s) for s in range(base.N_CURVES)]
    flux, cx, cy = (numpy.array([r[i] for r in rows]) for i in range(3))
    ctx = _lib.Context(0)
    try:
        def run(names, **more):
            kw = dict(context=ctx, peaks=4, peak_fits=True, **base.KW)
            for name in names:
                kw.update(STAGES[name][0], **(dict(centroids=(cx, cy)) if name == "centroids" else {}))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return survey.power_batch(base.T, flux, **dict(kw, **more))[-1]

        every = run(STAGES, phase_scan=True)
        # (the views take their secondary view from the phase scan, so that stage alone runs behind the scan as well)
        alone = {name: run([name], phase_scan=name == "views") for name in STAGES}
    finally:
        ctx.close()
    peaks = every["peaks"]
    status = peaks["status"]
    assert peaks.shape == (base.N_CURVES, 4) and (status == 0).sum() >= 16 and (status != 0).sum() >= 1
    names = _lib.PEAK_DTYPE.names + ("duration",) + survey.peak_fit_fields() + survey.phase_scan_fields()
    for name in STAGES:
        names += tuple(STAGES[name][1]())
    assert peaks.dtype.names == names
    assert list(every) == ["peaks", "n_peaks"] + [EXTRAS[name] for name in STAGES if name in EXTRAS]
    for name, (_, fields) in STAGES.items():
        got = alone[name]
        assert got["peaks"].dtype.names[-len(fields()):] == tuple(fields()), name
        for k in fields():
            assert got["peaks"].dtype[k] == peaks.dtype[k] and _same(got["peaks"][k], peaks[k]), (name, k)
        assert set(got) == {"peaks", "n_peaks"} | ({EXTRAS[name]} if name in EXTRAS else set()), name
        if name in EXTRAS:
            a, b = got[EXTRAS[name]], every[EXTRAS[name]]
            if isinstance(a, dict):
                assert list(a) == list(b) and all(_same(a[k], b[k]) for k in a), name
            else:
                assert _same(a, b), name
    assert (peaks["tt_status"][status != 0] == 1).all() and (peaks["match_rank"][status != 0] == -1).all()
