"""no result depends on what the LDS or the scratch memory held before -- for every survey stage and every
kernel of the post-search chain, not only for the search.

(a) every case of tests/stage_memory_cases.py behind tls_debug_poison_lds (every CU's LDS filled with a word, every device
    buffer of the context that a call fills for itself smeared with 0xFF bytes), under the three words the search tests use:
    the first poisoned run -- the first call of that stage on its context -- equals the stage's statement as the stage's own
    test compares it, and the three runs equal each other byte for byte, NaN payloads included;
(b) the smaller case of a stage behind its larger one on one context, nothing poisoned between them: the buffers never shrink,
    so the small call finds the large call's counts, indices and sums, which a `< n` guard does not mask as it masks 0xFF
    bytes; it equals the same call on a fresh context byte for byte;
(c) the whole vetting chain in one power_batch call on 40 curves (two search groups, two slabs of peak fits) against one
    call a keyword on a second context, behind poison, and dealt out over two contexts of one device.

Every test runs on contexts of its own, so that its history is the test's."""
import warnings

import numpy
import pytest

import stage_memory_cases as cases
from tls_amd import _lib, survey, transit_model

pytestmark = pytest.mark.gpu

WORDS = (0x7ff80000, 0xfff00000, 0xffffffff)   # a quiet NaN's high word, -inf's, all ones: what the search tests poison with


def same_bytes(a, b, what):
    a, b = cases.arrays(a), cases.arrays(b)
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, "output %d" % i)


def statement(case):
    """The statement's side of a case; a statement that runs a kernel itself gets a context of its own."""
    if case.want is None:
        return None
    if not case.want_on_device:
        return case.want()
    ref = _lib.Context(0)
    try:
        return case.want(ref)
    finally:
        ref.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_stage_behind_poisoned_memory(name):
    case = cases.CASES[name]
    ctx = _lib.Context(0)
    try:
        runs = []
        for word in WORDS:
            ctx.poison_lds(word)
            runs.append(case.run(ctx))
            if len(runs) == 1 and case.compare is not None:
                case.compare(runs[0], statement(case))     # (the first call of this stage on this context, behind poison)
        for word, again in zip(WORDS[1:], runs[1:]):
            same_bytes(again, runs[0], (name, hex(word), "against", hex(WORDS[0])))
    finally:
        ctx.close()


@pytest.mark.parametrize("stage", list(cases.BEHIND))
def test_small_call_behind_a_large_one(stage):
    large, small = (cases.CASES[k] for k in cases.BEHIND[stage])
    ctx, fresh = _lib.Context(0), _lib.Context(0)
    try:
        large.run(ctx)
        behind = small.run(ctx)
        alone = small.run(fresh)
        same_bytes(behind, alone, (stage,) + cases.BEHIND[stage])
    finally:
        ctx.close()
        fresh.close()


# ---- (c) the whole vetting chain in one call ------------------------------------------------------------------------------------
T = 3.0 + numpy.arange(500) / 16.0                    # 31 d at 90 min: the series of test_folded_views.flux_rows
KW = dict(period_min=1.5, period_max=6, oversampling_factor=1)
N_CURVES, K = 40, 4                                   # two search groups of 32; 160 fits: two peak-fit slabs of 128


def chain_rows():
    """40 rows of 500 points built as test_folded_views.flux_rows builds its four -- planets, a binary with a secondary, quiet
    rows, in turn -- and their centroid rows as centroid_cases.curves makes them (noise, a slow drift)."""
    kinds = ((2.9, 0.1, 0.0), (4.3, 0.12, 0.0), (3.7, 0.15, 6e-3), (0.0, 0.0, 0.0))
    rows = []
    for s in range(N_CURVES):
        per, rp, sec = kinds[s % 4]
        per = per * (1.0 + 0.01 * (s // 4))
        rng = numpy.random.RandomState(2000 + s)
        f = 1.0 + rng.normal(0, 3e-4, len(T)) + 1e-3 * numpy.sin(T / 2.3 + s)
        if per:
            f += transit_model.light_curve(T, T[0] + 0.8, per, rp, 9.0, 89.9, 0, 90, [0.4, 0.3], "quadratic") - 1
            f -= sec * (numpy.fabs((T - T[0] - 0.8) / per - 0.5 - numpy.round((T - T[0] - 0.8) / per - 0.5)) * per < 0.1)
        rows.append(f)
    import centroid_cases
    _, cx, cy = centroid_cases.curves(T, N_CURVES, 31)
    return numpy.array(rows), cx, cy


def run_chain(flux, floor, **kw):
    """power_batch(peaks=4, statistics=True, peak_fits=True, with_arrays=True) of the rows, with the stages `kw` names."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return survey.power_batch(T, flux, peaks=K, peak_fits=True, statistics=True, with_arrays=True, peak_min_power=floor,
                                  **kw, **KW)


def results_equal(got, want, what):
    """Two results of the same call: every array, every field and every side array byte for byte."""
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got[:-1], want[:-1])):
        same_bytes(a, b, (what, i))
    assert set(got[-1]) == set(want[-1]), what
    for k in want[-1]:
        same_bytes(got[-1][k], want[-1][k], (what, k))


def test_the_whole_vetting_chain_in_one_call():
    flux, cx, cy = chain_rows()
    stages = dict(phase_scan=True, transit_times=True, shape_fit=True, sine_test=True, views=True, event_vetting=True,
                  centroids=(cx, cy), ephemeris_match=True)
    one, two = _lib.Context(0), _lib.Context(0)
    try:
        # a floor above the weakest tenth of the peaks' powers (as test_folded_views.run sets its floor): those peaks are not
        # taken, some curves keep fewer than K peaks, and their places -- status 1, no such peak -- flow through every stage
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            power = survey.power_batch(T, flux, peaks=K, context=two, **KW)[2]["peaks"]["power"].ravel()
        power = numpy.sort(power[~numpy.isnan(power)])
        assert len(power) > N_CURVES * K // 2 and power[len(power) // 10 - 1] < power[len(power) // 10]
        floor = float(0.5 * (power[len(power) // 10 - 1] + power[len(power) // 10]))
        full = run_chain(flux, floor, context=one, **stages)
        summary, periods, chi2, row, depth, spectrum, pk = full
        peaks, n_peaks = pk["peaks"], pk["n_peaks"]
        assert peaks.shape == (N_CURVES, K) and n_peaks.min() < K and n_peaks.max() >= 2
        assert N_CURVES * K > _lib.VIEWS_SLAB // 8 and (peaks["status"][32:] == 0).any() and (peaks["status"] != 0).any()
        # the summary, the periods, the search's arrays and the spectrum are the plain call's, the peaks' and the fits' fields too
        plain = run_chain(flux, floor, context=two)
        for i in range(len(plain) - 1):
            same_bytes(full[i], plain[i], ("plain", i))
        same_bytes(n_peaks, plain[-1]["n_peaks"], "n_peaks")
        seen = set(plain[-1]["peaks"].dtype.names)
        for k in plain[-1]["peaks"].dtype.names:
            same_bytes(peaks[k], plain[-1]["peaks"][k], ("plain", k))
        # every keyword alone on the second context: its fields of `peaks` and its side arrays
        for keyword, value in stages.items():
            more = {keyword: value}
            if keyword == "views":
                more["phase_scan"] = True              # (the secondary view is centred on the scan's phase, which the full call has)
            alone = run_chain(flux, floor, context=two, **more)[-1]
            added = [k for k in alone["peaks"].dtype.names if k not in plain[-1]["peaks"].dtype.names]
            assert added, keyword
            for k in added:
                same_bytes(peaks[k], alone["peaks"][k], (keyword, k))
            seen |= set(added)
            for side in set(alone) - {"peaks", "n_peaks"}:
                same_bytes(pk[side], alone[side], (keyword, side))
        assert seen == set(peaks.dtype.names), set(peaks.dtype.names) - seen
        assert {"transit_times", "events", "views"} <= set(pk)
        # the full call again behind poison, and dealt out over two contexts of the device
        one.poison_lds(0xffffffff)
        results_equal(run_chain(flux, floor, context=one, **stages), full, "behind poison")
        results_equal(run_chain(flux, floor, devices=[0, 0], **stages), full, "devices=[0, 0]")
    finally:
        one.close()
        two.close()
