"""Iterative pre-whitening on the device (tls_prewhiten, survey.prewhiten_batch and detrend=Prewhiten(...) of the survey calls)
against tests/prewhiten_spec.py.  Every check is local to one (iteration, harmonic): the row that enters it is the device's own
(out_steps), so nothing propagates from one step into the next.

  * the mean and the variance of the row fitted equal the statement's ordered 256-lane sums bit for bit;
  * the six sums lie within gls_spec.sum_bound of the exact sums;
  * the pick equals the statement's (tests/test_prewhiten_host.py asserts of these inputs that the highest power stands clear);
  * f* equals the statement's formula of the device's own three powers bit for bit; ca, sa, power and amplitude equal the
    statement's epilogue of the device's own sums bit for bit; phase is the device's atan2 (4 * 2^-53 cycles, as test_gls.py);
  * the row behind a subtraction equals the statement's subtraction with the device's ca, sa, C, S within
    prewhiten_spec.subtract_bound;
  * flat == y / trend bit for bit; trend == ybar_0 where nothing was subtracted, bit for bit; elsewhere the device's sum of
    what it subtracted is not among its outputs, and trend is held to ybar_0 + the statement's q of the device's coefficients
    within the same bound a term (plus the roundings of the additions).

The inputs are tests/prewhiten_cases.py's: 255, 256 and 257 points, 700 with a gap, 3 and 40 curves (either side of the 32 rows
of the small product kernel), 4097 curves (two slabs), 333 frequencies, with and without dy, (K, H) = (3, 1) and (2, 2), and
6144 / 6145 points (the last row length fitted in the LDS, the first fitted in device memory)."""
import warnings

import numpy
import pytest

import gls_spec
import prewhiten_cases
import prewhiten_spec as spec
from tls_amd import _lib, survey, synthetic

pytestmark = pytest.mark.gpu

PHASE_TOL = 4 * 2.0 ** -53
EPS = 2.0 ** -52


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


def same(a, b, what):
    assert numpy.array_equal(_bits(a), _bits(b)), what


def run(gpu, case):
    flat, trend, info = gpu.prewhiten(case.t, case.y, case.f, case.n_terms, case.harmonics, case.min_power, dy=case.dy,
                                      return_trend=True, debug=True)
    return flat, trend, info


def check_curve(case, c, flat, trend, info, want):
    """Curve c of a device run against the statement step by step; `want` is the statement's own run of the curve."""
    t, f, K, H = case.t, case.f, case.n_terms, case.harmonics
    y = case.y[c]
    dy = None if case.dy is None else case.dy[c]
    steps, terms, sums = info["steps"][:, c], info["terms"][c], info["sums"][c]
    ran = int(info["n_iterations"][c])
    what = "curve %d" % c
    assert ran == want["n_iterations"] and info["status"][c] == want["status"], what
    same(steps[0], y, what)
    mean0 = gls_spec.prologue(y, dy)[2]
    total = numpy.zeros(len(y))
    slack = numpy.zeros(len(y))
    for j in range(K):
        if j >= ran:
            assert numpy.all(terms[j]["status"] == 2.0) and numpy.isnan(terms[j]["frequency"]).all(), (what, j)
            assert numpy.isnan(sums[j]).all()
            for h in range(H):
                same(steps[j * H + h], steps[K * H], (what, j, h, "a row that stopped stays"))
            continue
        head = terms[j][0]
        power = spec.spectrum(t, steps[j * H], f, dy)[0]
        k = spec.pick(power)
        assert int(head["index"]) == k == int(want["terms"][j][0]["index"]), (what, j)
        assert head["frequency_grid"] == f[k] and head["power_peak"] >= case.min_power
        assert numpy.isnan(head["power_left"]) == (k == 0) and numpy.isnan(head["power_right"]) == (k == len(f) - 1)
        fstar = spec.refine(f, k, head["power_left"], head["power_peak"], head["power_right"])
        for h in range(H):
            term, row = terms[j][h], steps[j * H + h]
            tag = (what, j, h)
            for name in ("index", "frequency_grid", "power_left", "power_peak", "power_right"):
                same(term[name], head[name], tag + (name,))
            fh = numpy.float64(h + 1) * fstar
            same(term["frequency"], fh, tag + ("f*",))
            w, a, mean, YY = spec.lane_prologue(row, dy)
            same(term["mean"], mean, tag + ("mean",))
            same(term["variance"], YY, tag + ("variance",))
            exact = spec.exact_six_sums(t, w, a, fh)
            reach = numpy.array([fh, 2.0 * fh])
            bound = numpy.repeat([gls_spec.sum_bound(t, a, reach)[0], gls_spec.sum_bound(t, w, reach)[0]], [2, 4])
            assert numpy.all(numpy.abs(sums[j][h] - exact) <= bound), tag + ("sums", numpy.abs(sums[j][h] - exact) / bound)
            p, amplitude, phase, ca, sa = spec.fit_epilogue(sums[j][h], YY)
            for name, value in (("power", p), ("amplitude", amplitude), ("ca", ca), ("sa", sa), ("C", sums[j][h][2]), ("S", sums[j][h][3])):
                same(term[name], value, tag + (name,))
            assert term["status"] == 0.0 and abs(term["phase"] - phase) <= PHASE_TOL, tag
            after, q = spec.subtraction(t, row, fh, term["ca"], term["sa"], term["C"], term["S"])
            bound = spec.subtract_bound(row, after, term["ca"], term["sa"])
            off = numpy.abs(steps[j * H + h + 1] - after)
            assert numpy.all(off <= bound), tag + ("subtraction", float(numpy.max(off / bound)))
            slack = slack + 8.0 * EPS * (abs(term["ca"]) + abs(term["sa"])) + numpy.spacing(numpy.maximum(numpy.abs(total), numpy.abs(total + q)))
            total = total + q
    same(flat[c], y / trend[c], what + " flat")
    if ran == 0:
        same(trend[c], numpy.full(len(y), mean0), what + " trend")
    else:
        off = numpy.abs(trend[c] - (mean0 + total))
        assert numpy.all(off <= slack + numpy.spacing(numpy.maximum(numpy.abs(trend[c]), numpy.abs(mean0 + total)))), (what, "trend", float(off.max()))
    return ran


@pytest.mark.parametrize("name", ["n255_c3", "n256_c3_dy_h2", "n257_c40", "n700_gap_c40_dy_h2", "lds_side", "global_side",
                                  "one_stops", "edges"])
def test_every_step_against_the_statement(gpu, name):
    case = prewhiten_cases.cases()[name]
    want = prewhiten_cases.statement(name)
    flat, trend, info = run(gpu, case)
    ran = [check_curve(case, c, flat, trend, info, want[c]) for c in range(len(case.y))]
    # the plain call (no test outputs) and the survey call return the same rows
    same(gpu.prewhiten(case.t, case.y, case.f, case.n_terms, case.harmonics, case.min_power, dy=case.dy), flat, name)
    got = survey.prewhiten_batch(case.t, case.y, case.n_terms, case.harmonics, case.min_power, frequencies=case.f,
                                 dy_batch=case.dy, return_trend=True, return_terms=True, context=gpu)
    same(got[0], flat, name)
    same(got[1], trend, name)
    assert got[2]["terms"].tobytes() == info["terms"].tobytes() and list(got[2]["n_iterations"]) == ran
    if name == "one_stops":
        assert ran == [3, 1, 3] and list(info["status"]) == [0.0, 1.0, 0.0]
    if name == "edges":
        F = len(case.f)
        assert list(info["status"]) == [2.0, 0.0, 0.0, 0.0] and ran == [0, 1, 1, 1]
        same(flat[0], case.y[0] / 0.75, "constant row")
        first, last, inner = (info["terms"][c][0][0] for c in (1, 2, 3))
        assert first["index"] == 0 and first["frequency"] == case.f[0]
        assert last["index"] == F - 1 and last["frequency"] == case.f[-1]
        assert inner["frequency"] != inner["frequency_grid"]


def test_two_slabs(gpu):
    """4097 curves, eight distinct ones repeated: every copy equals its original bit for bit, across the slab's edge too."""
    case = prewhiten_cases.cases()["two_slabs"]
    want = prewhiten_cases.statement("two_slabs")
    flat, trend, info = run(gpu, case)
    for c in range(case.distinct):
        check_curve(case, c, flat, trend, info, want[c])
    rows = numpy.arange(len(case.y)) % case.distinct
    same(flat, flat[rows], "flat")
    same(trend, trend[rows], "trend")
    same(info["steps"], info["steps"][:, rows], "steps")
    assert info["terms"].tobytes() == info["terms"][rows].tobytes()
    assert numpy.array_equal(info["n_iterations"], info["n_iterations"][rows]) and numpy.all(info["n_iterations"] == 2)


def test_min_power_one_removes_nothing(gpu):
    case = prewhiten_cases.cases()["n255_c3"]
    flat, trend, info = gpu.prewhiten(case.t, case.y, case.f, 3, 1, 1.0, return_trend=True, debug=True)
    assert numpy.all(info["status"] == 1.0) and numpy.all(info["n_iterations"] == 0) and numpy.all(info["terms"]["status"] == 2.0)
    for c in range(len(case.y)):
        mean = gls_spec.prologue(case.y[c])[2]
        same(trend[c], numpy.full(case.y.shape[1], mean), c)
        same(flat[c], case.y[c] / mean, c)
    same(info["steps"], numpy.broadcast_to(case.y, info["steps"].shape), "steps")


def test_argument_refusals_of_the_c_entry(gpu):
    lib = _lib.load()
    case = prewhiten_cases.cases()["n255_c3"]
    t, y, f = case.t, numpy.ascontiguousarray(case.y), case.f
    n_c, n = y.shape
    flat = numpy.empty_like(y)
    terms = numpy.zeros((n_c, 32, 8), dtype=_lib.PREWHITEN_DTYPE)
    iters, status = numpy.zeros(n_c, dtype=numpy.int64), numpy.zeros(n_c)
    dp, vp = _lib._dp, terms.ctypes.data_as(_lib.ctypes.c_void_p)

    def c_call(tt=t, nn=n, curves=n_c, ff=f, F=len(f), K=3, H=1, low=0.0):
        return lib.tls_prewhiten(gpu._h, dp(tt), dp(y), None, nn, curves, dp(ff), F, K, H, low, dp(flat), None, vp,
                                 _lib._ip(iters), dp(status), None, None)

    assert c_call() == 0
    for kw in (dict(K=0), dict(K=33), dict(H=0), dict(H=9), dict(low=-1e-9), dict(low=1.0 + 1e-9), dict(low=numpy.nan),
               dict(nn=2), dict(curves=-1), dict(F=0), dict(tt=t[::-1].copy()), dict(ff=-f),
               dict(ff=numpy.where(numpy.arange(len(f)) == 3, numpy.inf, f))):
        assert c_call(**kw) == -1, kw
    assert c_call(curves=0) == 0                         # a no-op
    assert c_call(K=32, H=8, low=1.0) == 0               # the limits themselves
    for kw in (dict(n_terms=0), dict(harmonics=9), dict(min_power=2.0)):
        with pytest.raises(ValueError, match="prewhiten"):
            survey.prewhiten_batch(t, y, frequencies=f, context=gpu, **kw)
    same(gpu.prewhiten(t, y[0], f, 3, 1, 0.0), gpu.prewhiten(t, y, f, 3, 1, 0.0)[0], "one row as [n]")


# ---- the survey calls with detrend=Prewhiten(...)

def _pulsating_batch(n_curves):
    t, base = synthetic.light_curve(20.0, 24, 3e-4, per=3.3, rp=0.05, a=10)
    rng = numpy.random.default_rng(5)
    raw = numpy.array([base * (1.0 + 4e-3 * numpy.sin(2.0 * numpy.pi * ((5.0 + 0.7 * s) * t + 0.1 * s))) for s in range(n_curves)])
    raw *= 1.0 + 1e-5 * rng.standard_normal(raw.shape)
    return t, raw, dict(period_min=2.0, period_max=5.0, oversampling_factor=2)


def _same_summary(got, want):
    assert got.dtype == want.dtype
    for k in want.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), k


PW = survey.Prewhiten(2, 1, None, 2.0, None)


def _prewhitened(gpu, t, raw):
    grid, k, h, low = survey._prewhiten_step(t, PW, len(t))
    return survey.prewhiten_batch(t, raw, k, h, low, frequencies=grid, context=gpu)


def test_power_batch_detrend(gpu):
    t, raw, kw = _pulsating_batch(3)
    flat = _prewhitened(gpu, t, raw)
    assert numpy.std(flat) < 0.5 * numpy.std(raw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.power_batch(t, raw, detrend=PW, with_arrays=True, context=gpu, **kw)
        want = survey.power_batch(t, flat, with_arrays=True, context=gpu, **kw)
        _same_summary(got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert numpy.asarray(a).tobytes() == numpy.asarray(b).tobytes()
        assert survey.power_batch(t, raw, context=gpu, **kw)[0]["SDE"].tobytes() != got[0]["SDE"].tobytes()
        # in a tuple with the biweight
        both = (PW, survey.Biweight(1.5))
        got = survey.power_batch(t, raw, detrend=both, context=gpu, **kw)
        want = survey.power_batch(t, survey.biweight_batch(t, flat, 1.5, context=gpu), context=gpu, **kw)
        _same_summary(got[0], want[0])
        spectrum = survey.lomb_scargle(t, raw, detrend=PW, context=gpu)
        assert spectrum["power"].tobytes() == survey.lomb_scargle(t, flat, context=gpu)["power"].tobytes()


def test_injection_recovery_detrend(gpu):
    t, _, kw = _pulsating_batch(1)
    base = (1.0 + 4e-3 * numpy.sin(2.0 * numpy.pi * 5.0 * t)) * (1.0 + 3e-4 * numpy.random.default_rng(6).standard_normal(len(t)))
    inj = survey.injection_grid(t, [3.0], [0.05, 0.08], per_cell=2, seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec, summary, rows = survey.injection_recovery(t, base, inj, detrend=PW, return_rows=True, context=gpu, **kw)
        injected = gpu.inject_transits(t, base, survey.injection_constants(inj), *survey._injection_law(None, None, kw)[1:])[0]
        same(rows, _prewhitened(gpu, t, injected), "rows")
        _same_summary(summary, survey.power_batch(t, rows, context=gpu, **kw)[0])
