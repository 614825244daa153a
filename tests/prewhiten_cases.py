"""The inputs of the pre-whitening tests: what tests/test_prewhiten.py sends through the device, and what
tests/test_prewhiten_host.py checks the premise of (in every iteration of every input the statement's highest power stands clear
of every other power of the grid).  Everything is generated from fixed seeds."""
import collections
import functools

import numpy

import prewhiten_spec

Case = collections.namedtuple("Case", ("t", "y", "dy", "f", "n_terms", "harmonics", "min_power", "distinct"))

SPAN = 20.0   # days
MIN_GAP = 1e-6   # the relative gap the GPU tests rest on (the issue's condition)


def times(n, seed, gap=None):
    """n ascending, slightly irregular time stamps over SPAN days; gap=(lo, hi): none inside it (the count stays n)."""
    rng = numpy.random.default_rng(seed)
    t = numpy.linspace(0.0, SPAN, n) + rng.uniform(-0.2, 0.2, n) * SPAN / n
    if gap is not None:
        t = numpy.where(t > gap[0], t + (gap[1] - gap[0]), t) * SPAN / (SPAN + gap[1] - gap[0])
    return 2457000.25 + numpy.sort(t)


def grid(F, lo=0.05, step=0.01):
    return lo + step * numpy.arange(F)


def pulsator(t, rng, f_lo, f_hi, amplitudes=(5e-3, 3e-3, 2e-3), noise=3e-4, dy=None):
    """1 + sinusoids of the amplitudes (each within 20 %) at frequencies at least 0.15 apart in [f_lo, f_hi] + noise."""
    while True:
        fs = rng.uniform(f_lo, f_hi, len(amplitudes))
        if len(fs) < 2 or numpy.min(numpy.diff(numpy.sort(fs))) > 0.15:
            break
    y = numpy.ones(len(t))
    for f, amp in zip(fs, amplitudes):
        y += amp * rng.uniform(0.8, 1.2) * numpy.sin(2.0 * numpy.pi * (f * (t - t[0]) + rng.uniform()))
    sigma = noise if dy is None else dy
    return y + sigma * rng.standard_normal(len(t))


def batch(n, n_curves, F, seed, with_dy, n_terms, harmonics, gap=None, step=0.01, min_power=0.0, single=()):
    """n_curves pulsators of three signals; the curves of `single` carry one signal only."""
    rng = numpy.random.default_rng(seed)
    t = times(n, seed + 1000, gap)
    f = grid(F, step=step)
    dy = rng.uniform(2e-4, 4e-4, (n_curves, n)) if with_dy else None
    f_hi = min(f[-1] - 0.2, 3.0)
    y = numpy.array([pulsator(t, rng, 0.3, f_hi, (5e-3,) if c in single else (5e-3, 3e-3, 2e-3), dy=None if dy is None else dy[c])
                     for c in range(n_curves)])
    return Case(t, y, dy, f, n_terms, harmonics, min_power, None)


def _two_slabs():
    """4097 curves, one more than a slab: eight distinct ones, repeated."""
    base = batch(40, 8, 40, 7, False, 2, 1, step=0.02)
    rows = numpy.arange(4097) % 8
    return base._replace(y=numpy.ascontiguousarray(base.y[rows]), distinct=8)


def _edges():
    """Curve 0: a constant row (256 points: 1 / 256 and the sum are exact, so the mean is the constant and YY is 0).  Curve 1: a
    signal below the grid (the pick is the first frequency).  Curve 2: a signal above it (the last).  Curve 3: three signals."""
    case = batch(256, 4, 120, 11, False, 2, 1)
    t, f = case.t, case.f
    y = case.y.copy()
    y[0] = 0.75
    rng = numpy.random.default_rng(12)
    y[1] = 1.0 + 5e-3 * numpy.sin(2.0 * numpy.pi * (f[0] - 0.012) * (t - t[0]) + 0.3) + 3e-4 * rng.standard_normal(len(t))
    y[2] = 1.0 + 5e-3 * numpy.sin(2.0 * numpy.pi * (f[-1] + 0.012) * (t - t[0]) + 1.1) + 3e-4 * rng.standard_normal(len(t))
    return case._replace(y=y, n_terms=1)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    return {
        "n255_c3": batch(255, 3, 333, 1, False, 3, 1),
        "n256_c3_dy_h2": batch(256, 3, 333, 2, True, 2, 2),
        "n257_c40": batch(257, 40, 333, 3, False, 3, 1),
        "n700_gap_c40_dy_h2": batch(700, 40, 333, 4, True, 2, 2, gap=(8.0, 9.5)),
        "two_slabs": _two_slabs(),
        "lds_side": batch(6144, 2, 100, 5, True, 2, 1, step=0.03),
        "global_side": batch(6145, 2, 100, 6, False, 2, 2, step=0.03),
        # curve 1 carries one signal and stops behind it; the others run all three iterations
        "one_stops": batch(300, 3, 333, 8, False, 3, 1, min_power=0.2, single=(1,)),
        "edges": _edges(),
    }


@functools.lru_cache(maxsize=None)
def statement(name):
    """The statement's run of every distinct curve of a case: a list of prewhiten_spec.prewhiten's dicts."""
    case = cases()[name]
    count = case.distinct or len(case.y)
    return [prewhiten_spec.prewhiten(case.t, case.y[c], case.f, None if case.dy is None else case.dy[c], case.n_terms,
                                     case.harmonics, case.min_power) for c in range(count)]
