"""What tests/test_multi_planet_host.py and tests/test_multi_planet.py share: the two-planet injection the multi-planet search
was measured on (DESIGN.md "Multi-planet search") and the candidate layouts remove_transits is compared on."""
import numpy

import transit_fit_spec as fit_spec
from tls_amd import survey, transit_model

U = [0.4804, 0.1867]
T = numpy.linspace(0.0, 30.0, 1440)
SIGMA = 3e-4
PLANET_B = dict(t0=0.7, per=2.1, rp=0.08, a=6.9)
PLANET_C = dict(t0=1.3, per=3.7, rp=0.045, a=10.0)
SEARCH = dict(period_min=1, period_max=8, oversampling_factor=2)
_PROFILES = {}


def profile(M=1024, k_rows=None):
    key = (M, None if k_rows is None else tuple(k_rows))
    if key not in _PROFILES:
        _PROFILES[key] = survey.transit_profile(k_rows, M, u=U)
    return _PROFILES[key]


def dip(planet, t=T):
    return transit_model.light_curve(t, planet["t0"], planet["per"], planet["rp"], planet["a"], 90, 0, 90, U, "quadratic")


def curve(seed, planets=(PLANET_B, PLANET_C)):
    """White noise of SIGMA from numpy.random.default_rng(seed) on the product of the planets' dips."""
    y = numpy.ones(len(T))
    for planet in planets:
        y = y * dip(planet)
    return y + numpy.random.default_rng(seed).normal(0, SIGMA, len(T))


def batch():
    """The recovery batch: three two-planet curves, one with the first planet alone, four of noise alone."""
    return numpy.array([curve(s) for s in (0, 1, 2)] + [curve(3, (PLANET_B,))] + [curve(s, ()) for s in (100, 101, 102, 103)])


def layout(n, M, S, offset=0.0, many_epochs=False):
    """The candidate layout of the device comparison on 5 curves of n points at 48 a day: curve 0 without a candidate, curve 1
    with one, curve 2 with two whose transits coincide at an epoch, curve 3 with a grazing one (bb just under e2), curve 4
    with a skipped one in front of a valid one.  A dict of remove_transits_spec's arguments."""
    t = offset + numpy.arange(n) / 48.0
    span = n / 48.0
    k_rows, table = profile(M, numpy.geomspace(0.03, 0.15, 9))
    rng = numpy.random.default_rng(n + M + S)
    y = 1.0 + rng.normal(0, 1e-3, (5, n))
    short = span / 40.5 if many_epochs else span / 3.7
    first = offset + 0.31 * short
    graze_row = 6
    e1 = 1.0 + k_rows[graze_row]
    cand = [
        # curve, P, T0, row, A, b, T, c0
        (1, short, first, 4, 0.9, 0.3 * (1.0 + k_rows[4]), 0.12 if not many_epochs else 0.25 * short, 0.004),
        (2, span / 2.9, offset + 0.4 * span / 2.9, 2, 1.1, 0.0, 0.15, -0.003),
        (2, span / 1.45, offset + 0.4 * span / 2.9, 7, 0.7, 0.6 * (1.0 + k_rows[7]), 0.2, 0.0),     # (every other epoch of the one above)
        (3, span / 3.3, offset + 0.2, graze_row, 1.0, numpy.nextafter(e1, 0.0) * (1.0 - 2.0 ** -40), 0.18, 0.0),
        (4, span / 3.1, offset + 0.1, 3, numpy.nan, 0.1, 0.1, 0.0),
        (4, span / 3.1, offset + 0.1, 3, 0.8, 0.1, 0.1, 0.001),
    ]
    columns = list(zip(*cand))
    return dict(t=t, y=y, curve=numpy.array(columns[0], dtype=numpy.int64), P=numpy.array(columns[1]), T0=numpy.array(columns[2]),
                row=numpy.array(columns[3], dtype=numpy.int64), A=numpy.array(columns[4]), b=numpy.array(columns[5]),
                T=numpy.array(columns[6]), c0=numpy.array(columns[7]), k_rows=k_rows, profile=table,
                sub=fit_spec.sub_offsets(1 / 48.0, S))
