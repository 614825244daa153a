"""Inputs at the scales survey data have, for test_search_spec_host.py and test_input_scales.py: time stamps at a Julian-date
offset (0; BTJD 1325; full JD 2457000, where a double resolves 4.7e-10 d) and per-point uncertainties of wide range (a few
cadences de-weighted by a factor R, a few R times more precise than the rest).

Two series: the first 1500 points of the k2_90d configuration (31 d, three transits of the injected planet), and a gapped
one of any length on plan_edges.light_curve's pattern -- one point in seven off the cadence grid, a gap of 37.37 cadences,
four exact ties, a transit centred on phase 0 of its period AT THE OFFSET (its window wraps the phase origin of the fold)."""
import functools

import numpy

import search_spec
from tls_amd import synthetic

OFFSETS = (0.0, 1325.0, 2457000.0)
SIGMA = 50e-6
N_PRECISE, N_DOWN = 5, 15
# (name, kind, R): None -> uniform weights; "uniform" -> the factor-2 spread; the three wide-range kinds
DY_CASES = ((("none", None, 1.0), ("uniform", "uniform", 1.0))
            + tuple(("%s_R%g" % (kind, R), kind, R) for kind in ("down", "precise", "both") for R in (10.0, 1e2, 1e3))
            + (("both_R10000_nofit", "both", 1e4),))   # mean-normalised dy makes S0 exceed N: (almost) nothing is fitted


def k2_prefix(offset, seed=0, n=1500):
    t, flux, kw = synthetic.config("k2_90d", seed=seed)
    return t[:n] + offset, flux[:n].copy(), kw


def gapped(offset, n=2900, cadence=48.0, sigma=SIGMA):
    rng = numpy.random.RandomState(100003 + n)
    k = numpy.arange(n, dtype=numpy.float64)
    k[(2 * n) // 5:] += 37.37
    off = rng.rand(n) < 1.0 / 7.0
    k[off] += rng.uniform(-0.3, 0.3, int(off.sum()))
    t = offset + (3.0 + k / cadence)
    for i in (n // 9, n // 2 + 1, n - 3):
        t[i + 1] = t[i]
    t[n // 3 + 2] = t[n // 3]
    true_period = min(2.0 + 1.0 / 7.0, (t.max() - t.min()) / 3.3)
    phase = t / true_period - numpy.floor(t / true_period)
    flux = 1.0 + rng.normal(0, sigma, n)
    flux[(phase < 0.01) | (phase > 0.99)] -= 3 * sigma
    return t, flux, dict(_true_period=true_period)


def make_dy(n, kind, R, seed=5):
    """dy of a case (None for uniform weights): uniform(0.7, 1.4) sigma, five points divided by R and/or fifteen multiplied."""
    if kind is None:
        return None
    rng = numpy.random.RandomState(seed)
    dy = rng.uniform(0.7, 1.4, n) * SIGMA
    idx = rng.choice(n, N_PRECISE + N_DOWN, replace=False)
    if kind in ("precise", "both"):
        dy[idx[:N_PRECISE]] /= R
    if kind in ("down", "both"):
        dy[idx[N_PRECISE:]] *= R
    return dy


def pick_periods(grid, count, extra=()):
    """`count` periods spread over the grid, the grid periods nearest to `extra` among them."""
    at = set(numpy.round(numpy.linspace(0, len(grid) - 1, count - len(extra))).astype(int).tolist())
    for p in extra:
        near = numpy.argsort(numpy.abs(grid - p))
        at.add(int([i for i in near if int(i) not in at][0]))
    return numpy.ascontiguousarray(grid[sorted(at)])


@functools.lru_cache(maxsize=None)
def case(series, offset, dy_name, n_periods, n=None):
    """search_inputs of a case with its chosen periods ("selected")."""
    kind, R = [(k, r) for name, k, r in DY_CASES if name == dy_name][0]
    if series == "k2":
        t, flux, kw = k2_prefix(offset, n=n or 1500)
        extra = (10.123,)
    else:
        t, flux, kw = gapped(offset, n=n or 2900)
        extra = (kw.pop("_true_period"),)
    inp = synthetic.search_inputs(t, flux, make_dy(len(t), kind, R), **kw)
    inp["selected"] = pick_periods(inp["periods"], n_periods, extra)
    return inp


@functools.lru_cache(maxsize=None)
def statement(series, offset, dy_name, n_periods, n=None):
    """The long-double statement of the case's search (computed once a session, shared, never changed)."""
    inp = case(series, offset, dy_name, n_periods, n)
    return search_spec.search(inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])


def rows_agree(row, spec, what, cap=0.10, min_gap=1e-8):
    """Rows equal wherever the statement's other-row gap exceeds min_gap; at most `cap` of the periods left out."""
    decided = spec["row_gap"] > min_gap
    assert (~decided).sum() <= cap * len(decided), (what, int((~decided).sum()), len(decided))
    numpy.testing.assert_array_equal(numpy.asarray(row)[decided], spec["row"][decided], err_msg=str(what))
    return int((~decided).sum())
