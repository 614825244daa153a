"""Template tables of every shape the search can be handed, for test_template_shapes_host.py and test_template_shapes.py:
input_scales.py's two series at offset 0 (the first 1500 points of k2_90d; the gapped one of any length), each searched
with a table that is NOT the default planet's.

From power()'s keywords, through synthetic.search_inputs(t, flux, dy, **kw):

    grazing      transit_template="grazing"
    box          transit_template="box"
    grazing_ld   transit_template="grazing", u=[1.6, -0.6]: a limb BRIGHTENED star, overshoot up to 2.33
    ecc_full     ecc=0.3, w=140: asymmetric rows (ingress and egress differ by 7e-3), every row as long as its width
    ecc_short    ecc=0.6, w=20: asymmetric by 0.46, and EVERY row one sample shorter than its width (the stability cut-off
                 trims the slow side of the transit: template.get_cache)
    grazing_ecc  transit_template="grazing", ecc=0.7, w=10: rows up to 3 (1500 points) to 5 (2900) samples short

Synthetic tables keep the default table's widths and durations and replace row r (length L) by 1 - 0.5 f(x),
x = (j + 0.5) / L * 2 - 1, overshoot = 1 / (2 - mean / min) as template.get_cache forms it:

    flat         f = 1: every tap equal, overshoot exactly 1
    skew         f = ((x + 1) / 1.6)^2 for x < 0.6, ((1 - x) / 0.4)^2 beyond: the bottom at 0.8 of the row
    cusp3        f = (1 - |x|)^3: sum q - overshoot sum q^2 < 0 on about half the rows, the rows the pruning bound does not
                 hold for (build_widths: prunable = 0) beside rows it holds for

The default planet's table and the two presets are symmetric to 3e-13: a kernel that reads a row backwards, or pairs tap j with
sample d - 1 - j, returns the same numbers on them.  On skew and the eccentric tables it does not (test_template_shapes_host.py
asserts by how much).  Widths do not depend on the shape, so plan_edges' edge lengths hold for every shape; what a short row
changes in the plan is restated in plan_edges.expected_plan (short_rows)."""
import functools

import numpy

import input_scales as S
import search_spec
from tls_amd import synthetic, template

KEYWORD_SHAPES = {
    "grazing": dict(transit_template="grazing"),
    "box": dict(transit_template="box"),
    "grazing_ld": dict(transit_template="grazing", u=[1.6, -0.6]),
    "ecc_full": dict(ecc=0.3, w=140),
    "ecc_short": dict(ecc=0.6, w=20),
    "grazing_ecc": dict(transit_template="grazing", ecc=0.7, w=10),
}


def _skew(x):
    return numpy.where(x < 0.6, ((x + 1) / 1.6) ** 2, ((1 - x) / 0.4) ** 2)


SYNTHETIC_SHAPES = {
    "flat": lambda x: numpy.ones_like(x),
    "skew": _skew,
    "cusp3": lambda x: (1 - numpy.abs(x)) ** 3,
}
SHAPES = tuple(KEYWORD_SHAPES) + tuple(SYNTHETIC_SHAPES)
SHORT_SHAPES = ("ecc_short", "grazing_ecc")          # len(row) < width on every row
PRESETS = ("grazing", "box")


def synthetic_table(default_inp, f):
    """The default table's widths and durations with every row replaced by 1 - 0.5 f(x)."""
    overview = default_inp["overview"].copy()
    rows = []
    for r, old in enumerate(default_inp["rows"]):
        L = len(old)
        x = (numpy.arange(L) + 0.5) / L * 2 - 1
        row = 1 - 0.5 * f(x)
        rows.append(row)
        overview["overshoot"][r] = 1 / (2 - numpy.mean(row) / numpy.min(row))
    return template.TemplateTable(overview, rows), overview, rows


def _shaped(shape, t, flux, dy, kw):
    inp = synthetic.search_inputs(t, flux, dy, **dict(kw, **KEYWORD_SHAPES.get(shape, {})))
    if shape in SYNTHETIC_SHAPES:
        inp["table"], inp["overview"], inp["rows"] = synthetic_table(inp, SYNTHETIC_SHAPES[shape])
    return inp


@functools.lru_cache(maxsize=None)
def case(shape, series, dy_name, n_periods, n=None, margin=None):
    """search_inputs of input_scales' series at offset 0 under a shape ("default": the default planet), with its chosen
    periods ("selected"); margin: another T0_fit_margin (0.1: strided rows)."""
    kind, R = [(k, r) for name, k, r in S.DY_CASES if name == dy_name][0]
    if series == "k2":
        t, flux, kw = S.k2_prefix(0.0, n=n or 1500)
        extra = (10.123,)
    else:
        t, flux, kw = S.gapped(0.0, n=n or 2900)
        extra = (kw.pop("_true_period"),)
    if margin is not None:
        kw["T0_fit_margin"] = margin
    inp = _shaped(shape, t, flux, S.make_dy(len(t), kind, R), kw)
    inp["selected"] = S.pick_periods(inp["periods"], n_periods, extra)
    return inp


@functools.lru_cache(maxsize=None)
def statement(shape, series, dy_name, n_periods, n=None, variant=None):
    """The long-double statement of the case's search (computed once a session, shared, never changed); variant:
    "reverse_rows" or "pad_short_rows" (search_spec.search_period)."""
    inp = case(shape, series, dy_name, n_periods, n)
    return search_spec.search(inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"],
                              **({variant: True} if variant else {}))


@functools.lru_cache(maxsize=None)
def noisy_case(shape, sigma, n=1500, every=3):
    """The first n points of k2_90d at noise level sigma under a shape, every third period of its grid."""
    t, flux, kw = synthetic.config("k2_90d", sigma=sigma)
    inp = _shaped(shape, t[:n], flux[:n].copy(), None, kw)
    inp["selected"] = numpy.ascontiguousarray(inp["periods"][::every])
    return inp


def k_mono(table):
    """sum q - overshoot sum q^2 of every row: the pruning bound holds for a row where it is >= 0 (build_widths)."""
    out = []
    for r in range(table.n_rows):
        q = 1 - table.row(r)
        out.append(float(q.sum() - table.overshoot[r] * (q * q).sum()))
    return numpy.array(out)


def short_by(table):
    """width - len(row) of every row."""
    return numpy.asarray(table.width) - numpy.asarray(table.length)


def asymmetry(table):
    """max |row - reversed row| over the table."""
    return max(float(numpy.max(numpy.abs(table.row(r) - table.row(r)[::-1]))) for r in range(table.n_rows))
