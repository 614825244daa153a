"""The CPU side of the template-shape tests (template_shapes.py): the goldens of the unmodified reference under the two
presets and an eccentric orbit, the CPU oracle against them, and the long-double statement (search_spec.py, extended to
rows shorter than their width) against the oracle on every shape.  No GPU.

Asserted per shape x {k2 prefix 1500 points, gapped 2900} x 14 periods: the oracle's chi2 within RTOL_CONTRACT of the
statement (test_search_spec_host.py's bound), rows equal wherever the statement's other-row gap exceeds 1e-8 (rows_agree's
cap on the periods left out), depth within 1e-12, chi2 == n in the same periods, the argmin period, and both work counters.

Measured here (largest |oracle - statement| / statement over a case's 14 periods; no period left out of the row
comparison on any shape -- the smallest row gap is 7.3e-7 --; argmin gaps 3.1e-2 to 1.4e-1):

    shape        rows short by     k2 prefix    gapped
    grazing      0                 1.1e-14      1.4e-14
    box          0                 6.3e-15      6.0e-15
    grazing_ld   0                 1.6e-14      7.3e-15
    ecc_full     0                 1.7e-14      8.4e-15
    ecc_short    1 (every row)     1.2e-14      6.3e-15
    grazing_ecc  1 to 3 / 1 to 5   1.3e-14      1.2e-14
    flat         0                 2.6e-15      4.7e-15
    skew         0                 1.2e-14      1.3e-14
    cusp3        0                 1.7e-14      1.6e-14

Reversed rows move the k2 statement by 1.7e-15 (grazing), 3.4e-16 (box), 1.2e-5 (ecc_full), 1.3e-3 (ecc_short), 1.2e-3
(grazing_ecc) and 9.3e-3 (skew, 10 of 14 rows change); a short row padded with q = 0 is 6.8e-3 to 9.8e-3 from the statement.

The module also asserts what gives the GPU tests (test_template_shapes.py) their power: how far the statement moves when every
row is read backwards -- less than 1e-12 on the presets (the suite could not see such a kernel before), more than 1e-5 on
skew and the two short shapes, more than 1e-6 on ecc_full --, that cusp3 has rows on both sides of the pruning bound's
validity, that the short shapes are short on every row, and that valuing a short row as if it were padded with q = 0 sits
more than 1e-3 from the statement."""
import numpy
import pytest

import plan_edges as pe
import search_spec
import template_shapes as T
from conftest import GOLDEN, load_search_golden, oracle_search
from test_gpu_parity import RTOL_CONTRACT

N_PERIODS = 14
DEPTH_ATOL = 1e-12
SHAPE_GOLDENS = ("grazing", "box", "ecc")          # search_<name>.npz, power_<name>.npz (tools/gen_golden.py shapes)
GOLDEN_KEYWORDS = {"grazing": "grazing", "box": "box", "ecc": "ecc_short"}
SERIES = ("k2", "gapped")
MEASURED = {}


@pytest.mark.parametrize("name", SHAPE_GOLDENS)
def test_oracle_matches_reference_search_period(oracle_lib, name):
    """test_oracle_golden's assertions on the three template-shape goldens."""
    g, table, params = load_search_golden(name)
    chi2, row, depth, counters = oracle_lib.search(
        g["t"], g["y"], g["dy"], g["periods"], table, params["transit_depth_min"],
        params["R_star_min"], params["R_star_max"], params["M_star_min"], params["M_star_max"],
        params["T0_fit_margin"])
    numpy.testing.assert_allclose(chi2, g["chi2"], rtol=1e-11, atol=0)
    numpy.testing.assert_array_equal(row, g["row"])
    numpy.testing.assert_allclose(depth, g["depth"], rtol=0, atol=1e-13)
    assert counters[0] > 0


@pytest.mark.parametrize("name", SHAPE_GOLDENS)
def test_statement_against_the_unmodified_reference(name):
    """test_search_spec_host's assertions on the three goldens: the ecc one has every row one sample short."""
    g, table, params = load_search_golden(name)
    assert bool((table.length < table.width).all()) == (name == "ecc")
    spec = search_spec.search(g["t"], g["y"], g["dy"], g["periods"], table, params)
    T.S.rows_agree(g["row"], spec, name)
    numpy.testing.assert_allclose(g["depth"], spec["depth"], rtol=0, atol=DEPTH_ATOL)
    numpy.testing.assert_array_equal(numpy.isfinite(g["chi2"]), numpy.isfinite(spec["chi2"]))
    assert search_spec.distance(g["chi2"], spec["chi2"]) <= 1e-11
    numpy.testing.assert_array_equal(g["chi2"] == len(g["t"]), spec["chi2"] == len(g["t"]))


@pytest.mark.parametrize("name", SHAPE_GOLDENS)
def test_keyword_table_equals_the_references(name):
    """The template table search_inputs builds under the case's keywords against the reference's own (transit.get_cache)."""
    import json
    g, table, _ = load_search_golden(name)
    kwargs = json.loads(str(g["kwargs_json"]))
    assert {k: v for k, v in kwargs.items() if k in ("transit_template", "ecc", "w")} == \
        {k: v for k, v in T.KEYWORD_SHAPES[GOLDEN_KEYWORDS[name]].items()}
    inp = T.synthetic.search_inputs(g["t"], g["y"], None, **kwargs)
    for key in ("offset", "length", "width"):
        numpy.testing.assert_array_equal(getattr(inp["table"], key), getattr(table, key), err_msg=key)
    numpy.testing.assert_allclose(inp["table"].values, table.values, rtol=0, atol=1e-14)
    numpy.testing.assert_allclose(inp["table"].overshoot, table.overshoot, rtol=1e-13, atol=0)
    numpy.testing.assert_allclose(inp["table"].duration, g["tmpl_duration"], rtol=1e-14, atol=0)


def test_fixtures_are_no_larger_than_the_largest_of_their_kind():
    import os
    for kind in ("search", "power"):
        old = [os.path.getsize(os.path.join(GOLDEN, "%s_%s.npz" % (kind, n)))
               for n in (("small", "weights", "stride", "margin0", "nofit", "gap_ties") if kind == "search" else ("small", "weights", "nofit"))]
        for name in SHAPE_GOLDENS:
            assert os.path.getsize(os.path.join(GOLDEN, "%s_%s.npz" % (kind, name))) <= max(old), (kind, name)


@pytest.mark.parametrize("series", SERIES)
@pytest.mark.parametrize("shape", T.SHAPES)
def test_oracle_against_the_statement(oracle_lib, shape, series):
    what = (shape, series)
    inp = T.case(shape, series, "none", N_PERIODS)
    n = len(inp["t"])
    spec = T.statement(shape, series, "none", N_PERIODS)
    chi2, row, depth, counters = oracle_search(oracle_lib, inp, periods=inp["selected"])
    dist = search_spec.distance(chi2, spec["chi2"])
    MEASURED[what] = dist
    print("%-12s %-7s oracle off the statement %.2e   smallest row gap %.1e   argmin gap %.1e   rows short by %d to %d"
          % (shape, series, dist, spec["row_gap"].min(), spec["period_gap"], T.short_by(inp["table"]).min(),
             T.short_by(inp["table"]).max()))
    assert T.S.rows_agree(row, spec, what) == 0
    numpy.testing.assert_allclose(depth, spec["depth"], rtol=0, atol=DEPTH_ATOL, err_msg=str(what))
    assert numpy.isfinite(spec["chi2"]).all() and dist <= RTOL_CONTRACT, (what, dist)
    numpy.testing.assert_array_equal(chi2 == n, spec["chi2"] == n, err_msg=str(what))
    assert spec["period_gap"] > 1e-8 and int(numpy.argmin(chi2)) == spec["argmin"], what
    assert int(counters[1]) == int(spec["evaluated_cells"].sum()), what
    assert int(counters[2]) == int(spec["inner_steps"].sum()), what
    assert (spec["chi2"] < n).sum() >= len(row) - len(row) // 4, what       # cells win: a comparison of fitted values


@pytest.mark.parametrize("series", SERIES)
def test_widths_and_the_plan_do_not_depend_on_the_shape(series):
    """Every shape has the default table's widths and durations: plan_edges' shapes and edge lengths hold for all of them; a
    short row changes the family (expected_plan, short_rows)."""
    default = T.case("default", series, "none", N_PERIODS)
    assert not pe.short_rows(default) and pe.expected_plan(*pe.shape(default))[0] == "slim"
    for shape in T.SHAPES:
        inp = T.case(shape, series, "none", N_PERIODS)
        numpy.testing.assert_array_equal(inp["table"].width, default["table"].width, err_msg=shape)
        numpy.testing.assert_array_equal(inp["table"].duration, default["table"].duration, err_msg=shape)
        numpy.testing.assert_array_equal(inp["periods"], default["periods"], err_msg=shape)
        assert pe.shape(inp) == pe.shape(default), shape
        assert pe.short_rows(inp) == (shape in T.SHORT_SHAPES), shape
        assert pe.expected_plan(*pe.shape(inp), short_rows=pe.short_rows(inp))[0] == ("resident" if shape in T.SHORT_SHAPES else "slim")


def test_the_synthetic_tables_are_what_the_docstring_says():
    for series in SERIES:
        flat = T.case("flat", series, "none", N_PERIODS)["table"]
        assert (flat.values == 0.5).all() and (flat.overshoot == 1.0).all()
        k = T.k_mono(T.case("cusp3", series, "none", N_PERIODS)["table"])
        assert (k < 0).sum() >= 10 and (k >= 0).sum() >= 10, k
        for shape in T.SHAPES:
            if shape != "cusp3":        # every preset and keyword combination stays on the bound's valid side
                assert (T.k_mono(T.case(shape, series, "none", N_PERIODS)["table"]) >= 0).all(), shape
    assert T.case("grazing_ld", "k2", "none", N_PERIODS)["table"].overshoot.max() > 2.3


def test_the_short_shapes_are_short_on_every_row():
    assert (T.short_by(T.case("ecc_short", "k2", "none", N_PERIODS)["table"]) == 1).all()
    assert (T.short_by(T.case("ecc_short", "gapped", "none", N_PERIODS)["table"]) == 1).all()
    k2, gapped = (T.short_by(T.case("grazing_ecc", s, "none", N_PERIODS)["table"]) for s in SERIES)
    assert k2.min() >= 1 and k2.max() == 3 and gapped.min() >= 1 and gapped.max() == 5
    for shape in T.SHAPES:
        if shape not in T.SHORT_SHAPES:
            assert (T.short_by(T.case(shape, "gapped", "none", N_PERIODS)["table"]) == 0).all(), shape


def test_reading_a_row_backwards_shows_on_the_asymmetric_shapes_only():
    """The distance between the statement and the statement with every row reversed (k2 prefix): what a kernel that pairs tap
    j with sample d - 1 - j would be off by."""
    moved = {}
    for shape in ("grazing", "box", "ecc_full", "ecc_short", "grazing_ecc", "skew"):
        spec = T.statement(shape, "k2", "none", N_PERIODS)
        back = T.statement(shape, "k2", "none", N_PERIODS, variant="reverse_rows")
        moved[shape] = search_spec.distance(back["chi2"], spec["chi2"])
        print("%-12s asymmetry %.1e   reversed rows move the statement by %.1e, %d of %d rows change"
              % (shape, T.asymmetry(T.case(shape, "k2", "none", N_PERIODS)["table"]), moved[shape],
                 int((back["row"] != spec["row"]).sum()), len(spec["row"])))
    for shape in T.PRESETS:
        assert moved[shape] < 1e-12, moved
    for shape in ("skew", "ecc_short", "grazing_ecc"):
        assert moved[shape] > 1e-5, moved
    assert moved["ecc_full"] > 1e-6, moved


@pytest.mark.parametrize("series", SERIES)
@pytest.mark.parametrize("shape", T.SHORT_SHAPES)
def test_padding_a_short_row_with_zero_taps_is_not_the_reference(shape, series):
    spec = T.statement(shape, series, "none", N_PERIODS)
    padded = T.statement(shape, series, "none", N_PERIODS, variant="pad_short_rows")
    dist = search_spec.distance(padded["chi2"], spec["chi2"])
    print("%-12s %-7s padded with q = 0: %.1e from the statement, %d of %d rows change"
          % (shape, series, dist, int((padded["row"] != spec["row"]).sum()), len(spec["row"])))
    assert dist > 1e-3, (shape, series, dist)
