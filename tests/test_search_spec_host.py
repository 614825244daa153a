"""The CPU oracle against the long-double statement of the search (search_spec.py), at the input scales of survey data
(input_scales.py): time stamps at JD offsets 0, 1325 and 2457000, and dy of wide range.  No GPU.

The oracle restates the reference's ARITHMETIC -- out_of_transit_residuals' running sum and `intransit + ootr[i] - edge` --
and is what every kernel is held to (1e-9, test_gpu_parity.assert_parity).  This module measures how far that arithmetic
itself sits from the definition, so that a device-against-oracle distance can be read: the statement decides the cell set as
the reference does (in double) and values every cell in numpy.longdouble.

Asserted per case (2 series x 3 offsets x 12 dy cases, 32 periods each): rows equal wherever the statement's other-row gap
exceeds 1e-8 (at most 10 % of a case's periods left out), depth within 1e-12, the oracle's chi2 within RTOL_CONTRACT of the
statement (not tighter: the distance is the reference arithmetic's own property), and the same number of evaluated cells and
template samples (the cell set is exact).

Measured here (largest |oracle - statement| / statement of a case; 2304 periods; every row equal where the gap rule
compares it, 8 periods left out, all on the gapped series; every depth inside the asserted 1e-12):

    dy                                              k2 prefix, 1500 points        gapped, 2900 points
                                          offset    0       1325    2457000       0       1325    2457000
    none, uniform(0.7, 1.4)                         3.4e-14 3.5e-14 1.9e-14       1.1e-14 1.5e-14 1.4e-14
    15 points x R,   R = 10 .. 1e3                  3.5e-14 3.4e-14 3.4e-14       1.0e-14 9.3e-15 1.8e-14
    5 points / R,    R = 10                         1.4e-13 9.8e-14 9.9e-14       1.3e-14 1.7e-14 1.5e-14
    5 points / R,    R = 1e2, 1e3                   1.1e-12 7.0e-13 7.0e-13       6.0e-13 4.8e-13 4.9e-13
    both,            R = 10                         1.4e-13 9.9e-14 9.9e-14       1.2e-14 2.0e-14 1.6e-14
    both,            R = 1e2, 1e3                   1.1e-12 7.0e-13 7.0e-13       6.0e-13 4.9e-13 4.9e-13
    both,            R = 1e4 (k2: nothing fitted)   0       0       0             6.1e-13 4.9e-13 4.9e-13

The time offset does not show.  A few precise points carry the sums (five terms of R^2 each against n of 1) and every step of
the running sum rounds at the size of the whole: the distance grows by ~30 between R = 1 and 1e2 and then stays, three orders
below the 1e-9 the kernels are held to.  (The device's distances on the same cases: test_input_scales.py)"""
import numpy
import pytest

import input_scales as S
import search_spec
from conftest import SEARCH_GOLDENS, load_search_golden, oracle_search
from test_gpu_parity import RTOL_CONTRACT

N_PERIODS = 32
DEPTH_ATOL = 1e-12


def test_longdouble_is_wider_than_double():
    assert numpy.finfo(numpy.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("name", SEARCH_GOLDENS)
def test_statement_against_the_unmodified_reference(name):
    """search_period outputs of the reference itself (tests/golden/search_*.npz): the statement's selection rules, cell set
    and row rule against them, chi2 at the distance of the reference's arithmetic."""
    g, table, params = load_search_golden(name)
    spec = search_spec.search(g["t"], g["y"], g["dy"], g["periods"], table, params)
    S.rows_agree(g["row"], spec, name)
    numpy.testing.assert_allclose(g["depth"], spec["depth"], rtol=0, atol=DEPTH_ATOL)
    finite = numpy.isfinite(g["chi2"])
    numpy.testing.assert_array_equal(finite, numpy.isfinite(spec["chi2"]))
    assert search_spec.distance(g["chi2"], spec["chi2"]) <= 1e-11
    numpy.testing.assert_array_equal(g["chi2"] == len(g["t"]), spec["chi2"] == len(g["t"]))


@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("series", ["k2", "gapped"])
def test_oracle_against_the_statement(oracle_lib, series, offset):
    left_out = 0
    for dy_name, _, _ in S.DY_CASES:
        what = (series, offset, dy_name)
        inp = S.case(series, offset, dy_name, N_PERIODS)
        n = len(inp["t"])
        spec = S.statement(series, offset, dy_name, N_PERIODS)
        chi2, row, depth, counters = oracle_search(oracle_lib, inp, periods=inp["selected"])
        dist = search_spec.distance(chi2, spec["chi2"])
        nofit = int((spec["chi2"] == n).sum())
        print("%-8s offset %-9g %-18s oracle off the statement %.2e   smallest row gap %.1e   nothing fitted in %d of %d"
              % (series, offset, dy_name, dist, spec["row_gap"].min(), nofit, len(row)))
        left_out += S.rows_agree(row, spec, what)
        numpy.testing.assert_allclose(depth, spec["depth"], rtol=0, atol=DEPTH_ATOL, err_msg=str(what))
        assert numpy.isfinite(spec["chi2"]).all() and dist <= RTOL_CONTRACT, (what, dist)
        numpy.testing.assert_array_equal(chi2 == n, spec["chi2"] == n, err_msg=str(what))
        assert int(numpy.argmin(chi2)) == spec["argmin"] or spec["period_gap"] <= 1e-8, what
        assert int(counters[1]) == int(spec["evaluated_cells"].sum()), what
        assert int(counters[2]) == int(spec["inner_steps"].sum()), what
        if dy_name.endswith("nofit") and series == "k2":
            # the no-fit path: chi2 = n, depth 0, and the row of the FIRST in-range duration -- which is not row 0 once the
            # period's shortest duration leaves the narrowest widths out
            assert nofit == len(row) and (spec["depth"] == 0).all() and (spec["row"] != 0).any(), what
        else:
            # cells win in most periods: the comparison is one of fitted values (with uniform weights S0 is about n, and a
            # period without a signal in it may keep the straight line)
            assert nofit <= len(row) // 4, (what, nofit)
    print("%s offset %g: %d periods left out of the row comparison" % (series, offset, left_out))
