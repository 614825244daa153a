"""Every search kernel at the edges of its plan (tests/plan_edges.py has the inputs, the parameter sets, the independent
restatement of the plan and the list of clauses).

An edge is located from the library's own report -- plan_info() of the full period grid and last_kernel() after a search --
by bisection inside a bracket the restatement gives, and then asserted against the restatement, with the region pad taken
from plan_info() of a neighbouring classic plan.  On the last length inside and the first outside: parity with the oracle by
the project's own tolerances (assert_parity), the counting and the plain instantiation bit for bit, the oracle's work
counters, a search after poisoning the LDS bit for bit, tls_period_costs' workgroups in flight against the kernel that ran,
and on the sort edges the fold and the prefix sum against numpy.

Edges that cannot be stated independently in a few lines -- the slab's tile count and its first `oversize` row (tile bounds
are multiples of 320 positions behind a halo that depends on the strides of the rows in range) -- are pinned by the kernels
the header documents on either side, lds_bytes <= 160 KB, and the same parity checks.

Clauses no series reaches (plan_edges.py lists them with the arithmetic): the two index-bit clauses, n > 512 * 20, n < 64
(and search_inputs forms no template table below ~90 points), and `sort2_bytes <= lds_budget` (the two-level sort's windows
take at most 119 KB + header at 1024 threads): the last is pinned through its switch on either side of the bucket edge.

The last test of the module asserts that the cases that ran covered every clause and every kernel name: run the module
whole."""
import numpy
import pytest

import plan_edges as pe
from conftest import oracle_search
from test_gpu_parity import assert_parity, _folded_reference
from tls_amd import synthetic

SEEN_CLAUSES, SEEN_KERNELS = set(), set()


# ---- without a GPU: the brackets, and the second copy of the planner ------------------------------------------------

def test_no_length_a_bisection_can_visit_raises():
    """search_inputs forms a template table for every length of every bracket (a length that raised would have to be
    skipped, and a bisection that skips can settle on the wrong side of an edge)."""
    for edge in pe.PLAN_EDGES:
        if edge.inside is None:
            continue
        lo, hi = edge.bracket()
        for n in range(lo, hi + 1):
            assert len(edge.inputs(n)["selected"]) <= 60
    at = pe.one_tile_estimate()
    for n in range(at - 400, at + 81):
        pe.inputs("default", n)
    at = pe.oversize_estimate()
    for n in range(at - 64 - at % 2, at + 66, 2):
        pe.inputs("wide", n)
    for n in pe.cumsum_chunk_lengths() + [pe.sort_bucket_edge(), pe.sort_bucket_edge() + 1]:
        pe.inputs("default", n, weights=True)
    for n in pe.width_table_edge():
        pe.inputs("fine", n, 10e-6)


def test_the_unreachable_clauses_are_unreachable():
    """n < 64 and n > 512 * 20 of the four-slot kernel's admission: another clause refuses every such series first."""
    for n in range(3, 64):
        for pad in (48, 56):                        # (windows of up to 64 samples share samples up to a stride of 8)
            room = (8 * (n + n + n % 2 + 1 + pad) - 6 * n - 2048) // 4      # the widest template is n wide
            assert room < 16
    assert 2 * (pe.slim_header(512) + 8 * (512 * pe.SLIM_PER_THREAD + 1 + 1 + 1 + 48)) > pe.LDS


@pytest.mark.parametrize("edge", [e for e in pe.PLAN_EDGES if e.inside is not None and not e.weights], ids=lambda e: e.name)
def test_period_costs_prices_the_kernel_the_restatement_names(edge):
    """tls_period_costs restates tls_prepare's choice for uniform weights and reports it as workgroups in flight: on either
    side of every edge of A and B it must be the restatement's slots on every CU (256 where no device can be asked)."""
    at = edge.model_edge()
    cus = pe.planned_slots(pe.inputs("default", 12000))          # a slab plan: one workgroup a CU
    for n in (at, at + 1):
        assert pe.planned_slots(edge.inputs(n), options=edge.options) == edge.plan(n)[1] * cus, (edge.name, n, edge.plan(n))
    assert edge.inside(edge.plan(at)) and not edge.inside(edge.plan(at + 1))


# ---- on the GPU -----------------------------------------------------------------------------------------------------

def _cus(gpu):
    if not hasattr(gpu, "edge_cus"):
        t, f, kw = synthetic.config("tess_27d")
        inp = synthetic.search_inputs(t, f, **kw)
        gpu.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
        info = gpu.plan_info()
        assert not info["resident"]
        gpu.edge_cus = info["n_blocks"]
    return gpu.edge_cus


def _report(gpu, inp):
    """(kernel, periods a CU holds) as the library reports them: the full grid's plan, a search of the selected periods."""
    gpu.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    info = gpu.plan_info()
    assert info["lds_bytes"] <= pe.LDS
    assert len(inp["periods"]) >= 4 * _cus(gpu) and info["n_blocks"] % _cus(gpu) == 0
    gpu.search(inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])
    kernel, per_cu = gpu.last_kernel(), info["n_blocks"] // _cus(gpu)
    if kernel.startswith("resident"):
        # the classic kernel launches up to four 512-thread workgroups a CU for a short series; its 128 registers a lane let
        # two of them be resident ("two 512-thread workgroups per CU, 4 waves/SIMD, 128 VGPRs")
        assert per_cu in (1, 2, 3, 4)
        per_cu = min(per_cu, 2)
    return kernel, per_cu


def _pad_of_the_classic_neighbour(gpu, inp, uniform):
    """The region pad from plan_info()["lds_bytes"] of the classic plan of the same series (switch slim = 0)."""
    before = gpu.get_options()["slim"]
    gpu.set_options(slim=0)
    gpu.prepare(inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])
    info = gpu.plan_info()
    gpu.set_options(slim=before)
    assert info["resident"]
    n, M, nw, model_pad = pe.shape(inp)
    doubles, rest = divmod(info["lds_bytes"] - pe.classic_header(nw), 8 * (2 if uniform else 3))
    assert rest == 0
    return doubles - M - 1


def _check_fold_and_prefix(gpu, inp):
    """gpu.folded() against numpy's stable argsort of the phases and gpu.prefix_sums() against numpy.cumsum, bit for bit.
    (Both entries run the classic or the slab kernel's sort: the four-slot kernel's own sort is pinned by the parity of its
    search and the oracle's work counters.)"""
    periods, n = inp["selected"], len(inp["t"])
    gpu.prepare(inp["t"], inp["y"], inp["dy"], periods, inp["table"], inp["params"])
    got = gpu.folded(len(periods), n)
    C = gpu.prefix_sums(len(periods))
    W = C.shape[1] - 1 - n
    assert W == pe.shape(inp)[1] - n
    for k, period in enumerate(periods):
        f = _folded_reference(inp["t"], inp["y"], period)
        numpy.testing.assert_array_equal(got[k], f, err_msg="fold, n %d period %r" % (n, period))
        numpy.testing.assert_array_equal(C[k], numpy.cumsum(numpy.insert(numpy.append(f, f[:W]), 0, 0)),
                                         err_msg="prefix sum, n %d period %r" % (n, period))


def _check_case(gpu, oracle_lib, inp, kernel, slots=None, uniform=True, sort_check=False):
    """One length: the kernel that ran, parity, the two instantiations, the work counters, poisoned LDS, the second planner."""
    args = (inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])
    n = len(inp["t"])
    counted = gpu.search(*args, count_work=True)
    plain = gpu.search(*args)
    ran = gpu.last_kernel()
    SEEN_KERNELS.add(ran)
    assert ran == kernel, (n, ran, kernel)
    info = gpu.plan_info()
    assert info["lds_bytes"] <= pe.LDS
    for a, b in zip(counted[:3], plain[:3]):
        numpy.testing.assert_array_equal(a, b, err_msg="counting against plain instantiation, n %d (%s)" % (n, ran))
    want = oracle_search(oracle_lib, inp, periods=inp["selected"])
    assert_parity(counted, want, n)
    assert counted[3]["grid_cells"] == int(want[3][0])
    assert counted[3]["evaluated_cells"] == int(want[3][1])
    assert counted[3]["inner_steps"] == int(want[3][2])
    gpu.poison_lds(0x7ff80000)
    after = gpu.search(*args)
    for a, b in zip(plain[:3], after[:3]):
        numpy.testing.assert_array_equal(a, b, err_msg="after poisoned LDS, n %d (%s)" % (n, ran))
    if uniform and slots is not None:
        assert pe.planned_slots(inp, options=gpu.get_options()) == slots * _cus(gpu), (n, ran, slots)
    if sort_check:
        _check_fold_and_prefix(gpu, inp)


def _slots_of(kernel, report_slots):
    """The table of the README: slim 4 or 3, slim512 2, classic 2 or 1, slab 1."""
    allowed = {"slim": (3, 4), "slim512": (2,), "slab": (1,), "slab+split": (1,)}.get(kernel, (1, 2))
    assert report_slots in allowed, (kernel, report_slots)
    return report_slots


_located = {}


def _locate(gpu, edge):
    if edge.name not in _located:
        lo, hi = edge.bracket()
        gpu.set_options(**edge.options)
        _located[edge.name] = pe.bisect_last(lo, hi, lambda n: edge.inside(_report(gpu, edge.inputs(n))))
    return _located[edge.name]


@pytest.mark.gpu
@pytest.mark.parametrize("edge", pe.PLAN_EDGES, ids=lambda e: e.name)
def test_edges_of_the_resident_families(gpu, oracle_lib, edge):
    """Sections A and B: the last length inside and the first outside of every clause of the four-slot kernel's admission and
    of the classic LDS-resident kernel's, uniform and per-point weights."""
    by_name = dict((e.name, e) for e in pe.PLAN_EDGES)
    n_in = _locate(gpu, edge if edge.inside is not None else by_name["registers"])
    gpu.set_options(**edge.options)
    uniform = not edge.weights
    inside, outside = edge.inputs(n_in), edge.inputs(n_in + 1)
    # the pad of the restatement is the one the library's own plan holds ...
    pad = _pad_of_the_classic_neighbour(gpu, inside, uniform)
    assert pad == pe.shape(inside)[3]
    # ... and with it the restatement puts the edge where the library has it, and names the kernel and the slots
    reports = [_report(gpu, inp) for inp in (inside, outside)]
    plans = [edge.plan(n_in, pad), edge.plan(n_in + 1, pad)]
    assert reports == plans, (edge.name, n_in, reports, plans)
    if edge.inside is not None:
        assert edge.inside(plans[0]) and not edge.inside(plans[1])
        assert n_in == edge.model_edge()
    if edge.clause in ("slim_registers_256", "slim_gap_need_nonzero", "slim_uniform_only", "slim_exact_prefix"):
        assert n_in == 256 * 20
    for inp, report, name in zip((inside, outside), reports, edge.kernels):
        expected = report[0] if name == "slab*" else name
        assert name != "slab*" or report[0] == ("slab+split" if len(inp["t"]) % 2 == 0 else "slab")
        _check_case(gpu, oracle_lib, inp, expected, _slots_of(report[0], report[1]), uniform, edge.sort_check)
    SEEN_CLAUSES.add(edge.clause)
    print("\nedge %s (%s set): last inside n = %d, %s / %s" % (edge.name, edge.set_name, n_in, reports[0], reports[1]))


@pytest.mark.gpu
def test_width_table_edge(gpu, oracle_lib):
    """110 distinct widths fill the four-slot kernel's scratch header (three words a width and two more in 1328 bytes); the
    111th sends the series to the classic kernel.  The plan counts distinct widths: len(numpy.unique(table.width))."""
    n_in, n_out = pe.width_table_edge()
    inside, outside = pe.inputs("fine", n_in, 10e-6), pe.inputs("fine", n_out, 10e-6)
    assert pe.shape(inside)[2] <= 110 < pe.shape(outside)[2]
    assert 4 * (3 * 110 + 2) <= 1328 < 4 * (3 * 111 + 2)
    reports = [_report(gpu, inside), _report(gpu, outside)]
    assert reports == [("slim", 4), ("resident", 2)], reports
    _check_case(gpu, oracle_lib, inside, "slim", 4)
    _check_case(gpu, oracle_lib, outside, "resident", 2)
    SEEN_CLAUSES.add("slim_width_table")
    print("\nwidth table edge (fine set): n = %d (%d widths) / %d (%d widths)" % (n_in, pe.shape(inside)[2], n_out, pe.shape(outside)[2]))


def _slab_kernel(n, uniform, oversize=False):
    return "slab+split" if uniform and n % 2 == 0 and not oversize else "slab"


@pytest.mark.gpu
@pytest.mark.parametrize("weights", [False, True])
def test_slab_sort_bucket_edge_and_both_sorts(gpu, oracle_lib, weights):
    """One sort bucket a point until 4-byte counters behind the header fill the 160 KB, fewer after: the general bucket sort
    reads `nb` of them.  The two-level sort fits the LDS at every length (module docstring), so the general sort is forced
    by its switch: fold and prefix sum bit for bit with either sort on either side of the edge."""
    n_in = pe.sort_bucket_edge(weights)
    for n in (n_in, n_in + 1):
        inp = pe.inputs("default", n, weights=weights)
        assert (pe.classic_header(pe.shape(inp)[2]) + 4 * n <= pe.LDS) == (n == n_in)
        for sort2 in (None, 0):
            gpu.set_options(sort2=sort2)
            _check_case(gpu, oracle_lib, inp, _slab_kernel(n, not weights), 1, not weights, sort_check=True)
    SEEN_CLAUSES.update(["slab_sort_buckets", "slab_sort2"])
    print("\nsort bucket edge (default set, weights %s): n = %d" % (weights, n_in))


@pytest.mark.gpu
def test_slab_one_tile_against_two(gpu, oracle_lib):
    """The last series one LDS tile stages whole ((lds_bytes - header) / 8 >= M doubles) and the first that takes two; per-point
    weights at the same lengths (two staged buffers: already more tiles)."""
    at = pe.one_tile_estimate()

    def one_tile(n):
        inp = pe.inputs("default", n)
        gpu.prepare(inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])
        info = gpu.plan_info()
        assert not info["resident"] and info["lds_bytes"] <= pe.LDS
        nn, M, nw, pad = pe.shape(inp)
        assert M > 2 * pe.CUMSUM_CHUNK + 4                       # (below that the prefix sum's scratch hides the tile)
        return (info["lds_bytes"] - pe.classic_header(nw)) // 8 >= M
    n_in = pe.bisect_last(at - 400, at + 80, one_tile)
    for n in (n_in, n_in + 1):
        for weights in (False, True):
            inp = pe.inputs("default", n, weights=weights)
            _check_case(gpu, oracle_lib, inp, _slab_kernel(n, not weights), 1, not weights)
    SEEN_CLAUSES.add("slab_tiles")
    print("\none tile against two (default set): last inside n = %d" % n_in)


@pytest.mark.gpu
def test_slab_first_oversize_row(gpu, oracle_lib):
    """The first length at which a row is wider than half a tile (`oversize`: evaluated from the slab, one window a
    wavefront).  The library's report of it: a short launch of an even, uniformly weighted series takes the two roles
    only while no row is oversize (include/tls_amd.h, tls_last_kernel)."""
    at = pe.oversize_estimate() // 2

    def no_oversize(half):
        inp = pe.inputs("wide", 2 * half)
        gpu.search(inp["t"], inp["y"], inp["dy"], inp["selected"], inp["table"], inp["params"])
        assert gpu.last_kernel() in ("slab", "slab+split") and gpu.plan_info()["lds_bytes"] <= pe.LDS
        return gpu.last_kernel() == "slab+split"
    n_in = 2 * pe.bisect_last(at - 32, at + 32, no_oversize)
    _check_case(gpu, oracle_lib, pe.inputs("wide", n_in), "slab+split", 1)
    _check_case(gpu, oracle_lib, pe.inputs("wide", n_in + 1), "slab", 1)
    _check_case(gpu, oracle_lib, pe.inputs("wide", n_in + 2), "slab", 1)
    # (per-point weights stage two buffers a tile, so their rows are oversize on either side: the same lengths all the same)
    for n in (n_in, n_in + 2):
        _check_case(gpu, oracle_lib, pe.inputs("wide", n, weights=True), "slab", uniform=False)
    SEEN_CLAUSES.add("slab_oversize")
    print("\nfirst oversize row (wide set): last length without one n = %d" % n_in)


@pytest.mark.gpu
def test_slab_odd_length_and_prefix_sum_chunks(gpu, oracle_lib):
    """An odd number of points keeps a short launch with the one-workgroup kernel (the two roles' fast mode wants an even
    one); and the non-resident prefix sum at M + 1 = 16383, 16384 and 16385 entries -- two chunks of 8192 one short, exactly,
    one over -- against numpy.cumsum, uniform and per-point weights."""
    lengths = pe.cumsum_chunk_lengths()
    entries = []
    for n in lengths:
        for weights in (False, True):
            inp = pe.inputs("default", n, weights=weights)
            _check_case(gpu, oracle_lib, inp, _slab_kernel(n, not weights), 1, not weights, sort_check=True)
        entries.append(pe.shape(inp)[1] + 1)
    assert entries == [2 * pe.CUMSUM_CHUNK - 1, 2 * pe.CUMSUM_CHUNK, 2 * pe.CUMSUM_CHUNK + 1]
    assert SEEN_KERNELS >= set(["slab", "slab+split"]) and len(set(n % 2 for n in lengths)) == 2
    SEEN_CLAUSES.update(["slab_cumsum_chunk", "slab_split_odd"])
    print("\nprefix-sum chunk lengths (default set): n = %s" % lengths)


def _two_role_rule(k, blocks, can_split):
    """include/tls_amd.h and DESIGN.md section 4: up to four rounds of workgroups, the last filled to between 1 and 70 %"""
    last = k % blocks
    return "slab+split" if can_split and k <= 4 * blocks and last > 0 and 10 * last <= 7 * blocks else "slab"


@pytest.mark.gpu
@pytest.mark.parametrize("name,weights,family,blocks", [("k2_90d", False, "slim", None), ("k2_90d", True, "resident", None),
                                                        ("tess_27d", False, "slab", None), ("tess_27d", True, "slab", None),
                                                        ("tess_27d", False, "slab", 250)])
def test_a_periods_result_does_not_depend_on_the_launch_shape(gpu, name, weights, family, blocks):
    """Section D: 1, B - 1, B, B + 1, 4 B and 4 B + 1 periods for B workgroups in flight (and, in the slab, a last round of
    floor(0.7 B) periods and one more, behind one and behind three whole rounds): every period's (chi2, row, depth) has the
    bits the longest launch gives it, and the kernel is the one the rule names.  70 % of a CU count of 256 is no whole
    number, so `<=` and `<` of the rule cannot be told apart there: the switch `blocks` = 250 gives a launch whose last
    round of 175 periods is filled to exactly 70 %."""
    t, f, kw = synthetic.config(name)
    dy = numpy.random.RandomState(5).uniform(0.7, 1.5, len(f)) * synthetic.CONFIGS[name][2] if weights else None
    inp = synthetic.search_inputs(t, f, dy, **kw)
    args = (inp["t"], inp["y"], inp["dy"])
    gpu.prepare(*args, inp["periods"], inp["table"], inp["params"])
    B = gpu.plan_info()["n_blocks"]
    assert B % _cus(gpu) == 0 and B // _cus(gpu) == {"slim": 4, "resident": 1, "slab": 1}[family]
    if blocks is not None:
        assert blocks <= B and (7 * blocks) % 10 == 0
        gpu.set_options(blocks=blocks)
        B = blocks
    sub = numpy.ascontiguousarray(inp["periods"][::2][::-1])          # a fixed subsample, longest period first
    assert len(sub) >= 4 * B + 1
    counts = [1, B - 1, B, B + 1, 4 * B, 4 * B + 1]
    if family == "slab":
        counts += [B + (7 * B) // 10, B + (7 * B) // 10 + 1, 3 * B + (7 * B) // 10, 3 * B + (7 * B) // 10 + 1]
    longest = gpu.search(*args, sub[:4 * B + 1], inp["table"], inp["params"])
    ran = set()
    for k in counts:
        got = gpu.search(*args, numpy.ascontiguousarray(sub[:k]), inp["table"], inp["params"])
        kernel = gpu.last_kernel()
        ran.add(kernel)
        assert kernel == (family if family != "slab" else _two_role_rule(k, B, can_split=not weights)), (k, B, kernel)
        for a, b in zip(got[:3], longest[:3]):
            numpy.testing.assert_array_equal(a, b[:k], err_msg="%d of %d periods (%s)" % (k, 4 * B + 1, kernel))
    if family == "slab" and not weights:
        assert ran == set(["slab", "slab+split"])
    SEEN_KERNELS.update(ran)


@pytest.mark.gpu
def test_every_clause_and_every_kernel_was_on_an_edge():
    """So that a later change to the planner cannot quietly turn these edge tests into mid-range tests."""
    assert SEEN_CLAUSES == set(pe.CLAUSES), sorted(set(pe.CLAUSES) ^ SEEN_CLAUSES)
    assert SEEN_KERNELS == set(pe.KERNELS), sorted(set(pe.KERNELS) ^ SEEN_KERNELS)
