"""The edges of the search planner, for tests/test_plan_edges.py: light curves of any requested length that are hostile
to index arithmetic, the parameter sets that make each clause of the plan the binding one, an independent restatement
of the plan (written from DESIGN.md section 4 and the header comments of the kernels, not from tls_prepare), and the
bisection that finds the last length on one side of an edge from the library's own report.

Parameter sets (chosen on the CPU with tls_period_costs and search_inputs; a process without a GPU plans for 256 CUs):

  default  48 samples a day, power()'s default grids.  The widest window is 0.12 N: a series leaves the four-slot
           kernel at the 20 samples a thread keeps (5120 points), long before its region leaves a third of the LDS.
  wide     the same series with the template table of a series three times as long: windows up to 0.36 N (the rows beyond
           0.18 N are in no period's range; they widen M).  The LDS shares bind before the register clause does, a series
           of at most 5120 points can fall between a third and a half of the LDS, and the slab's rows turn `oversize` at a
           third of the default set's length.  power() itself cannot widen the windows: T14 is capped at 0.12 of the
           period (constants.FRACTIONAL_TRANSIT_DURATION_MAX), whatever R_star_max and M_star_min are; a caller of the C
           ABI brings its own table.
  fine     the default windows on a duration grid of step 1.02 (default 1.1): the width table reaches 110 distinct
           widths, the last that fit the four-slot kernel's scratch header, at ~1460 points.

search_inputs forms no template table for fewer than ~90-145 points at any cadence and period range tried (the narrowest
template rows have no sample below 1), so no set reaches 64 points; the clause n < 64 cannot bind anyway (below).

Every set is searched at low noise (50 ppm, 10 ppm below ~2600 points: the four-slot kernel where the plan admits it), and
the classic family's fp32-screen and pruning variants by raising the noise (the host's choice by noise level, README)."""
import numpy

from tls_amd import synthetic

LDS = 160 * 1024            # bytes of LDS a CU has (MI355X_MICROARCH; DESIGN.md section 4: "ONE period per CU's 160 KB")
HOST_ONLY_CUS = 256         # what a process without a GPU plans for
SLIM_PER_THREAD = 20        # "20 points a thread" 
CUMSUM_CHUNK = 8192         # elements the non-resident prefix sum scans per LDS round trip

SETS = {
    "default": dict(cadence=48.0, kwargs={}, stretch=1),
    "wide": dict(cadence=48.0, kwargs={}, stretch=3),
    "fine": dict(cadence=48.0, kwargs=dict(duration_grid_step=1.02), stretch=1),
}
QUIET, SCREEN_NOISE, PRUNE_NOISE = 50e-6, 100e-6, 1000e-6

# every clause of sections A to C of the plan that CAN bind; test_plan_edges.py ends by asserting that each was the
# binding clause of at least one case that ran
CLAUSES = (
    # A: the four-slot kernel
    "slim_registers_256",   # n <= 256 threads * 20
    "slim_bucket_room",     # the sort's buckets beside its records: at least n / 8 and 16
    "slim_width_table",     # 110 widths fill the scratch header
    "slim_lds_quarter",     # four slots against three
    "slim_lds_third",       # three slots against none
    "slim512_lds_half",     # 512-thread shape: two regions' worth of LDS for two periods
    "slim_uniform_only",    # per-point weights take the classic kernel
    "slim_exact_prefix",    # exact prefix sums throughout take the classic kernel
    "slim_gap_need_nonzero",  # <= 5120 points, a region between a third and a half of the LDS: neither shape
    # B: the classic LDS-resident kernel
    "resident_uniform",     # two regions in 160 KB
    "resident_weighted",    # three regions in 160 KB
    "classic_two_per_cu",   # two 512-thread workgroups against one of 1024 threads
    # C: the slab kernels
    "slab_sort_buckets",    # one sort bucket per point until the counters fill the LDS
    "slab_sort2",           # two-level sort against the general bucket sort
    "slab_tiles",           # M = k * tile capacity, and one more
    "slab_oversize",        # the first row wider than half a tile
    "slab_split_odd",       # an odd number of points: the two roles run the plan exact throughout or not at all
    "slab_cumsum_chunk",    # M + 1 a multiple of 8192, and one either side
)
# Clauses of tlsdev::slim_lds_bytes that no series can reach, so that no case pins them:
#   n >= 1 << slim_idx_bits   5120 < 8192 and 10240 < 16384: the register clause binds first.
#   n > 512 * 20              the 512-thread shape needs its region within half the LDS, M + 1 + pad <= 10028 doubles,
#                             and M > n: no series beyond 10027 points gets as far as this clause.
#   n < 64                    a template is at most n wide, so at 63 points the region holds at most 63 + 64 + 1 + pad
#                             doubles, and the bucket-room clause (below) wants 1.5 n + 8 (W + 1 + pad) >= 2048 + 64:
#                             it refuses every series below ~700 points first (test_the_unreachable_clauses_are_unreachable).
KERNELS = ("slim", "slim512", "resident", "resident+prune", "resident+screen32", "slab", "slab+split")


def light_curve(n, cadence=48.0, sigma=QUIET, weights=False):
    """(t, flux, dy, true period, commensurate period) of exactly n points: time stamps on the cadence grid with one point in
    seven off it and a gap of 37.37 cadences two fifths in, four exact ties, a transit centred on phase 0 of its period
    (its window wraps the phase origin), and a trial period of a whole number of cadences."""
    rng = numpy.random.RandomState(100003 + n)
    k = numpy.arange(n, dtype=numpy.float64)
    gap = (2 * n) // 5
    k[gap:] += 37.37
    off = rng.rand(n) < 1.0 / 7.0
    k[off] += rng.uniform(-0.3, 0.3, int(off.sum()))
    t = 3.0 + k / cadence
    for i in (n // 9, n // 2 + 1, n - 3):
        t[i + 1] = t[i]
    t[n // 3 + 2] = t[n // 3]                      # (a tie across a point in between)
    span = t.max() - t.min()
    true_period = min(2.0 + 1.0 / 7.0, span / 3.3)
    phase = t / true_period - numpy.floor(t / true_period)
    half = 0.01                                    # (2 % of the points, 3 sigma deep: the scatter of the flux stays the noise's)
    flux = 1.0 + rng.normal(0, sigma, n)
    flux[(phase < half) | (phase > 1.0 - half)] -= 3 * sigma
    dy = rng.uniform(0.7, 1.4, n) * sigma if weights else None
    commensurate = max(8, min(48, n // 6)) / cadence
    return t, flux, dy, true_period, commensurate


def inputs(set_name, n, sigma=QUIET, weights=False):
    """search_inputs of the set's light curve of n points, with at most ~60 periods chosen ("selected"): the shortest and
    the longest of the grid, a spread of the rest, the transit's own period and the commensurate one."""
    spec = SETS[set_name]
    t, flux, dy, true_period, commensurate = light_curve(n, spec["cadence"], sigma, weights)
    inp = synthetic.search_inputs(t, flux, dy, **spec["kwargs"])
    if spec["stretch"] > 1:
        long_t, long_flux = light_curve(spec["stretch"] * n, spec["cadence"], sigma)[:2]
        inp["table"] = synthetic.search_inputs(long_t, long_flux, None, **spec["kwargs"])["table"]
    grid = inp["periods"]
    pick = numpy.unique(numpy.round(numpy.linspace(0, len(grid) - 1, 56)).astype(int))
    extra = [p for p in (true_period, commensurate) if grid[0] <= p <= grid[-1]]
    inp["selected"] = numpy.unique(numpy.concatenate([grid[pick], extra]))
    assert inp["selected"][0] == grid[0] and inp["selected"][-1] == grid[-1]
    return inp


def shape(inp):
    """(n, M, distinct widths, region pad) of a plan, from the template table alone.  The plan counts DISTINCT widths
    (tls_prepare drops later duplicates of a width): len(numpy.unique(table.width)).  M = n + the widest width made even
    (core.py:114-116).  The pad behind a region is what the sliding dot product reads past a window: two groups of 8 taps
    and 5 positions at the widest stride of a row whose windows share samples (at least 5), rounded up to 8 doubles; the
    GPU tests take it from plan_info() of a neighbouring plan instead and compare (test_plan_edges.py)."""
    width = numpy.unique(numpy.asarray(inp["table"].width))
    n = len(inp["t"])
    W = int(width[-1]) + int(width[-1]) % 2
    margin = inp["params"]["T0_fit_margin"]
    stride = 1
    for w in width:
        xth = max(1, int(w * margin)) if margin > 0 and w > margin else 1
        if xth <= 5 or (xth <= 128 and 8 * xth <= w):
            stride = max(stride, xth)
    pad = (16 + 5 * max(stride, 5) + 7) // 8 * 8
    return n, n + W, len(width), pad


def classic_header(n_widths):
    """wave scratch (560) | prefix-sum scratch (1920) | three words a width and two more, to a 16-byte boundary"""
    return (560 + 1920 + 4 * (3 * n_widths + 2) + 15) // 16 * 16


def slim_header(threads):
    """wave sums (128) | 24 bytes a wavefront | work counters (48) | scratch (1328): 1.6 KB for 256 threads"""
    return 128 + threads // 64 * 24 + 48 + 1328


def short_rows(inp):
    """A template row shorter than its width (an eccentric orbit's table): the plan keeps such a table out of the four-slot
    kernel and out of the classic kernel's fp32-screen and pruning variants, forced or not (include/tls_amd.h)."""
    return bool((numpy.asarray(inp["table"].length) < numpy.asarray(inp["table"].width)).any())


def expected_plan(n, M, n_widths, pad, uniform=True, exact_prefix=False, noise_variant=None, short_rows=False):
    """(kernel, periods a CU holds side by side) of a search of at most ~60 periods, restated from the documents: README
    ("Kernel variants"), DESIGN.md section 4, the header comments of tls_slim_kernel.hip.h and include/tls_amd.h.
    noise_variant: "resident+screen32" / "resident+prune" where the host takes one of those by the noise level.
    (Slab: a launch of ~60 periods is a partly filled round of workgroups, so it takes the two roles where they can run the
    plan's prefix-sum mode -- uniform weights and an even number of points; rows wider than a tile are not known here.)"""
    region = M + 1 + pad                                   # doubles
    regions = 2 if uniform else 3
    classic = classic_header(n_widths) + regions * 8 * region
    if classic > LDS or n > 65535:
        return ("slab+split" if uniform and n % 2 == 0 and not exact_prefix else "slab"), 1
    classic_slots = 2 if 2 * classic <= LDS else 1
    if not uniform or exact_prefix or short_rows:           # (a short row: the plain classic kernel, whatever the noise level)
        return "resident", classic_slots
    if noise_variant:
        return noise_variant, classic_slots
    # the four-slot kernel: sort records (4 n) | bucket counters | 2 KB pile stage | the order (2 n) inside ONE region
    room = (8 * region - 6 * n - 2048) // 4
    if room < max(n // 8, 16) or 4 * (3 * n_widths + 2) > 1328:
        return "resident", classic_slots
    if n <= 256 * SLIM_PER_THREAD:
        need = slim_header(256) + 8 * region
        if 3 * need <= LDS:
            return "slim", min(4, LDS // need)
        return "resident", classic_slots                   # (neither shape: PERF_LOG.md, open items)
    if 2 * (slim_header(512) + 8 * region) <= LDS:          # (which no series beyond 512 * 20 points meets: see above)
        return "slim512", 2
    return "resident", classic_slots


def bisect_last(lo, hi, inside):
    """The last n in [lo, hi) with inside(n), where inside(lo) holds and inside(hi) does not."""
    assert inside(lo) and not inside(hi), (lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if inside(mid):
            lo = mid
        else:
            hi = mid
    return lo


def planned_slots(inp, options=None):
    """Periods side by side on one GPU as tls_period_costs prices the search (uniform weights: the call has no dy)."""
    from tls_amd import _lib
    return _lib.period_costs(inp["t"], inp["selected"], inp["table"], inp["params"], float(numpy.std(inp["y"])),
                             with_slots=True, options=options)[3]


class Edge(object):
    """One edge of the plan: the clause that binds, the inputs that make it bind, a coarse bracket [lo, hi] with one flip of
    `inside` (a predicate on the (kernel, slots) of a plan), and the kernels the header documents on either side."""

    def __init__(self, name, clause, set_name, lo, hi, inside, kernels, sigma=QUIET, weights=False, variant=None,
                 options=None, sort_check=False):
        self.name, self.clause, self.set_name, self.lo, self.hi, self.inside = name, clause, set_name, lo, hi, inside
        self.kernels, self.sigma, self.weights, self.variant = kernels, sigma, weights, variant
        self.options, self.sort_check = options or {}, sort_check

    def inputs(self, n):
        return inputs(self.set_name, n, self.sigma, self.weights)

    def plan(self, n, pad=None):
        nn, M, nw, model_pad = shape(self.inputs(n))
        return expected_plan(nn, M, nw, model_pad if pad is None else pad, uniform=not self.weights,
                             exact_prefix=self.options.get("exact_prefix") == 1, noise_variant=self.variant)

    def model_edge(self):
        """The last length inside, by the restatement alone (no library call)."""
        return bisect_last(self.lo, self.hi, lambda n: self.inside(self.plan(n)))

    def bracket(self):
        """Every length the GPU tests' bisection may visit: 48 either side of the restatement's edge."""
        at = self.model_edge()
        return max(self.lo, at - 48), min(self.hi, at + 48)


def _kernel(*names):
    return lambda plan: plan[0] in names


# The edges of A and B (all located by bisection; the restatement above gives the bracket and the expectation)
PLAN_EDGES = (
    Edge("registers", "slim_registers_256", "default", 4500, 5400, _kernel("slim"), ("slim", "slim512")),
    Edge("registers-weighted", "slim_uniform_only", "default", 4500, 5400, None, ("resident", "resident"), weights=True),
    Edge("registers-exact", "slim_exact_prefix", "default", 4500, 5400, None, ("resident", "resident"), options=dict(exact_prefix=1)),
    Edge("bucket-room", "slim_bucket_room", "default", 500, 900, _kernel("resident"), ("resident", "slim"), sigma=10e-6, sort_check=True),
    Edge("quarter", "slim_lds_quarter", "default", 3000, 5000, lambda plan: plan[1] == 4, ("slim", "slim")),
    Edge("third", "slim_lds_third", "wide", 4000, 5100, _kernel("slim"), ("slim", "resident")),
    Edge("gap", "slim_gap_need_nonzero", "wide", 4900, 5300, _kernel("resident"), ("resident", "slim512")),
    Edge("half", "slim512_lds_half", "default", 6000, 8938, _kernel("slim512"), ("slim512", "resident")),
    Edge("resident", "resident_uniform", "default", 8000, 9500, _kernel("slim512", "resident"), ("resident", "slab*"), sort_check=True),
    Edge("resident-weighted", "resident_weighted", "default", 5000, 7000, _kernel("resident"), ("resident", "slab"), weights=True, sort_check=True),
    Edge("two-per-cu-weighted", "classic_two_per_cu", "default", 2000, 4000, lambda plan: plan[1] == 2, ("resident", "resident"), weights=True),
    Edge("two-per-cu-screen", "classic_two_per_cu", "default", 3500, 5000, lambda plan: plan[1] == 2,
         ("resident+screen32", "resident+screen32"), sigma=SCREEN_NOISE, variant="resident+screen32"),
    Edge("two-per-cu-prune", "classic_two_per_cu", "default", 3500, 5000, lambda plan: plan[1] == 2,
         ("resident+prune", "resident+prune"), sigma=PRUNE_NOISE, variant="resident+prune"),
)
# (the two cases that are no edge in n -- per-point weights and exact prefix sums at the register edge -- run at the lengths
# of "registers")


def width_table_edge(lo=1400, hi=1520):
    """(n, n + 1) in the fine set with at most 110 distinct widths at n and more at n + 1.  The count does not grow
    monotonically with n (a width is int(duration * n)), so this one is found by a scan, not by bisection."""
    counts = [shape(inputs("fine", n, 10e-6))[2] for n in range(lo, hi)]
    for i in range(len(counts) - 1):
        if counts[i] <= 110 < counts[i + 1]:
            return lo + i, lo + i + 1
    raise AssertionError("no length in [%d, %d) where the width table passes 110" % (lo, hi))


def cumsum_chunk_lengths(lo=12000, hi=16000):
    """Lengths of the default set whose prefix sum has M + 1 = 16383, 16384 and 16385 entries (two chunks of 8192: one short,
    exactly, one over)."""
    first = bisect_last(lo, hi, lambda n: shape(inputs("default", n))[1] + 1 < 2 * CUMSUM_CHUNK - 1) + 1
    found = {}
    for n in range(first, first + 8):
        found.setdefault(shape(inputs("default", n))[1] + 1, n)
    want = [2 * CUMSUM_CHUNK - 1, 2 * CUMSUM_CHUNK, 2 * CUMSUM_CHUNK + 1]
    assert all(m in found for m in want), sorted(found)
    return [found[m] for m in want]


def sort_bucket_edge(weights=False):
    """The last length of the default set with one sort bucket a point: 4 bytes a counter behind the header in 160 KB."""
    n = LDS // 4
    for _ in range(8):
        n = (LDS - classic_header(shape(inputs("default", n, QUIET, weights))[2])) // 4
    assert LDS - 4 * n - classic_header(shape(inputs("default", n, QUIET, weights))[2]) in range(0, 4)
    return n


def _halo_estimate(n, M, n_widths, pad):
    """the widest window and what four more positions at the widest stride read behind it, roughly (doubles)"""
    return (M - n) + 4 * (pad - 16) // 5 + 24


def one_tile_estimate():
    """Roughly where the default set's padded series (M doubles) and the halo of its widest window stop fitting ONE LDS tile;
    only the centre of a bracket (tile bounds are multiples of 320 positions, and the halo depends on the strides: the GPU
    test finds the edge from plan_info)."""
    def fits(n):
        s = shape(inputs("default", n))
        return 8 * (s[1] + _halo_estimate(*s)) + classic_header(s[2]) <= LDS
    return bisect_last(12000, 20000, fits)


def oversize_estimate():
    """Roughly where the wide set's widest window leaves four tile units (1280 positions) of a tile no room."""
    def fits(n):
        s = shape(inputs("wide", n))
        return 8 * (_halo_estimate(*s) + 1280) + classic_header(s[2]) <= LDS
    return bisect_last(40000, 60000, fits)
