"""Pins of tls_period_costs for tests/test_plan_host.py (no GPU needed: the call is host-only planning).

    python tools/period_costs_pins.py          writes tests/golden/period_costs_pins.npz from the library as built

The cases: every uniform-weight edge of plan_edges.PLAN_EDGES at the restatement's edge and one point past it, a slab plan of
the default set and the tess_27d configuration; each at the three noise levels of plan_edges and at one whose passing
fraction lies in [0.24, 0.30) (between the pruning threshold alone and the one beside an admissible fp32 screen: DESIGN.md
section 8); each of those under the switch sets below.  Trial cells do not depend on the noise or the switches and the
expected taps not on the switches: each is stored once."""
import math
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

FIXTURE = os.path.join(ROOT, "tests", "golden", "period_costs_pins.npz")
OPTION_SETS = (None, dict(slim=0), dict(exact_prefix=1), dict(prune=1), dict(screen32=1), dict(threads=512), dict(fast_slab=0))
BETWEEN_THE_THRESHOLDS = 0.27


def passing_fraction(widths, sigma, depth_min):
    """the library's passing_fraction: the mean over the distinct widths of Q(depth_min sqrt(d) / sigma)"""
    return sum(0.5 * math.erfc(depth_min * math.sqrt(w) / sigma / math.sqrt(2.0)) for w in widths) / len(widths)


def sigma_between_the_thresholds(inp):
    """the noise at which passing_fraction is 0.27 (it grows with sigma): by bisection"""
    widths = [int(w) for w in numpy.unique(numpy.asarray(inp["table"].width))]
    depth_min = inp["params"]["transit_depth_min"]
    lo, hi = 1e-7, 1e-1
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if passing_fraction(widths, mid, depth_min) < BETWEEN_THE_THRESHOLDS:
            lo = mid
        else:
            hi = mid
    assert 0.24 <= passing_fraction(widths, hi, depth_min) < 0.30
    return hi


def cases():
    """[(name, inputs with "selected")]"""
    import plan_edges as pe
    from tls_amd import synthetic
    out = []
    registers = [e for e in pe.PLAN_EDGES if e.name == "registers"][0].model_edge()
    for edge in pe.PLAN_EDGES:
        if edge.weights:
            continue
        at = edge.model_edge() if edge.inside is not None else registers
        for n in (at, at + 1):
            out.append(("%s@%d" % (edge.name, n), edge.inputs(n)))
    out.append(("default@12000", pe.inputs("default", 12000)))
    t, flux, kwargs = synthetic.config("tess_27d")
    inp = synthetic.search_inputs(t, flux, **kwargs)
    grid = inp["periods"]
    inp["selected"] = grid[numpy.unique(numpy.round(numpy.linspace(0, len(grid) - 1, 56)).astype(int))]
    out.append(("tess_27d", inp))
    return out


def compute(inp, sigmas):
    """(cells [periods], taps [sigma][periods], time [sigma][option set][periods], slots [sigma][option set])"""
    from tls_amd import _lib
    cells, taps, time, slots = None, [], [], []
    for sigma in sigmas:
        time.append([])
        slots.append([])
        for k, options in enumerate(OPTION_SETS):
            c, tp, tm, s = _lib.period_costs(inp["t"], inp["selected"], inp["table"], inp["params"], sigma,
                                             with_slots=True, options=options)
            assert cells is None or numpy.array_equal(cells, c)
            cells = c
            if k == 0:
                taps.append(tp)
            assert numpy.array_equal(taps[-1], tp)
            time[-1].append(tm)
            slots[-1].append(s)
    return cells, numpy.array(taps), numpy.array(time), numpy.array(slots, dtype=numpy.int64)


def sigmas_of(inp):
    import plan_edges as pe
    return [pe.QUIET, pe.SCREEN_NOISE, pe.PRUNE_NOISE, sigma_between_the_thresholds(inp)]


def main():
    store = {"names": [], "sigmas": []}
    for i, (name, inp) in enumerate(cases()):
        sigmas = sigmas_of(inp)
        cells, taps, time, slots = compute(inp, sigmas)
        store["names"].append(name)
        store["sigmas"].append(sigmas)
        store["cells_%d" % i], store["taps_%d" % i], store["time_%d" % i], store["slots_%d" % i] = cells, taps, time, slots
        print("%-28s %3d periods, slots %s" % (name, len(cells), slots.tolist()))
    store["names"] = numpy.array(store["names"])
    store["sigmas"] = numpy.array(store["sigmas"])
    numpy.savez_compressed(FIXTURE, **store)
    print("%s: %d bytes" % (FIXTURE, os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
