"""Developer tool: the event-vetting kernel at Kepler length, where the chase pass is nearly all of it -- 512 candidates on 64
curves of 65536 points at 30 min, periods 20 to 400 d, durations 0.2 to 0.6 d, the rows of survey.event_vetting_rows at its
defaults (chase reach 96 to 1919 samples).  Prints the best wall time of Context.event_vetting, the chase taps counted exactly
from the records (the sum of n_chased * L), the window steps of the held-window search and a digest of both records, so that two
builds (tls_amd/csrc/Makefile `variant`, TLS_AMD_DEBUG=1 TLS_AMD_LIB=...) can be compared for time and for bits.  The kernel's
own time comes from running this tool under `rocprofv3 --kernel-trace --stats -- python tools/event_vetting_chase.py 2`
(PERF_LOG.md, "Event vetting: the chase pass").

Usage: python tools/event_vetting_chase.py [runs=5]"""
import hashlib
import json
import os
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = dict(per=12.9, rp=0.03, a=23.1, inc=89.21, ecc=0, w=90, u=[0.4804, 0.1867], limb_dark="quadratic")


def main():
    from tls_amd import _lib, survey
    from tls_amd.template import reference_transit
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rng = numpy.random.default_rng(5)
    n, n_curves, n_fits = 65536, 64, 512
    t = 100.0 + numpy.arange(n) / 48.0
    y = 1 + rng.normal(0, 3e-4, (n_curves, n))
    dy = numpy.full((n_curves, n), 3e-4)
    period = rng.uniform(20.0, 400.0, n_fits)
    T0 = t[0] + rng.uniform(0, 1, n_fits) * period
    duration = rng.uniform(0.2, 0.6, n_fits)
    curve = rng.integers(0, n_curves, n_fits)
    for f in range(n_fits):   # a box dip of 1e-3 at every epoch of every candidate
        e = numpy.round((t - T0[f]) / period[f])
        y[curve[f]][numpy.abs(t - (T0[f] + e * period[f])) < duration[f] / 2] -= 1e-3
    widths, span_max, row, reach, chase_reach, guard, chase_span = survey.event_vetting_rows(t, period, duration)
    shapes = [1.0 - numpy.asarray(reference_transit(int(L), **SHAPE)) for L in widths]
    ctx = _lib.Context(0)

    def run():
        return ctx.event_vetting(t, y, dy, period, T0, row, reach, chase_reach, guard, chase_span, widths, shapes, span_max,
                                 curve=curve, max_epochs=80)

    out = run()   # (warm: device buffers, code objects)
    best = float("inf")
    for _ in range(runs):
        t0 = time.perf_counter()
        out = run()
        best = min(best, time.perf_counter() - t0)
    ctx.close()
    print(json.dumps(dict(
        lib=_lib.LIB_PATH, call_s=best, candidates=n_fits, n=n,
        chase_taps=float(numpy.sum(numpy.nansum(out[1]["n_chased"], axis=1) * widths[row])),
        window_steps=float(numpy.sum(numpy.nan_to_num(out[0]["n_epochs"]) * (2 * reach + 1) * widths[row])),
        widths=[int(widths.min()), int(widths.max())], chase_reach=[int(chase_reach.min()), int(chase_reach.max())],
        held_events=float(numpy.nansum(out[0]["n_held"])),
        digest=hashlib.sha1(out[0].tobytes() + out[1].tobytes()).hexdigest())))


if __name__ == "__main__":
    main()
