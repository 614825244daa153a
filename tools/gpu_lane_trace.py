"""Developer tool: a short loop of back-to-back plain searches of one plan, the command `rocprofv3 --kernel-trace` wraps to
see how consecutive launches lie against each other (tools/lane_trace_overlap.py reads the trace).
    python tools/gpu_lane_trace.py k2_90d [executes] [lanes]            a BASELINE configuration
    python tools/gpu_lane_trace.py 720:4096 [executes] [lanes]          points:periods, the series of tests/test_search_lanes.py
lanes: 1 (default) or 0 (every launch on lane A)."""
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import synthetic, _lib  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "k2_90d"
executes = int(sys.argv[2]) if len(sys.argv) > 2 else 100
lanes = int(sys.argv[3]) if len(sys.argv) > 3 else 1
ctx = _lib.Context(0)
if ":" in what:
    n, count = (int(v) for v in what.split(":"))
    t, flux = synthetic.light_curve((n + 0.5) / 48.0, 48, 60e-6, seed=0, per=2.345, rp=0.03, a=9)
    inp = synthetic.search_inputs(t, flux)
    periods = numpy.ascontiguousarray(numpy.linspace(inp["periods"][0], inp["periods"][-1], count))
    ctx.set_options(slim=1, prune=0, screen32=0)
else:
    t, flux, kw = synthetic.config(what, seed=0)
    inp = synthetic.search_inputs(t, flux, **kw)
    periods = inp["periods"]
if hasattr(ctx, "lanes") and hasattr(ctx._lib, "tls_debug_lanes"):   # (a library built from older sources has no lanes)
    ctx.set_options(lanes=lanes)
ctx.prepare(inp["t"], inp["y"], inp["dy"], periods, inp["table"], inp["params"])
for _ in range(30):   # fills the table of folded orders; clocks up
    ctx.execute()
ctx.synchronize()
t0 = time.perf_counter()
for _ in range(executes):
    ctx.execute()
enqueued = time.perf_counter() - t0
ctx.synchronize()
wall = time.perf_counter() - t0
print("%s: %d points, %d periods, kernel %s, %d executes: %.2f us per execute on the wall, %.2f us per enqueue on the host"
      % (what, len(inp["t"]), len(periods), ctx.last_kernel(), executes, 1e6 * wall / executes, 1e6 * enqueued / executes), flush=True)
ctx.close()
