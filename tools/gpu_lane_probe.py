"""Developer probe: what would two launch lanes buy?  Two contexts in one process (each with a stream, plan and
scratch of its own) search the same flux of one BASELINE configuration alternately, so that search i+1 may start on the
compute units search i has already left; against that, the same number of searches on one context, back to back on its
one stream.  ms per search, alternating rounds.
    python tools/gpu_lane_probe.py [config] [searches] [rounds]
Under `rocprofv3 --kernel-trace` (a run of its own) the trace says whether launch i+1 begins before launch i ends:
tools/lane_trace_overlap.py reads it."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import synthetic, _lib  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "k2_90d"
searches = int(sys.argv[2]) if len(sys.argv) > 2 else 400
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
t, f, kw = synthetic.config(name, seed=0)
inp = synthetic.search_inputs(t, f, **kw)
a, b = _lib.Context(0), _lib.Context(0)
for ctx in (a, b):
    ctx.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
    ctx.execute()   # fills the table of folded orders
    ctx.execute()   # reads it
    ctx.synchronize()
# untimed pre-roll as in bench.py: until two consecutive 10-launch means agree to 0.5 %
prev = None
for _ in range(40):
    ms = a.execute_timed(10)
    if prev is not None and abs(ms - prev) <= 0.005 * prev:
        break
    prev = ms
a.synchronize()


def single():
    a.synchronize(); b.synchronize()
    t0 = time.perf_counter()
    for _ in range(searches):
        a.execute()
    a.synchronize()
    return 1e3 * (time.perf_counter() - t0) / searches


def pair():
    a.synchronize(); b.synchronize()
    t0 = time.perf_counter()
    for _ in range(searches // 2):
        a.execute()
        b.execute()
    a.synchronize(); b.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (2 * (searches // 2))


def host_enqueue():
    """Host time of one execute call alone (the queue is never waited for inside the loop)."""
    a.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        a.execute()
    dt = time.perf_counter() - t0
    a.synchronize()
    return 1e3 * dt / 50


one, two = [], []
for _ in range(rounds):
    one.append(single())
    two.append(pair())
spread = lambda v: (max(v) - min(v)) / (sum(v) / len(v))
m1, m2 = sum(one) / len(one), sum(two) / len(two)
print("%s: %d points, %d periods, %d searches per round" % (name, len(inp["t"]), len(inp["periods"]), searches))
print("one context  ms/search: " + " ".join("%.5f" % v for v in one) + "  mean %.5f spread %.3f %%" % (m1, 100 * spread(one)))
print("two contexts ms/search: " + " ".join("%.5f" % v for v in two) + "  mean %.5f spread %.3f %%" % (m2, 100 * spread(two)))
print("gain %.3f %% (%.2f x the larger spread); host enqueue loop %.4f ms per execute (50 calls, includes back-pressure)"
      % (100 * (m1 - m2) / m1, (m1 - m2) / m1 / max(spread(one), spread(two), 1e-12), host_enqueue()), flush=True)
a.close()
b.close()
