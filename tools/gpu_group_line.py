"""Developer tool: the line T(k) -- kernel time (HIP events, tls_kernel_timing) of ONE group launch of k identical copies of
config 2's seed-0 flux, k = 1, 2, 4, 8, 16, 32, on warm clocks.  T(k) = a k + b: a is what a light curve costs once a period is
set up, b what a launch pays per period and per launch whatever it searches (PERF_LOG.md, "a period's claim and set-up").
    python tools/gpu_group_line.py [tag] [launches per k] [out.json]   -> one line per k, the fits; with a third argument
the same figures as JSON in that file"""
import json
import os
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import synthetic, _lib  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "lib"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
ctx = _lib.Context(0)
t, f, kw = synthetic.config("k2_90d")
inp = synthetic.search_inputs(t, f, **kw)
y, dy = inp["y"], inp["dy"]
# warm clocks: a pre-roll of plain launches, as bench.py's
ctx.prepare(inp["t"], y, dy, inp["periods"], inp["table"], inp["params"])
for _ in range(60):
    ctx.execute()
ctx.synchronize()
out = {"tag": tag, "n_periods": len(inp["periods"]), "reps": reps, "k": {}}
ks = (1, 2, 4, 8, 16, 32)
for k in ks:
    yb = numpy.tile(y, (k, 1))
    dyb = numpy.tile(dy, (k, 1))
    for _ in range(4):
        ctx.search_batch(inp["t"], yb, dyb, inp["periods"], inp["table"], inp["params"])
    ctx.kernel_timing()
    ms = []
    for _ in range(reps):
        ctx.search_batch(inp["t"], yb, dyb, inp["periods"], inp["table"], inp["params"])
        m, n = ctx.kernel_timing()
        assert n == 1, n
        ms.append(m)
    ms = numpy.asarray(ms)
    out["k"][k] = {"mean": float(ms.mean()), "min": float(ms.min()), "max": float(ms.max()), "std": float(ms.std()),
                   "kernel": ctx.last_kernel()}
    print("k=%2d mean %.4f min %.4f max %.4f std %.4f ms (%s)" % (k, ms.mean(), ms.min(), ms.max(), ms.std(), ctx.last_kernel()), flush=True)
kk = numpy.asarray(ks, dtype=float)
for stat in ("mean", "min"):
    tt = numpy.asarray([out["k"][k][stat] for k in ks])
    a, b = numpy.polyfit(kk, tt, 1)
    out["fit_" + stat] = {"a": float(a), "b": float(b), "b_over_T1": float(b / tt[0])}
    print("fit on %s: a = %.4f ms/curve, b = %.4f ms, b/T(1) = %.2f %%" % (stat, a, b, 100 * b / tt[0]), flush=True)
# the same line with every k weighted alike (least squares on T(k) / k = a + b / k), all six and without k = 32
for stat in ("mean", "min"):
    for top in (32, 16):
        sel = [k for k in ks if k <= top]
        per = numpy.asarray([out["k"][k][stat] / k for k in sel])
        b, a = numpy.polyfit(1.0 / numpy.asarray(sel, dtype=float), per, 1)
        out["fit_rel_%s_k%d" % (stat, top)] = {"a": float(a), "b": float(b), "b_over_T1": float(b / out["k"][1][stat])}
        print("relative fit on %s, k <= %d: a = %.4f ms/curve, b = %.4f ms, b/T(1) = %.2f %%" % (stat, top, a, b, 100 * b / out["k"][1][stat]), flush=True)
# a plain reading launch for comparison
ctx.prepare(inp["t"], y, dy, inp["periods"], inp["table"], inp["params"])
for _ in range(10):
    ctx.execute()
ctx.synchronize()
out["plain_ms"] = ctx.execute_timed(40)
print("plain execute: %.4f ms" % out["plain_ms"], flush=True)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as fh:
        json.dump(out, fh, indent=1)
