"""Developer tool: the streaming use of one context -- a survey that searches light curves one at a time as they arrive:
tls_update_flux, tls_execute, repeat -- over distinct fluxes of one BASELINE configuration, ms per light curve on the wall
(the host's two passes over the flux and the 35 KB upload included), results left on the device.
    python tools/gpu_stream_time.py [config] [curves] [rounds]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import synthetic, _lib  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "k2_90d"
curves = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
t, f, kw = synthetic.config(name, seed=0)
inp = synthetic.search_inputs(t, f, **kw)
fluxes = [synthetic.search_inputs(t, synthetic.config(name, seed=s)[1], **kw) for s in range(curves)]
ctx = _lib.Context(0)
ctx.prepare(inp["t"], inp["y"], inp["dy"], inp["periods"], inp["table"], inp["params"])
for _ in range(3):
    ctx.execute()
prev = None
for _ in range(40):   # untimed pre-roll as in bench.py
    ms = ctx.execute_timed(10)
    if prev is not None and abs(ms - prev) <= 0.005 * prev:
        break
    prev = ms
for one in fluxes[:4]:   # untimed: whatever the context allocates at its first streamed search
    ctx.update_flux(one["y"], one["dy"])
    ctx.execute()
out = []
for _ in range(rounds):
    ctx.synchronize()
    t0 = time.perf_counter()
    for one in fluxes:
        ctx.update_flux(one["y"], one["dy"])
        ctx.execute()
    ctx.synchronize()
    out.append(1e3 * (time.perf_counter() - t0) / curves)
print("%s: update_flux + execute over %d fluxes, ms per light curve: %s  mean %.5f" % (
    name, curves, " ".join("%.5f" % v for v in out), sum(out) / len(out)), flush=True)
ctx.close()
