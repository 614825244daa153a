"""Developer tool: survey-mode injection-recovery throughput on the seed-0 k2_90d light curve, best of three runs of each in one
process: (1) survey.injection_recovery (injection on the device, tls_inject_transits), (2) the same injections formed on the
host (transit_model.light_curve) plus survey.power_batch, (3) the injection call alone (Context.inject_transits), and (4) survey.power_batch on the rows of (1), the search alone.
Usage: python tools/injection_recovery_time.py [n_injections=1024] [--json OUT]"""
import json
import os
import sys
import time
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import _lib, survey, synthetic, transit_model  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_inj = int(args[0]) if args else 1024
out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
t, f0, kw = synthetic.config("k2_90d", seed=0)
per_cell = max(1, n_inj // 32)
inj = survey.injection_grid(t, numpy.linspace(1.0, 20.0, 8), numpy.linspace(0.01, 0.1, 4), per_cell=per_cell, b_max=0.8,
                            seed=0)[:n_inj]
n_inj = len(inj)
u = [0.4804, 0.1867]
ctx = _lib.Context(0)
consts = survey.injection_constants(inj)


def host_path():
    rows = numpy.empty((n_inj, len(t)))
    for k in range(n_inj):
        rows[k] = f0 * transit_model.light_curve(t, float(inj["T0"][k]), float(inj["period"][k]), float(inj["rp_rs"][k]),
                                                 float(inj["a"][k]), float(inj["inc"][k]), 0, 90, u, "quadratic")
    return survey.power_batch(t, rows, context=ctx, **kw)


rows = ctx.inject_transits(t, f0, consts, u[0], u[1])[0]
runs = {
    "injection_recovery": lambda: survey.injection_recovery(t, f0, inj, context=ctx, **kw),
    "power_batch_same_rows": lambda: survey.power_batch(t, rows, context=ctx, **kw),
    "host_rows_power_batch": host_path,
    "inject_only": lambda: ctx.inject_transits(t, f0, consts, u[0], u[1]),
}
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    survey.injection_recovery(t, f0, inj[:64], context=ctx, **kw)   # (warm: plan, device buffers, pinned staging)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
res = {"injections": n_inj, "n": len(t), "best_s": best, "injections_per_s": {k: n_inj / v for k, v in best.items()},
       "ratio_injection_recovery_vs_host_rows": best["host_rows_power_batch"] / best["injection_recovery"],
       "ratio_injection_recovery_vs_power_batch": best["power_batch_same_rows"] / best["injection_recovery"]}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
