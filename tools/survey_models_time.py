"""Developer tool: survey-mode throughput with the plotted arrays (power_batch(models=True)) against the statistics alone
(statistics=True, per_transit=True), and power_results (the 41-key objects), on k2_90d light curves, best of three runs of
each in one process.  Usage: python tools/survey_models_time.py [n_curves=1024] [--json OUT]"""
import json
import os
import sys
import time
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import _lib, survey, synthetic  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 1024
out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
t, f0, kw = synthetic.config("k2_90d", seed=0)
fluxes = numpy.stack([synthetic.config("k2_90d", seed=s)[1] for s in range(n)])
ctx = _lib.Context(0)
runs = {
    "statistics": lambda: survey.power_batch(t, fluxes, context=ctx, statistics=True, per_transit=True, **kw),
    "models": lambda: survey.power_batch(t, fluxes, context=ctx, models=True, **kw),
    "power_results": lambda: survey.power_results(t, fluxes, context=ctx, **kw),
}
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for name, run in runs.items():   # (warm: plan, device buffers, pinned staging)
        survey.power_batch(t, fluxes[:64], context=ctx, models=name != "statistics", statistics=True, **kw)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
res = {"curves": n, "n": len(t), "best_s": best, "curves_per_s": {k: n / v for k, v in best.items()},
       "ratio_models_vs_statistics": best["statistics"] / best["models"],
       "ratio_power_results_vs_statistics": best["statistics"] / best["power_results"]}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
