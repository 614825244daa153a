"""Developer tool: survey-mode false-alarm calibration throughput on the k2_90d time stamps, best of three runs of each in one
process: (1) survey.null_sde with white noise (rows formed on the device, tls_null_rows mode 0) and (2) with a block
bootstrap of one planet-free row of white plus red noise (mode 1, one day per block), each against (3, 4)
survey.power_batch on the same rows, the search alone, and (5, 6) the row generation alone (Context.null_rows).  Then the calibrated SDE at a false-alarm
probability of 1 % and 0.1 % of each null (survey.fap_table / sde_threshold) beside the reference's table (stats._fap_table).
Usage: python tools/null_calibration_time.py [n_trials=1024] [--json OUT]"""
import json
import os
import sys
import time
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import _lib, stats, survey, synthetic  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_trials = int(args[0]) if args else 1024
out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
t, _, kw = synthetic.config("k2_90d", seed=0)
n = len(t)
sigma = 50e-6
block = 48   # (one day of the 48-a-day cadence)
ctx = _lib.Context(0)

# the bootstrap's source: a planet-free row of white noise plus red noise correlated over 6 hours (a 12-point box filter),
# the time scale of a transit
rng = numpy.random.RandomState(1)
red = numpy.convolve(rng.standard_normal(n + 11), numpy.ones(12), "valid")
source = 1.0 + rng.normal(0.0, sigma, n) + sigma * red / numpy.std(red)
rows_white = ctx.null_rows(n, n_trials, 0, sigma=sigma)
rows_boot = ctx.null_rows(n, n_trials, 0, source=source, block=block)
runs = {
    "null_sde_white": lambda: survey.null_sde(t, n_trials, sigma=sigma, seed=0, context=ctx, **kw),
    "power_batch_white_rows": lambda: survey.power_batch(t, rows_white, context=ctx, **kw),
    "null_sde_bootstrap": lambda: survey.null_sde(t, n_trials, source=source, block=block, seed=0, context=ctx, **kw),
    "power_batch_bootstrap_rows": lambda: survey.power_batch(t, rows_boot, context=ctx, **kw),
    "null_rows_white_only": lambda: ctx.null_rows(n, n_trials, 0, sigma=sigma),
    "null_rows_bootstrap_only": lambda: ctx.null_rows(n, n_trials, 0, source=source, block=block),
}
best, sde = {}, {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    survey.null_sde(t, 64, sigma=sigma, context=ctx, **kw)   # (warm: plan, device buffers, pinned staging)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            out = run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
            if name.startswith("null_sde"):
                sde[name] = out["SDE"]
ref_fap, ref_thr = stats._fap_table()
ref = (ref_fap, ref_thr, 12495)
thresholds = {"reference_table": {"fap_1pct": survey.sde_threshold(ref, 0.01), "fap_0.1pct": survey.sde_threshold(ref, 0.001)}}
for name, values in sde.items():
    table = survey.fap_table(values)
    thresholds[name] = {"fap_1pct": survey.sde_threshold(table, 0.01),
                        "fap_0.1pct": survey.sde_threshold(table, 0.001) if n_trials >= 1000 else None,
                        "no_fit": int(numpy.sum(values == 0)), "median_sde": float(numpy.median(values))}
res = {"trials": n_trials, "n": n, "sigma": sigma, "block": block, "best_s": best,
       "trials_per_s": {k: n_trials / v for k, v in best.items()},
       "ratio_null_sde_vs_power_batch": {
           "white": best["power_batch_white_rows"] / best["null_sde_white"],
           "bootstrap": best["power_batch_bootstrap_rows"] / best["null_sde_bootstrap"]},
       "sde_threshold": thresholds}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
