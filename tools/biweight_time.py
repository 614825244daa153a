"""Developer tool: survey-mode biweight detrending, best of three runs of each in one process: (1) survey.biweight_batch on
1024 k2_90d rows at 0.5 d and on 1024 tess_27d rows at 0.5 d and 1 d (rows on the host, one device round trip),
(2) survey.power_batch(detrend=Biweight(0.5)) against survey.power_batch on the same rows detrended beforehand, and
(3) survey.injection_recovery(detrend=Biweight(0.5)) against survey.power_batch on the rows it returns (the search alone).
Kernel times come from a rocprofv3 --kernel-trace --stats run of this tool (--only-detrend: the biweight_batch calls alone).
Usage: python tools/biweight_time.py [n_rows=1024] [--json OUT] [--only-detrend]"""
import json
import os
import sys
import time
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import _lib, survey, synthetic  # noqa: E402

args = sys.argv[1:]
out_path = None
if "--json" in args:
    i = args.index("--json")
    out_path = args[i + 1]
    del args[i:i + 2]
only_detrend = "--only-detrend" in args
args = [a for a in args if a != "--only-detrend"]
n_rows = int(args[0]) if args else 1024
BW = survey.Biweight(0.5)


def rows_of(name):
    """n_rows copies of the seed-0 light curve of a configuration, each with noise and a slow trend of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    f *= 1.0 + 0.01 * numpy.sin(t[None, :] / rng.uniform(2.0, 6.0, (n_rows, 1)) + rng.uniform(0, 6.3, (n_rows, 1)))
    return t, f, kw


ctx = _lib.Context(0)
t_k2, k2, kw_k2 = rows_of("k2_90d")
t_tess, tess, _ = rows_of("tess_27d")
runs = {
    "biweight_batch_k2_0.5d": lambda: survey.biweight_batch(t_k2, k2, 0.5, context=ctx),
    "biweight_batch_tess_0.5d": lambda: survey.biweight_batch(t_tess, tess, 0.5, context=ctx),
    "biweight_batch_tess_1d": lambda: survey.biweight_batch(t_tess, tess, 1.0, context=ctx),
}
if not only_detrend:
    k2_flat = survey.biweight_batch(t_k2, k2, 0.5, context=ctx)
    inj = survey.injection_grid(t_k2, numpy.linspace(1.0, 20.0, 8), numpy.linspace(0.01, 0.1, 4),
                                per_cell=max(1, n_rows // 32), b_max=0.8, seed=0)[:n_rows]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inj_rows = survey.injection_recovery(t_k2, k2[0], inj, detrend=BW, return_rows=True, context=ctx, **kw_k2)[2]
    runs.update({
        "power_batch_biweight": lambda: survey.power_batch(t_k2, k2, detrend=BW, context=ctx, **kw_k2),
        "power_batch_detrended_rows": lambda: survey.power_batch(t_k2, k2_flat, context=ctx, **kw_k2),
        "injection_recovery_biweight": lambda: survey.injection_recovery(t_k2, k2[0], inj, detrend=BW, context=ctx, **kw_k2),
        "power_batch_injected_detrended_rows": lambda: survey.power_batch(t_k2, inj_rows, context=ctx, **kw_k2),
    })
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    # (warm: plan, device buffers, code objects)
    survey.biweight_batch(t_tess, tess[:4], 1.0, context=ctx)
    if not only_detrend:
        survey.power_batch(t_k2, k2[:64], detrend=BW, context=ctx, **kw_k2)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
res = {"rows": n_rows, "n_k2": len(t_k2), "n_tess": len(t_tess), "best_s": best}
if not only_detrend:
    res["ratio_power_batch_biweight_vs_detrended_rows"] = best["power_batch_detrended_rows"] / best["power_batch_biweight"]
    res["ratio_injection_recovery_biweight_vs_power_batch_same_rows"] = (best["power_batch_injected_detrended_rows"]
                                                                          / best["injection_recovery_biweight"])
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
