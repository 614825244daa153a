"""Developer tool: survey-mode median-filter detrending, best of three runs of each in one process:
(1) survey.detrend_batch on 1024 k2_90d rows at k = 25 and on 1024 tess_27d rows at k = 361 (rows on the host, one device
round trip), (2) scipy.signal.medfilt on the same rows with 16 host threads, for context, (3) survey.power_batch(detrend=25)
against survey.power_batch on the same rows detrended beforehand, and (4) survey.injection_recovery(detrend=25) against
survey.power_batch on the rows it returns (the search alone) and against survey.injection_recovery without it (whose raw rows
keep their trend: another search, not the same work).  Kernel times come from a rocprofv3 --kernel-trace --stats run of this tool.
Usage: python tools/detrend_time.py [n_rows=1024] [--json OUT]"""
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy
from scipy.signal import medfilt

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import _lib, survey, synthetic  # noqa: E402

args = sys.argv[1:]
out_path = None
if "--json" in args:
    i = args.index("--json")
    out_path = args[i + 1]
    del args[i:i + 2]
n_rows = int(args[0]) if args else 1024
HOST_WORKERS = 16


def rows_of(name):
    """n_rows copies of the seed-0 light curve of a configuration, each with noise and a slow trend of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    f *= 1.0 + 0.01 * numpy.sin(t[None, :] / rng.uniform(2.0, 6.0, (n_rows, 1)) + rng.uniform(0, 6.3, (n_rows, 1)))
    return t, f, kw


def host_medfilt(rows, k, pool):
    return numpy.array(list(pool.map(lambda r: r / medfilt(r, k), rows)))


ctx = _lib.Context(0)
pool = ThreadPoolExecutor(HOST_WORKERS)
t_k2, k2, kw_k2 = rows_of("k2_90d")
_, tess, _ = rows_of("tess_27d")
k2_flat = host_medfilt(k2, 25, pool)
inj = survey.injection_grid(t_k2, numpy.linspace(1.0, 20.0, 8), numpy.linspace(0.01, 0.1, 4), per_cell=max(1, n_rows // 32),
                            b_max=0.8, seed=0)[:n_rows]
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    inj_rows = survey.injection_recovery(t_k2, k2[0], inj, detrend=25, return_rows=True, context=ctx, **kw_k2)[2]
runs = {
    "detrend_batch_k2_k25": lambda: survey.detrend_batch(k2, 25, context=ctx),
    "detrend_batch_tess_k361": lambda: survey.detrend_batch(tess, 361, context=ctx),
    "scipy_medfilt_k2_k25_%dthreads" % HOST_WORKERS: lambda: host_medfilt(k2, 25, pool),
    "scipy_medfilt_tess_k361_%dthreads" % HOST_WORKERS: lambda: host_medfilt(tess, 361, pool),
    "power_batch_detrend25": lambda: survey.power_batch(t_k2, k2, detrend=25, context=ctx, **kw_k2),
    "power_batch_detrended_rows": lambda: survey.power_batch(t_k2, k2_flat, context=ctx, **kw_k2),
    "injection_recovery_detrend25": lambda: survey.injection_recovery(t_k2, k2[0], inj, detrend=25, context=ctx, **kw_k2),
    "power_batch_injected_detrended_rows": lambda: survey.power_batch(t_k2, inj_rows, context=ctx, **kw_k2),
    "injection_recovery": lambda: survey.injection_recovery(t_k2, k2[0], inj, context=ctx, **kw_k2),
}
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    # (warm: plan, device buffers, code objects)
    survey.power_batch(t_k2, k2[:64], detrend=25, context=ctx, **kw_k2)
    survey.detrend_batch(tess[:4], 361, context=ctx)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
res = {"rows": n_rows, "n_k2": len(t_k2), "n_tess": tess.shape[1], "best_s": best,
       "ratio_power_batch_detrend_vs_detrended_rows": best["power_batch_detrended_rows"] / best["power_batch_detrend25"],
       "ratio_injection_recovery_detrend_vs_power_batch_same_rows":
           best["power_batch_injected_detrended_rows"] / best["injection_recovery_detrend25"],
       "ratio_injection_recovery_detrend_vs_plain": best["injection_recovery"] / best["injection_recovery_detrend25"]}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
