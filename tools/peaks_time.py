"""Developer tool: survey-mode periodogram peaks on 1024 k2_90d rows, best of three runs of each in one process:
(1) survey.power_batch(peaks=8) against survey.power_batch alone, (2) against the route it replaces -- survey.power_batch(
with_arrays=True), which copies chi2, row, depth and power of every curve back, followed by the selection's numpy statement
(tests/peaks_spec.py) on the host --, and (3) the tls_find_peaks kernel's own time, from a rocprofv3 --kernel-trace --stats run
of this tool's --kernel mode in a child process of its own (started before this process opens the GPU).
Usage: python tools/peaks_time.py [n_rows=1024] [--json OUT] [--no-profile]"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import warnings

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import peaks_spec  # noqa: E402
from tls_amd import _lib, survey, synthetic  # noqa: E402

args = sys.argv[1:]
out_path = None
if "--json" in args:
    i = args.index("--json")
    out_path = args[i + 1]
    del args[i:i + 2]
kernel_mode = "--kernel" in args
profile = "--no-profile" not in args and not kernel_mode
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
K = 8


def rows_of(name):
    """n_rows copies of the seed-0 light curve of a configuration, each with noise of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_stats():
    """(calls, total ns, mean ns) of tls_find_peaks in a rocprofv3 --kernel-trace --stats run of `--kernel`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="peaks_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    if "tls_find_peaks" in rec.get("Name", ""):
                        return dict(calls=int(rec["Calls"]), total_ns=float(rec["TotalDurationNs"]), mean_ns=float(rec["AverageNs"]))
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


t, flux, kw = rows_of("k2_90d")
if kernel_mode:   # (the profiled child: the peaks call alone, once warm and once more)
    ctx = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(2):
            survey.power_batch(t, flux, peaks=K, context=ctx, **kw)
    ctx.close()
    sys.exit(0)

kernel = kernel_stats() if profile else None
ctx = _lib.Context(0)


def host_route():
    summary, periods, chi2, row, depth, power = survey.power_batch(t, flux, with_arrays=True, context=ctx, **kw)
    return [peaks_spec.expected(power[c], periods, K, 0.02, peaks_spec.HARMONICS, None, chi2[c], row[c], depth[c])
            for c in range(len(power))]


runs = {
    "power_batch": lambda: survey.power_batch(t, flux, context=ctx, **kw),
    "power_batch_peaks8": lambda: survey.power_batch(t, flux, peaks=K, context=ctx, **kw),
    "power_batch_with_arrays_then_numpy": host_route,
}
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    survey.power_batch(t, flux[:64], peaks=K, with_arrays=True, context=ctx, **kw)   # (warm: plan, device buffers, code objects)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
    # the two routes select the same peaks
    dev = survey.power_batch(t, flux[:64], peaks=K, context=ctx, **kw)[-1]
    host = host_route()[:64]
    same = all(dev["n_peaks"][c] == host[c][1] and numpy.array_equal(dev["peaks"]["index"][c], host[c][0]["index"]) for c in range(64))
res = {"rows": n_rows, "n": len(t), "k": K, "best_s": best, "same_peaks_both_routes": bool(same),
       "ratio_peaks8_vs_plain": best["power_batch"] / best["power_batch_peaks8"],
       "ratio_peaks8_vs_with_arrays_route": best["power_batch_with_arrays_then_numpy"] / best["power_batch_peaks8"],
       "tls_find_peaks_kernel": kernel}
if kernel:
    # one launch per group of 32 curves: the kernel's time per launch and per light curve
    res["tls_find_peaks_us_per_launch"] = kernel["mean_ns"] / 1e3
    res["tls_find_peaks_us_per_curve"] = kernel["total_ns"] / 1e3 / (2 * n_rows)
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
