"""Developer tool: what the phase scan of survey mode costs on 1024 k2_90d rows with K = 8 (the method of
tools/peak_fits_time.py: best of three runs of each call in one process, the calls taking turns).

In one run: survey.power_batch(peaks=8, statistics=True) -- the call without the peak-fit stage --, the same with
peak_fits=True and the same with peak_fits=True, phase_scan=True; the time the peak-fit stage adds and the time the scan adds
behind it (the condition: the scan adds less than the stage it sits behind); and the scan kernel's time per launch group,
from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process of its own, started before this
process opens the GPU).  The results with and without the scan are compared byte for byte on the way.

Usage: python tools/phase_scan_time.py [n_rows=1024] [--json OUT] [--no-profile]"""
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

args = sys.argv[1:]


def option(name):
    if name not in args:
        return None
    i = args.index(name)
    value = args[i + 1]
    del args[i:i + 2]
    return value


out_path = option("--json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
kernel_mode = option("--kernel")                      # "scan": the profiled child
profile = "--no-profile" not in args and not kernel_mode
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
K = 8
KERNEL = "tls_phase_scan_kernel"
sys.path.insert(0, ROOT)
from tls_amd import _lib, survey, synthetic  # noqa: E402


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns():
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel scan`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="phase_scan_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", "scan"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    name = rec.get("Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                    calls, total = out.get(name, (0, 0.0))
                    out[name] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
        return out or None
    finally:
        shutil.rmtree(work, ignore_errors=True)


t, flux, kw = rows_of("k2_90d", n_rows)
if kernel_mode:   # (the profiled child: one call, once warm and once more)
    ctx = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(2):
            survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=True, phase_scan=True, context=ctx, **kw)
    ctx.close()
    sys.exit(0)

kernels = kernel_ns() if profile else None
ctx = _lib.Context(0)
runs = {
    "power_batch_peaks8_statistics": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, context=ctx, **kw),
    "power_batch_peaks8_statistics_peak_fits": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=True,
                                                                          context=ctx, **kw),
    "power_batch_peaks8_statistics_peak_fits_phase_scan": lambda: survey.power_batch(
        t, flux, peaks=K, statistics=True, peak_fits=True, phase_scan=True, context=ctx, **kw),
}
best, last = {}, {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for run in runs.values():   # (warm: plan, device buffers, code objects)
        run()
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            last[name] = run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
fits, scans = (last["power_batch_peaks8_statistics_peak_fits" + s] for s in ("", "_phase_scan"))
same = fits[0].tobytes() == scans[0].tobytes() and all(fits[2]["peaks"][k].tobytes() == scans[2]["peaks"][k].tobytes()
                                                       for k in fits[2]["peaks"].dtype.names)
p = scans[2]["peaks"]
res = {"root": ROOT, "rows": n_rows, "n": len(t), "k": K, "best_s": best,
       "added_by_peak_fits_s": best["power_batch_peaks8_statistics_peak_fits"] - best["power_batch_peaks8_statistics"],
       "added_by_phase_scan_s": best["power_batch_peaks8_statistics_peak_fits_phase_scan"] - best["power_batch_peaks8_statistics_peak_fits"],
       "results_equal_without_the_scan": bool(same),
       "scanned": int((p["scan_status"] == 0).sum()), "n_bins_median": float(numpy.nanmedian(p["n_bins"])),
       "n_bins_max": float(numpy.nanmax(p["n_bins"]))}
res["scan_over_peak_fits"] = res["added_by_phase_scan_s"] / res["added_by_peak_fits_s"]
if kernels:
    groups = 2 * ((n_rows + 31) // 32)   # (the child runs the call twice)
    res["kernel_ns"] = {k: v for k, v in sorted(kernels.items())}
    scan = [v for k, v in kernels.items() if KERNEL in k]
    if scan:
        res["scan_kernel_launches"] = sum(v[0] for v in scan)
        res["scan_kernel_us_per_group"] = sum(v[1] for v in scan) / 1e3 / groups
        res["transit_stats_kernel_us_per_group"] = sum(v[1] for k, v in kernels.items() if "tls_transit_stats" in k) / 1e3 / groups
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
ctx.close()
