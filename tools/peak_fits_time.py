"""Developer tool: what the peak fits of survey mode cost on 1024 k2_90d rows (the method of tools/peaks_time.py: best of three
runs of each call in one process).

Default mode, on this checkout: survey.power_batch(peaks=8, statistics=True, peak_fits=True) against
survey.power_batch(peaks=8, statistics=True); the kernel time the peak-fit stage adds per launch group, from two
rocprofv3 --kernel-trace --stats runs of this tool's --kernel mode (with and without the fits, each a child process of its
own, started before this process opens the GPU); and the peak device bytes (tls_debug_device_bytes) after a K = 8 call at
k2_90d and at tess_27d.

--baseline: survey.power_batch(statistics=True) and survey.search_batch, whose difference C is what the post-search chain
of the ONE pick costs per batch.  With --root DIR the package of another checkout (the parent commit's, built) is measured:
the condition to meet is  added time of peak_fits <= 1.25 * 8 * C.

Usage: python tools/peak_fits_time.py [n_rows=1024] [--baseline] [--root DIR] [--json OUT] [--no-profile]"""
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
ROOT = os.path.abspath(option("--root") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
kernel_mode = option("--kernel")                      # "fits" | "plain": the profiled child
baseline = "--baseline" in args
profile = "--no-profile" not in args and not kernel_mode and not baseline
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
K = 8
sys.path.insert(0, ROOT)
from tls_amd import _lib, survey, synthetic  # noqa: E402


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns(mode):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel mode`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="peak_fits_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", mode], check=True, stdout=subprocess.DEVNULL,
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
            survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=kernel_mode == "fits", context=ctx, **kw)
    ctx.close()
    sys.exit(0)

kernels = {m: kernel_ns(m) for m in ("fits", "plain")} if profile else None
ctx = _lib.Context(0)
if baseline:
    runs = {
        "search_batch": lambda: survey.search_batch(t, flux, context=ctx, **kw),
        "power_batch_statistics": lambda: survey.power_batch(t, flux, statistics=True, context=ctx, **kw),
    }
else:
    runs = {
        "power_batch_peaks8_statistics": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, context=ctx, **kw),
        "power_batch_peaks8_statistics_peak_fits": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=True,
                                                                              context=ctx, **kw),
    }
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for run in runs.values():   # (warm: plan, device buffers, code objects)
        run()
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
res = {"root": ROOT, "rows": n_rows, "n": len(t), "k": K, "best_s": best}
if baseline:
    res["C_one_pick_chain_s"] = best["power_batch_statistics"] - best["search_batch"]
else:
    res["added_by_peak_fits_s"] = best["power_batch_peaks8_statistics_peak_fits"] - best["power_batch_peaks8_statistics"]
    res["device_bytes_k2_90d"] = ctx.device_bytes()[0]
    ctx.close()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = _lib.Context(0)
        survey.power_batch(t, flux[:32], peaks=K, statistics=True, context=plain, **kw)
        res["device_bytes_k2_90d_without_fits"] = plain.device_bytes()[0]
        plain.close()
        tt, ft, kwt = rows_of("tess_27d", 32)
        other = _lib.Context(0)
        survey.power_batch(tt, ft, peaks=K, statistics=True, peak_fits=True, context=other, **kwt)
        res["device_bytes_tess_27d"] = other.device_bytes()[0]
        plain = _lib.Context(0)
        survey.power_batch(tt, ft, peaks=K, statistics=True, context=plain, **kwt)
        res["device_bytes_tess_27d_without_fits"] = plain.device_bytes()[0]
    if kernels and kernels["fits"] and kernels["plain"]:
        groups = 2 * ((n_rows + 31) // 32)   # (the child runs the call twice)
        # (the stage launches these and nothing else; the search kernel's run-to-run spread would drown them in a total)
        stage = ("tls_peak_picks", "tls_power_prep", "tls_t0fit", "tls_first_min", "tls_transit_stats")
        total = {m: sum(v[1] for k, v in kernels[m].items() if any(s in k for s in stage)) for m in kernels}
        res["kernel_ns"] = {m: {k: v for k, v in sorted(kernels[m].items())} for m in kernels}
        res["stage_kernel_us_per_group"] = (total["fits"] - total["plain"]) / 1e3 / groups
        # the stage's own launches per group: one set per slab of 128 fits
        res["stage_by_kernel_us_per_group"] = {k: (v[1] - kernels["plain"].get(k, (0, 0.0))[1]) / 1e3 / groups
                                               for k, v in sorted(kernels["fits"].items())
                                               if abs(v[1] - kernels["plain"].get(k, (0, 0.0))[1]) > 1e3 * groups}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
