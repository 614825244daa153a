"""Developer tool: what the noise profile of survey mode costs (the method of tools/ephemeris_match_time.py: warm calls in one
process, the calls of a comparison taking turns).

In one run:
  - survey.noise_profile on n_rows rows of a configuration (k2_90d by default: 4320 points, measured in the LDS; --config
    tess_27d: 19 440 points, in device memory, widths up to 450 samples) at the default widths: the median of the warm calls,
    host clock around the whole call (copies in, both kernels, copies out, synchronise), and next to it the numpy statement
    tests/noise_profile_spec.py on 16 host processes, the arrays compared byte for byte.  The statement runs on
    --baseline-rows rows (64 by default) and its time for n_rows is that time scaled by n_rows / baseline_rows: the output
    says so;
  - the two kernels' time per call, from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process
    of its own, started before this process opens the GPU; no counters in that run);
  - survey.power_batch(peaks=8, statistics=True) on the same rows alone, with peak_fits=True and with peak_fits=True,
    noise=True, the calls taking turns: what noise adds next to what peak_fits adds, and the spread of each.  The results are
    compared byte for byte on the way.

--call-only [--root DIR] times power_batch(peaks=8, statistics=True, peak_fits=True) alone, on the tree at DIR (this one by
default): the call a parent commit's checkout is compared with, process by process, taking turns.

Usage: python tools/noise_profile_time.py [n_rows=1024] [--config NAME] [--json OUT] [--no-profile] [--no-pipeline]
           [--no-baseline] [--baseline-rows R] [--call-only [--root DIR]]"""
import csv
import glob
import hashlib
import json
import multiprocessing
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
config = option("--config") or "k2_90d"
kernel_mode = option("--kernel")                      # the rows of the profiled child
baseline_rows = int(option("--baseline-rows") or 64)
ROOT = os.path.abspath(option("--root") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
call_only = "--call-only" in args
profile = "--no-profile" not in args and not kernel_mode and not call_only
pipeline = "--no-pipeline" not in args
baseline = "--no-baseline" not in args
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
K = 8
CALLS = 9
PROCESSES = 16
KERNELS = ("tls_noise_curve_kernel", "tls_noise_width_kernel")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tls_amd import _lib, survey, synthetic  # noqa: E402


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def statement(job):
    """The numpy statement of a few rows (a worker of the pool: it never opens the GPU)."""
    import noise_profile_spec as spec
    t, rows, widths = job
    return spec.noise_profile_batch(rows, widths, t)


def kernel_ns():
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    out = {}
    work = tempfile.mkdtemp(prefix="noise_profile_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), "--kernel", str(n_rows), "--config", config], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    name = rec.get("Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                    calls, total = out.get(name, (0, 0.0))
                    out[name] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out or None


def digest(result):
    h = hashlib.sha256()
    h.update(result[0].tobytes())
    h.update(result[2]["peaks"].tobytes())
    return h.hexdigest()[:16]


if kernel_mode:   # (the profiled child: CALLS calls)
    ctx = _lib.Context(0)
    t, flux, _ = rows_of(config, int(kernel_mode))
    for _ in range(CALLS):
        survey.noise_profile(flux, t, context=ctx)
    ctx.close()
    sys.exit(0)

if call_only:
    ctx = _lib.Context(0)
    t, flux, kw = rows_of(config, n_rows)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run = lambda: survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=True, context=ctx, **kw)  # noqa: E731
        run()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = run()
            times.append(time.perf_counter() - t0)
    print(json.dumps({"root": ROOT, "config": config, "rows": n_rows, "calls_s": times, "digest": digest(got)}))
    ctx.close()
    sys.exit(0)

t, flux, kw = rows_of(config, n_rows)
widths = survey.noise_widths(t)
res = {"root": ROOT, "config": config, "rows": n_rows, "n": len(t), "widths": widths.tolist(), "calls": CALLS,
       "in_lds": bool(len(t) <= _lib.NOISE_LDS_POINTS)}
want = None
if baseline:   # (before this process opens the GPU: the workers are forked from a process that holds no device)
    sub = min(baseline_rows, n_rows)
    step = -(-sub // PROCESSES)
    jobs = [(t, flux[lo:lo + step], widths) for lo in range(0, sub, step)]
    with multiprocessing.Pool(PROCESSES) as pool:
        pool.map(statement, [(t, flux[:1], widths)] * PROCESSES)      # (warm: the workers exist and have imported numpy)
        t0 = time.perf_counter()
        parts = pool.map(statement, jobs)
        seconds = time.perf_counter() - t0
    want = [numpy.concatenate([p[i] for p in parts]) for i in range(5)]
    res["numpy_statement"] = {"processes": PROCESSES, "rows_measured": sub, "seconds_measured": seconds,
                              "seconds_for_all_rows": seconds * n_rows / sub,
                              "is": "measured" if sub == n_rows else "the time of %d rows scaled by %d / %d, not measured" % (sub, n_rows, sub)}
kernels = kernel_ns() if profile else None
ctx = _lib.Context(0)
res["device"] = ctx.name
survey.noise_profile(flux, t, context=ctx)           # (warm: code objects, device buffers)
times = []
for _ in range(CALLS):
    t0 = time.perf_counter()
    got = survey.noise_profile(flux, t, context=ctx)
    times.append(time.perf_counter() - t0)
res["device_call_s"] = {"median": float(numpy.median(times)), "min": min(times), "max": max(times)}
res["measured_curves"] = int((got["curves"]["status"] == 0).sum())
res["median_beta"] = numpy.nanmedian(got["beta"], axis=0).tolist()
if want is not None:
    sub = len(want[0])
    res["equal_to_the_statement"] = bool(
        all(got["curves"][k][:sub].tobytes() == want[0][k].tobytes() for k in want[0].dtype.names)
        and all(numpy.ascontiguousarray(got[k][:sub]).tobytes() == w.tobytes() for k, w in zip(("count", "robust", "rms", "beta"), want[1:])))
    res["numpy_over_device"] = res["numpy_statement"]["seconds_for_all_rows"] / res["device_call_s"]["median"]
if kernels:
    for name in KERNELS:
        found = [v for k, v in kernels.items() if name in k]
        if found:   # (a call launches each kernel once a slab of curves)
            res[name + "_us_per_call"] = sum(v[1] for v in found) / 1e3 / CALLS
            res[name + "_launches_per_call"] = sum(v[0] for v in found) / CALLS

if pipeline:
    common = dict(peaks=K, statistics=True, context=ctx)
    runs = {
        "peaks8_statistics": lambda: survey.power_batch(t, flux, **common, **kw),
        "peaks8_statistics_peak_fits": lambda: survey.power_batch(t, flux, peak_fits=True, **common, **kw),
        "peaks8_statistics_peak_fits_noise": lambda: survey.power_batch(t, flux, peak_fits=True, noise=True, **common, **kw),
    }
    seen, last = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for run in runs.values():   # (warm: plan, device buffers, code objects)
            run()
        for rep in range(3):
            for name, run in runs.items():
                t0 = time.perf_counter()
                last[name] = run()
                seen.setdefault(name, []).append(time.perf_counter() - t0)
    fits, noise = last["peaks8_statistics_peak_fits"], last["peaks8_statistics_peak_fits_noise"]
    same = fits[0].tobytes() == noise[0].tobytes() and all(fits[2]["peaks"][k].tobytes() == noise[2]["peaks"][k].tobytes()
                                                           for k in fits[2]["peaks"].dtype.names)
    med = {k: float(numpy.median(v)) for k, v in seen.items()}
    p = noise[2]["peaks"]
    res["pipeline"] = {"rows": n_rows, "k": K, "calls_s": seen, "median_s": med,
                       "spread": {k: float((max(v) - min(v)) / numpy.median(v)) for k, v in seen.items()},
                       "added_by_peak_fits_s": med["peaks8_statistics_peak_fits"] - med["peaks8_statistics"],
                       "added_by_noise_s": med["peaks8_statistics_peak_fits_noise"] - med["peaks8_statistics_peak_fits"],
                       "results_equal_without_noise": bool(same), "digest_without_noise": digest(fits),
                       "peaks_with_a_noise_mes": int(numpy.isfinite(p["noise_mes"]).sum()),
                       "median_noise_width": float(numpy.median(p["noise_width"][p["noise_width"] > 0]))}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
ctx.close()
