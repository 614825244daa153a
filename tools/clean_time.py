"""Developer tool: the cleaning stage on 1024 k2_90d rows and 1024 tess_27d rows that carry noise, NaN, flares and single low
samples of their own, with a sliding centre of 0.5 d and with the row's median, best of three runs of each:
(a) kernel times from a rocprofv3 --kernel-trace run of this tool's `--step kernel` (no counters in that run): the tile kernel
    a round beside tls_biweight_detrend's kernel on the same (repaired) rows and window, the per-row and the repair kernels;
(b) the whole survey.clean_batch call with its host round trip;
(c) the numpy statement (tests/clean_spec.py) on 16 host processes, on HOST_ROWS rows and scaled to the batch;
(d) survey.power_batch(detrend=Clean(...)) against survey.power_batch on rows cleaned beforehand (k2_90d).
The host step runs first, in this process, which never opens the GPU.  Every GPU step is a child process of its own under a
time limit; the tool stops at the first step that fails and starts nothing after it.
Usage: python tools/clean_time.py [n_rows=1024] [--json OUT] [--no-profile] [--no-search] [--no-host]"""
import csv
import glob
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

args = sys.argv[1:]


def _option(name):
    if name in args:
        i = args.index(name)
        value = args[i + 1]
        del args[i:i + 2]
        return value
    return None


def _flag(name):
    if name in args:
        args.remove(name)
        return True
    return False


out_path = _option("--json")
step = _option("--step")                  # a GPU child: kernel, call or search
only = _option("--config")                # ... on one configuration (the profiled child)
profile = not _flag("--no-profile")
search = not _flag("--no-search")
host = not _flag("--no-host")
n_rows = int(args[0]) if args else 1024
WINDOW, CALLS, PROCESSES, HOST_ROWS = 0.5, 3, 16, 64
CONFIGS = ("k2_90d", "tess_27d")
CLIP = dict(sigma_upper=4.0, sigma_lower=5.0, max_run=1, n_iter=3)
LIMITS = {"kernel": 600, "call": 300, "search": 900}       # seconds a GPU step may take


def rows_of(name):
    """(t, n_rows copies of the seed-0 light curve of a configuration, each with noise, 2 % NaN, twelve flares of 1 % and five
    single samples lowered by ten sigma of its own, the search keywords)."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    n = len(t)
    rng = numpy.random.default_rng(n)
    sigma = rng.uniform(2e-4, 6e-4, (n_rows, 1))
    f = numpy.tile(f0, (n_rows, 1)) * (1.0 + sigma * rng.standard_normal((n_rows, n)))
    for r in range(n_rows):
        for a in rng.integers(0, n - 6, 12):
            f[r, a:a + 6] += 0.01 * numpy.exp(-numpy.arange(6) / 2.0)
        f[r, rng.integers(0, n, 5)] -= 10.0 * sigma[r, 0]
        f[r, rng.choice(n, n // 50, replace=False)] = numpy.nan
    return t, f, kw


def statement_rows(job):
    import clean_spec
    t, y, window = job
    return clean_spec.clean(t, y, window_length=window, **CLIP)[0]


def kernel_launches(work):
    """{kernel: [duration ns of every launch, in launch order]} of the cleaning and biweight kernels in a rocprofv3
    --kernel-trace directory."""
    found = []
    for path in glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for rec in csv.DictReader(fh):
                name = rec.get("Kernel_Name", "")
                for key in ("tls_clean_tile", "tls_clean_row_kernel", "tls_clean_repair_kernel", "tls_clean_init", "tls_biweight_detrend"):
                    if key in name:
                        found.append((float(rec["Start_Timestamp"]), key, float(rec["End_Timestamp"]) - float(rec["Start_Timestamp"])))
                        break
    out = {}
    for _, key, ns in sorted(found):
        out.setdefault(key, []).append(ns)
    return out


def gpu_step(name, res, under_profiler=False, config=None):
    """Runs `--step name` as a child under its time limit and merges the JSON line it prints; False where it failed.  Under the
    profiler the child takes one configuration, so that the trace's launches are that configuration's."""
    command = [sys.executable, os.path.abspath(__file__), str(n_rows), "--step", name] + (["--config", config] if config else [])
    work = None
    if under_profiler:
        rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if not os.path.exists(rocprof):
            res["kernel"] = "not measured: no rocprofv3"
            return True
        work = tempfile.mkdtemp(prefix="clean_time_")
        command = [rocprof, "--kernel-trace", "--output-format", "csv", "-d", work, "--"] + command
    try:
        done = subprocess.run(["timeout", "-k", "10", str(LIMITS[name])] + command, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if done.returncode != 0:
            res["failed_step"] = {"step": name, "status": done.returncode, "stderr": done.stderr.decode(errors="replace")[-2000:]}
            return False
        lines = [l for l in done.stdout.decode().splitlines() if l.startswith("{")]
        if lines:
            res.update(json.loads(lines[-1]))
        if work:
            launches = kernel_launches(work)
            for key, every in launches.items():
                res["%s_%s_ms" % (key, config)] = {"best": min(every) / 1e6, "worst": max(every) / 1e6, "launches": len(every)}
            if not launches:
                res["kernel"] = "not measured: no launches in the trace"
        return True
    finally:
        if work:
            shutil.rmtree(work, ignore_errors=True)


def best_of_three(run):
    every = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = run()
        every.append(time.perf_counter() - t0)
    return min(every), every, out


def child(name):
    from tls_amd import _lib, survey
    ctx = _lib.Context(0)
    res = {}
    for config in CONFIGS:
        if only and config != only:
            continue
        t, flux, kw = rows_of(config)
        if name == "kernel":       # (the profiled child: CALLS sliding calls, then CALLS biweight calls on the repaired rows)
            for _ in range(CALLS):
                rows = survey.clean_batch(t, flux, WINDOW, context=ctx, **CLIP)
            for _ in range(CALLS):
                survey.biweight_batch(t, rows, WINDOW, context=ctx)
        elif name == "call":
            survey.clean_batch(t, flux[:2], WINDOW, context=ctx, **CLIP)          # (warm: code objects)
            for label, window in (("sliding", WINDOW), ("row_median", None)):
                best, every, out = best_of_three(lambda: survey.clean_batch(t, flux, window, return_record=True, context=ctx, **CLIP))
                res["clean_batch_%s_%s_s" % (label, config)] = best
                res["clean_batch_%s_%s_every_s" % (label, config)] = every
                res["rounds_%s_%s" % (label, config)] = float(out[1]["rounds"].max())
        elif name == "search" and config == "k2_90d":
            step_ = survey.Clean(None, CLIP["sigma_upper"], CLIP["sigma_lower"], CLIP["max_run"], CLIP["n_iter"])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                survey.power_batch(t, flux[:64], detrend=step_, context=ctx, **kw)
                cleaned = survey.clean_batch(t, flux, None, context=ctx, **CLIP)
                with_step = best_of_three(lambda: survey.power_batch(t, flux, detrend=step_, context=ctx, **kw))[1]
                on_clean = best_of_three(lambda: survey.power_batch(t, cleaned, context=ctx, **kw))[1]
            res["power_batch_every_s"] = {"detrend_clean": with_step, "on_cleaned_rows": on_clean}
            res["clean_rate_ratio"] = min(on_clean) / min(with_step)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    if step:
        child(step)
        sys.exit(0)
    res = {"rows": n_rows, "window": WINDOW, "clip": CLIP}
    if host:
        with multiprocessing.get_context("fork").Pool(PROCESSES) as pool:
            for config in CONFIGS:
                t, flux, kw = rows_of(config)
                rows = min(HOST_ROWS, n_rows)
                bounds = numpy.linspace(0, rows, PROCESSES + 1).astype(int)
                for label, window in (("sliding", WINDOW), ("row_median", None)):
                    jobs = [(t, flux[a:b], window) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
                    t0 = time.perf_counter()
                    pool.map(statement_rows, jobs)
                    res["numpy_statement_%d_processes_%s_%s_s" % (PROCESSES, label, config)] = \
                        (time.perf_counter() - t0) * n_rows / rows            # (scaled from `rows` rows to the batch)
    ok = True
    for config in CONFIGS:
        if ok and profile:
            ok = gpu_step("kernel", res, True, config)
    for name, wanted in (("call", True), ("search", search)):
        if ok and wanted:
            ok = gpu_step(name, res)
    for config in CONFIGS:
        for label in ("sliding", "row_median"):
            call = res.get("clean_batch_%s_%s_s" % (label, config))
            host_s = res.get("numpy_statement_%d_processes_%s_%s_s" % (PROCESSES, label, config))
            if call and host_s:
                res["speedup_over_numpy_statement_%s_%s" % (label, config)] = host_s / call
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0 if ok else 1)
