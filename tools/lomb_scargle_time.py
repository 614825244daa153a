"""Developer tool: what the variability periodogram and the sine test cost on 1024 k2_90d rows (the method of
tools/shape_fit_time.py: best of three runs of each call in one process, the calls taking turns).

In one run: survey.lomb_scargle on the default frequency grid, with the arrays and with peaks=8 alone; the same rows through
scipy.signal.lombscargle row by row on 16 host processes that never open the GPU (a sample of the rows, scaled);
survey.power_batch(peaks=8, peak_fits=True) with and without sine_test=True, the time the sine tests add, and survey.sine_test
alone on the same candidates.  The kernels' times come from a rocprofv3 --kernel-trace --stats run of this tool's --kernel
mode (a child process of its own, started before this process opens the GPU): the product's as a fraction of 2 R n F FMAs --
R rows of `a`, plus the weight row(s) at f and 2 f -- at the 78.6 TF fp64 peak.  The results with and without the sine tests
are compared byte for byte on the way.

Usage: python tools/lomb_scargle_time.py [n_rows=1024] [--json OUT] [--no-profile] [--host-sample 32] [--no-search]"""

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
K = 8
KERNELS = ("tls_nudft_kernel", "tls_gls_prologue_kernel", "tls_gls_epilogue_kernel", "tls_sine_test_kernel", "tls_find_peaks")
HOST_PROCESSES = 16
PEAK_FP64_FLOPS = 78.6e12


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns(n_rows):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel times`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="lomb_scargle_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", "times"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    name = rec.get("Name", "").split("(")[0].replace("void ", "").replace("tlsdev::", "")
                    calls, total = out.get(name, (0, 0.0))
                    out[name] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
        return out or None
    except subprocess.SubprocessError as e:           # (no trace: the other measurements are taken all the same)
        print("kernel trace failed: %r" % (e,), file=sys.stderr)
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


def host_part(job):
    """scipy's periodogram of a share of the rows (a process that never opens the GPU)."""
    from scipy.signal import lombscargle
    t, rows, f = job
    return numpy.array([lombscargle(t, y, 2 * numpy.pi * f, normalize=True, floating_mean=True) for y in rows])


def best_of(run, reps=3):
    every, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = run()
        every.append(time.perf_counter() - t0)
    return min(every), every, last


def main():
    args = sys.argv[1:]

    def option(name):
        if name not in args:
            return None
        i = args.index(name)
        value = args[i + 1]
        del args[i:i + 2]
        return value

    out_path = option("--json")
    kernel_mode = option("--kernel")                  # "times": the profiled child
    host_sample = int(option("--host-sample") or 32)
    profile = "--no-profile" not in args and not kernel_mode
    search = "--no-search" not in args
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    t, flux, kw = rows_of("k2_90d", n_rows)
    freqs = survey.variability_frequencies(t)
    rng = numpy.random.default_rng(7)
    cand_curve = numpy.repeat(numpy.arange(n_rows), K)
    cand_period = rng.uniform(1.0, 20.0, n_rows * K)
    cand_T0 = t[0] + rng.uniform(0.0, 1.0, n_rows * K) * cand_period
    cand_duration = rng.uniform(0.05, 0.3, n_rows * K)

    def sine_alone(ctx):
        return survey.sine_test(t, flux, cand_period, curve=cand_curve, T0=cand_T0, duration=cand_duration, context=ctx)

    if kernel_mode:   # (the profiled child: each call once warm and once more)
        ctx = _lib.Context(0)
        for _ in range(2):
            survey.lomb_scargle(t, flux, freqs, peaks=K, context=ctx)
            sine_alone(ctx)
        ctx.close()
        return
    kernels = kernel_ns(n_rows) if profile else None
    ctx = _lib.Context(0)
    res = {"root": ROOT, "rows": n_rows, "n": len(t), "frequencies": len(freqs), "k": K, "candidates": n_rows * K}
    survey.lomb_scargle(t, flux[:2], freqs, context=ctx)                       # (warm: code objects)
    res["lomb_scargle_s"], res["lomb_scargle_every_s"], full = best_of(lambda: survey.lomb_scargle(t, flux, freqs, context=ctx))
    res["lomb_scargle_peaks_only_s"], _, lean = best_of(
        lambda: survey.lomb_scargle(t, flux, freqs, peaks=K, with_arrays=False, context=ctx))
    res["sine_test_alone_s"], res["sine_test_alone_every_s"], sines = best_of(lambda: sine_alone(ctx))
    res["sine_test_done"] = int((sines["sine_status"] == 0).sum())
    fma = 2.0 * (n_rows + 2) * len(t) * len(freqs)                             # (cos and sin: two FMAs a (row, point, frequency))
    res["product_fma"] = fma
    if kernels:
        res["kernel_ns"] = {k: v for k, v in sorted(kernels.items())}
        for name in KERNELS:
            found = [v for k, v in kernels.items() if name in k]
            if found:   # (the child runs every call twice)
                res[name + "_us_per_call"] = sum(v[1] for v in found) / 2e3
        big = [v for k, v in kernels.items() if "tls_nudft_kernel<4>" in k]
        if big:
            us = sum(v[1] for v in big) / 2e3
            res["product_kernel_us"] = us
            res["product_fraction_of_fp64_peak"] = 2.0 * (2.0 * n_rows * len(t) * len(freqs)) / (us * 1e-6) / PEAK_FP64_FLOPS
    if search:
        runs = {"power_batch_peaks8_peak_fits": lambda: survey.power_batch(t, flux, peaks=K, peak_fits=True, context=ctx, **kw),
                "power_batch_peaks8_peak_fits_sine_test": lambda: survey.power_batch(t, flux, peaks=K, peak_fits=True,
                                                                                    sine_test=True, context=ctx, **kw)}
        best, last, every = {}, {}, {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for run in runs.values():   # (warm: plan, device buffers, code objects)
                run()
            for rep in range(3):
                for name, run in runs.items():
                    t0 = time.perf_counter()
                    last[name] = run()
                    every.setdefault(name, []).append(time.perf_counter() - t0)
                    best[name] = min(every[name])
        fits, tested = (last["power_batch_peaks8_peak_fits" + s] for s in ("", "_sine_test"))
        res["best_s"], res["every_s"] = best, every
        res["results_equal_without_the_stage"] = bool(
            fits[0].tobytes() == tested[0].tobytes()
            and all(fits[2]["peaks"][k].tobytes() == tested[2]["peaks"][k].tobytes() for k in fits[2]["peaks"].dtype.names))
        res["added_by_sine_test_s"] = best["power_batch_peaks8_peak_fits_sine_test"] - best["power_batch_peaks8_peak_fits"]
        res["sine_test_share"] = res["added_by_sine_test_s"] / best["power_batch_peaks8_peak_fits"]
    ctx.close()
    if host_sample > 0:
        import concurrent.futures
        import multiprocessing
        take = numpy.linspace(0, n_rows - 1, min(host_sample, n_rows)).astype(int)
        jobs = [(t, flux[i], freqs) for i in numpy.array_split(take, HOST_PROCESSES) if len(i)]
        with concurrent.futures.ProcessPoolExecutor(HOST_PROCESSES, mp_context=multiprocessing.get_context("spawn")) as pool:
            list(pool.map(host_part, [(t, flux[:1], freqs[:8])] * HOST_PROCESSES))   # (warm: interpreters, imports)
            t0 = time.perf_counter()
            theirs = numpy.concatenate(list(pool.map(host_part, jobs)))
            host_s = time.perf_counter() - t0
        res["scipy_sample"] = int(len(take))
        res["scipy_sample_s"] = host_s
        res["scipy_all_s"] = host_s * n_rows / len(take)
        res["scipy_max_difference"] = float(numpy.nanmax(numpy.abs(theirs - full["power"][take])))
        res["speedup_over_scipy"] = res["scipy_all_s"] / res["lomb_scargle_s"]
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
