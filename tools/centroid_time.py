"""Developer tool: what the centroid-shift test of survey mode costs on 1024 k2_90d rows with K = 8 (the method of
tools/shape_fit_time.py: best of three runs of each call in one process, the calls taking turns).

In one run: survey.power_batch(peaks=8, statistics=True, peak_fits=True), the same with shape_fit=True and the same with
centroids=(cx, cy): the time each keyword adds behind the peak-fit stage -- the centroid test's with its two extra
host-to-device copies of the batch -- and where the centroid test's time goes: Context.centroid_test (upload, kernel, copy
back) and the assembly of the result.  survey.centroid_test alone on the same candidates, against the statement's vectorised
form (tests/centroid_spec.py) on 16 host processes that never open the GPU, on a sample of the candidates.  The kernels' time
a slab comes from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process of its own, started
before this process opens the GPU): the child runs power_batch(..., shape_fit=True, centroids=(cx, cy)), so
tls_centroid_kernel and tls_shape_fit_kernel see the same candidates in the same trace.  The results with and without the
keyword are compared byte for byte on the way.

Usage: python tools/centroid_time.py [n_rows=1024] [--json OUT] [--no-profile] [--host-sample 512]"""

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
K = 8
KERNELS = ("tls_centroid_kernel", "tls_shape_fit_kernel")
HOST_PROCESSES = 16


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own, and centroid rows: a pointing
    drift of 0.01 px and noise of 1e-3 px."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    drift = 0.01 * numpy.sin(2 * numpy.pi * t / 6.0)
    cx = 100.0 + drift[None, :] + 1e-3 * rng.standard_normal(f.shape)
    cy = 200.0 - 0.7 * drift[None, :] + 1e-3 * rng.standard_normal(f.shape)
    return t, f, cx, cy, kw


def kernel_ns(n_rows):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel times`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="centroid_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", "times"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    name = rec.get("Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                    calls, total = out.get(name, (0, 0.0))
                    out[name] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
        return out or None
    except subprocess.SubprocessError as e:           # (no trace: the other measurements are taken all the same)
        print("kernel trace failed: %r" % (e,), file=sys.stderr)
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


def host_part(job):
    """The statement's vectorised form on a share of the candidates (a process that never opens the GPU)."""
    import centroid_spec as spec
    t, y_rows, cx, cy, b, max_epochs, curve, period, T0, duration = job
    return spec.centroid_batch(t, y_rows, cx, cy, period, T0, duration, curve, b, max_epochs=max_epochs)[:, 7]


def best_of(run, reps=3):
    best, last = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = run()
        best = min(best, time.perf_counter() - t0)
    return best, last


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
    host_sample = int(option("--host-sample") or 512)
    profile = "--no-profile" not in args and not kernel_mode
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    t, flux, cx, cy, kw = rows_of("k2_90d", n_rows)
    base = dict(peaks=K, statistics=True, peak_fits=True)
    if kernel_mode:   # (the profiled child: one call, once warm and once more)
        ctx = _lib.Context(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                survey.power_batch(t, flux, context=ctx, shape_fit=True, centroids=(cx, cy), **base, **kw)
        ctx.close()
        return
    kernels = kernel_ns(n_rows) if profile else None
    ctx = _lib.Context(0)
    runs = {
        "power_batch_peaks8_statistics_peak_fits": lambda: survey.power_batch(t, flux, context=ctx, **base, **kw),
        "power_batch_peaks8_statistics_peak_fits_shape_fit": lambda: survey.power_batch(t, flux, context=ctx, shape_fit=True,
                                                                                        **base, **kw),
        "power_batch_peaks8_statistics_peak_fits_centroids": lambda: survey.power_batch(t, flux, context=ctx,
                                                                                        centroids=(cx, cy), **base, **kw),
    }
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
        fits, tested = (last["power_batch_peaks8_statistics_peak_fits" + s] for s in ("", "_centroids"))
        same = fits[0].tobytes() == tested[0].tobytes() and all(fits[2]["peaks"][k].tobytes() == tested[2]["peaks"][k].tobytes()
                                                                for k in fits[2]["peaks"].dtype.names)
        # the stage's parts, on the candidates of the call
        p = tested[2]["peaks"]
        curve, rank = numpy.nonzero(p["status"] == 0)
        period, T0, duration = p["period"][curve, rank], p["T0"][curve, rank], p["duration_days"][curve, rank]
        inp, y_rows, _ = survey._batch_inputs(t, flux, None, dict(kw))
        b = survey._centroid_shape(inp)
        max_epochs = survey.centroid_epochs(inp["t"], period)
        device_s, raw = best_of(lambda: ctx.centroid_test(inp["t"], y_rows, cx, cy, period, T0, duration, b, curve=curve,
                                                          max_epochs=max_epochs))
        alone_s, alone = best_of(lambda: survey.centroid_test(t, flux, cx, cy, period, T0, duration, curve=curve, context=ctx, **kw))
    first = "power_batch_peaks8_statistics_peak_fits"
    added = best[first + "_centroids"] - best[first]
    res = {"root": ROOT, "rows": n_rows, "n": len(t), "k": K, "best_s": best, "every_s": every, "candidates": int(len(curve)),
           "max_epochs": int(max_epochs), "members_mean": float(numpy.nanmean(raw["n_points"])),
           "epochs_mean": float(numpy.nanmean(raw["n_epochs"])), "epochs_max": float(numpy.nanmax(raw["n_epochs"])),
           "added_by_centroids_s": added, "added_by_shape_fit_s": best[first + "_shape_fit"] - best[first],
           "results_equal_without_the_keyword": bool(same), "context_centroid_test_s": device_s, "assembly_s": added - device_s,
           "survey_centroid_test_alone_s": alone_s, "measured_candidates": int((raw["status"] == 0).sum()),
           "centroid_bytes_uploaded": int(2 * cx.nbytes), "record_bytes": int(raw.nbytes)}
    if kernels:
        res["kernel_ns"] = {k: v for k, v in sorted(kernels.items())}
        for name in KERNELS:
            found = [v for k, v in kernels.items() if name in k]
            if found:   # (the child runs the call twice)
                res[name + "_launches_per_call"] = sum(v[0] for v in found) / 2
                res[name + "_us_per_call"] = sum(v[1] for v in found) / 2e3
                res[name + "_us_per_slab"] = res[name + "_us_per_call"] / res[name + "_launches_per_call"]
        if all(name + "_us_per_slab" in res for name in KERNELS):
            res["centroid_over_shape_fit_per_slab"] = res[KERNELS[0] + "_us_per_slab"] / res[KERNELS[1] + "_us_per_slab"]
    ctx.close()
    # the statement on HOST_PROCESSES fresh processes, on a sample of the candidates, scaled to all of them
    if host_sample > 0 and len(curve):
        import concurrent.futures
        import multiprocessing
        take = numpy.linspace(0, len(curve) - 1, min(host_sample, len(curve))).astype(int)
        parts = numpy.array_split(take, HOST_PROCESSES)
        jobs = [(inp["t"], y_rows, cx, cy, b, max_epochs, curve[i], period[i], T0[i], duration[i]) for i in parts if len(i)]
        with concurrent.futures.ProcessPoolExecutor(HOST_PROCESSES, mp_context=multiprocessing.get_context("spawn")) as pool:
            list(pool.map(host_part, [j[:6] + tuple(a[:1] for a in j[6:]) for j in jobs]))   # (warm: interpreters, imports)
            t0 = time.perf_counter()
            shift = numpy.concatenate(list(pool.map(host_part, jobs)))
            host_s = time.perf_counter() - t0
        res["host_statement_sample"] = int(len(take))
        res["host_statement_sample_s"] = host_s
        res["host_statement_all_s"] = host_s * len(curve) / len(take)
        res["host_statement_agrees"] = bool(numpy.array_equal(shift, raw["shift_x"][take], equal_nan=True))
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
