"""Developer tool: what the folded views of survey mode cost on 1024 k2_90d rows with K = 8 (the method of
tools/shape_fit_time.py: best of three runs of each call in one process, the calls taking turns).

In one run: survey.power_batch(peaks=8, statistics=True) -- the call without the peak-fit stage --, the same with
peak_fits=True, the same with peak_fits=True, views=True at the default tables (2001 + 4 x 201 bins) and at ExoMiner's
(301 + 4 x 31); the time the peak-fit stage adds, the time the views add behind it and their share of it, and where that
time goes: Context.folded_views (upload, kernel, the copy of the view arrays back) at both table sizes, the kernel alone from
a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process of its own, started before this process
opens the GPU), and the assembly of the result.  survey.folded_views alone on the same candidates, against the numpy statement
(tests/folded_views_spec.py) on 16 host processes that never open the GPU, on a sample of the candidates scaled to all of
them.  The results with and without the keyword are compared byte for byte on the way.

--call-only times nothing but the call without the keyword, power_batch(peaks=8, peak_fits=True), three times behind a
warm-up, and prints a digest of its result; --root PATH imports the package from another checkout, so the same command runs
against the parent commit's build.

Usage: python tools/folded_views_time.py [n_rows=1024] [--json OUT] [--no-profile] [--host-sample 256] [--call-only] [--root PATH]"""

import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import warnings

import numpy

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))
K = 8
KERNEL = "tls_folded_views_kernel"
HOST_PROCESSES = 16
EXOMINER = dict(views_global_bins=301, views_local_bins=31)


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns(n_rows):
    """(calls, total ns) of the views kernel in a rocprofv3 --kernel-trace --stats run of `--kernel times`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="folded_views_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", "times"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        calls, total = 0, 0.0
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    if KERNEL in rec.get("Name", ""):
                        calls, total = calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"])
        return (calls, total) if calls else None
    except subprocess.SubprocessError as e:           # (no trace: the other measurements are taken all the same)
        print("kernel trace failed: %r" % (e,), file=sys.stderr)
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


def host_part(job):
    """The numpy statement on a share of the candidates (a process that never opens the GPU): the local medians' centres."""
    import folded_views_spec as spec
    t, y_rows, curve, period, T0, duration, phi = job
    return spec.folded_views(t, y_rows, period, T0, duration, curve=curve, secondary_phase=phi)[1]["local"][:, 100]


def best_of(run, reps=3):
    best, last = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = run()
        best = min(best, time.perf_counter() - t0)
    return best, last


def digest(result):
    h = hashlib.sha256()
    h.update(result[0].tobytes())
    h.update(result[2]["peaks"].tobytes())
    return h.hexdigest()[:16]


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
    option("--root")
    host_sample = int(option("--host-sample") or 256)
    call_only = "--call-only" in args
    profile = "--no-profile" not in args and not kernel_mode and not call_only
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    t, flux, kw = rows_of("k2_90d", n_rows)
    fits = dict(peaks=K, peak_fits=True)
    if call_only:
        ctx = _lib.Context(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            survey.power_batch(t, flux[:64], context=ctx, **fits, **kw)
            survey.power_batch(t, flux, context=ctx, **fits, **kw)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                last = survey.power_batch(t, flux, context=ctx, **fits, **kw)
                times.append(time.perf_counter() - t0)
        ctx.close()
        print(json.dumps({"root": ROOT, "rows": n_rows, "call": "power_batch(peaks=8, peak_fits=True)", "s": times,
                          "digest": digest(last)}))
        return
    with_views = dict(peaks=K, statistics=True, peak_fits=True, phase_scan=True, views=True)
    if kernel_mode:   # (the profiled child: one call, once warm and once more)
        ctx = _lib.Context(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                survey.power_batch(t, flux, context=ctx, **with_views, **kw)
        ctx.close()
        return
    kernel = kernel_ns(n_rows) if profile else None
    ctx = _lib.Context(0)
    base = dict(peaks=K, statistics=True, context=ctx)
    runs = {
        "peaks8_statistics": lambda: survey.power_batch(t, flux, **base, **kw),
        "peak_fits_phase_scan": lambda: survey.power_batch(t, flux, peak_fits=True, phase_scan=True, **base, **kw),
        "peak_fits_phase_scan_views": lambda: survey.power_batch(t, flux, context=ctx, **with_views, **kw),
        "peak_fits_phase_scan_views_301_31": lambda: survey.power_batch(t, flux, context=ctx, **with_views, **EXOMINER, **kw),
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
        plain, viewed = last["peak_fits_phase_scan"], last["peak_fits_phase_scan_views"]
        same = plain[0].tobytes() == viewed[0].tobytes() and all(plain[2]["peaks"][k].tobytes() == viewed[2]["peaks"][k].tobytes()
                                                                 for k in plain[2]["peaks"].dtype.names)
        # the stage's parts, on the candidates of the call: every peak is one, as the call passes them
        p = viewed[2]["peaks"]
        fitted = (p["status"] == 0).reshape(-1)
        period, T0, duration, phi = (numpy.where(fitted, p[k].reshape(-1), numpy.nan)
                                     for k in ("period", "T0", "duration_days", "secondary_phase"))
        curve = numpy.repeat(numpy.arange(n_rows), K)
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, None, dict(kw))
        cand = (inp["t"], y_rows, period, T0, duration)
        device_s, raw = best_of(lambda: ctx.folded_views(*cand, curve=curve, secondary_phase=phi))
        small_s, _ = best_of(lambda: ctx.folded_views(*cand, curve=curve, secondary_phase=phi, n_global=301, n_local=31))
        alone_s, alone = best_of(lambda: survey.folded_views(*cand, curve=curve, secondary_phase=phi, context=ctx))
    added = best["peak_fits_phase_scan_views"] - best["peak_fits_phase_scan"]
    added_small = best["peak_fits_phase_scan_views_301_31"] - best["peak_fits_phase_scan"]
    stage = best["peak_fits_phase_scan"] - best["peaks8_statistics"]
    view_bytes = int(sum(a.nbytes for a in raw[1:]))
    res = {"root": ROOT, "rows": n_rows, "n": len(t), "k": K, "best_s": best, "every_s": every, "candidates": int(len(curve)),
           "binned_candidates": int((raw[0]["status"] == 0).sum()), "added_by_peak_fits_and_scan_s": stage,
           "added_by_views_s": added, "added_by_views_301_31_s": added_small, "views_over_peak_fit_stage": added / stage,
           "views_301_31_over_peak_fit_stage": added_small / stage, "results_equal_without_the_keyword": bool(same),
           "context_folded_views_s": device_s, "context_folded_views_301_31_s": small_s, "assembly_s": added - device_s,
           "survey_folded_views_alone_s": alone_s, "view_bytes": view_bytes,
           "local_bin_members_mean": float(numpy.mean(raw[4][:, 0][raw[0]["status"] == 0])),
           "local_bin_members_max": int(numpy.max(raw[4]))}
    if kernel:
        calls, total = kernel              # (the child runs the call twice)
        res["kernel_launches_per_call"] = calls / 2
        res["kernel_us_per_call"] = total / 2e3
        res["kernel_us_per_slab"] = total / 1e3 / calls
        res["kernel_us_per_candidate"] = total / 2e3 / max(1, len(curve))
        res["copies_and_host_s"] = device_s - total / 2e9      # (Context.folded_views less its kernels: uploads, copies back)
    ctx.close()
    # the statement on HOST_PROCESSES fresh processes, on a sample of the candidates, scaled to all of them
    if host_sample > 0 and len(curve):
        import concurrent.futures
        import multiprocessing
        take = numpy.linspace(0, len(curve) - 1, min(host_sample, len(curve))).astype(int)
        parts = numpy.array_split(take, HOST_PROCESSES)
        jobs = [(inp["t"], y_rows, curve[i], period[i], T0[i], duration[i], phi[i]) for i in parts if len(i)]
        with concurrent.futures.ProcessPoolExecutor(HOST_PROCESSES, mp_context=multiprocessing.get_context("spawn")) as pool:
            list(pool.map(host_part, [j[:2] + tuple(a[:1] for a in j[2:]) for j in jobs]))   # (warm: interpreters, imports)
            t0 = time.perf_counter()
            centre = numpy.concatenate(list(pool.map(host_part, jobs)))
            host_s = time.perf_counter() - t0
        res["host_statement_sample"] = int(len(take))
        res["host_statement_sample_s"] = host_s
        res["host_statement_all_s"] = host_s * len(curve) / len(take)
        res["host_statement_agrees"] = bool(numpy.array_equal(centre, raw[3][take, 0, 100], equal_nan=True))
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
