"""Developer tool: spline detrending on 1024 k2_90d rows that carry a rotation signal of their own, with one knot spacing
(0.75 d) and with the ladder of eight (survey.spline_spacings), best of three runs of each:
(a) kernel time per call, from a rocprofv3 --kernel-trace run of this tool's `--step kernel` (no counters in that run);
(b) the whole survey.spline_batch call with its host round trip;
(c) the numpy statement (tests/spline_spec.py) on 16 host processes;
(d) a scipy.interpolate.make_lsq_spline loop with the same clip rounds on 16 host processes;
(e) survey.power_batch(detrend=Spline(...)) against survey.power_batch on the rows detrended beforehand.
The host steps run first, in this process, which never opens the GPU.  Every GPU step is a child process of its own under a
time limit; the tool stops at the first step that fails and starts nothing after it.  The share of a launch spent in the serial
band factorisation needs an instrumented kernel and is not measured here.
Usage: python tools/spline_time.py [n_rows=1024] [--json OUT] [--no-profile] [--no-search] [--no-host]"""
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
profile = not _flag("--no-profile")
search = not _flag("--no-search")
host = not _flag("--no-host")
n_rows = int(args[0]) if args else 1024
SPACING, N_ITER, CALLS, PROCESSES = 0.75, 5, 3, 16
LIMITS = {"kernel": 600, "call": 300, "search": 900}       # seconds a GPU step may take


def rows_of(name):
    """(t, n_rows copies of the seed-0 light curve of a configuration, each with noise and a rotation of 2 to 8 days of its
    own, the search keywords, the ladder of eight spacings)."""
    from tls_amd import survey, synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + rng.uniform(2e-4, 6e-4, (n_rows, 1)) * rng.standard_normal(f.shape)
    period, phase = rng.uniform(2.0, 8.0, (n_rows, 1)), rng.uniform(0.0, 6.0, (n_rows, 1))
    f *= 1.0 + 0.01 * numpy.sin(2.0 * numpy.pi * t[None, :] / period + phase)
    return t, f, kw, survey.spline_spacings(t, 0.5, 20.0, 8)


def statement_rows(job):
    import spline_spec
    t, y, spacing = job
    return spline_spec.fit(t, y, knot_spacing=spacing, n_iter=N_ITER)["flat"]


def scipy_rows(job):
    """make_lsq_spline on uniform knots in every segment, N_ITER clip rounds at 3 sigma (MAD); a list of spacings: each in
    turn, the least BIC kept."""
    from scipy.interpolate import make_lsq_spline
    import spline_spec
    t, y, spacing = job
    starts = spline_spec.segment_starts(t, 0.5)
    flat = numpy.empty_like(y)
    for i in range(len(y)):
        best = None
        for s in numpy.atleast_1d(spacing):
            trend, ssr, K, N = numpy.empty(len(t)), 0.0, 0, 0
            for a, b in zip(starts[:-1], starts[1:]):
                tt, yy = t[a:b], y[i, a:b]
                q = max(1, int(numpy.ceil((tt[-1] - tt[0]) / s)))
                knots = numpy.concatenate([[tt[0]] * 3, numpy.linspace(tt[0], tt[-1], q + 1), [tt[-1]] * 3])
                keep = numpy.ones(b - a, dtype=bool)
                for _ in range(N_ITER + 1):
                    try:
                        fit = make_lsq_spline(tt[keep], yy[keep], knots, k=3)
                    except (ValueError, numpy.linalg.LinAlgError):       # an interval without a point
                        fit = lambda x, m=yy[keep].mean(): numpy.full(len(x), m)
                    r = yy - fit(tt)
                    sigma = 1.4826 * numpy.median(numpy.abs(r[keep] - numpy.median(r[keep])))
                    out = keep & (numpy.abs(r) > 3.0 * sigma)
                    if not out.any():
                        break
                    keep &= ~out
                trend[a:b] = fit(tt)
                ssr, K, N = ssr + float(numpy.sum(r[keep] ** 2)), K + q + 3, N + int(keep.sum())
            d = numpy.diff(y[i])
            bic = K * numpy.log(N) + ssr / (1.4826 * numpy.median(numpy.abs(d - numpy.median(d))) / numpy.sqrt(2.0)) ** 2
            if best is None or bic < best[0]:
                best = (bic, trend)
        flat[i] = y[i] / best[1]
    return flat


def kernel_launches(work):
    """{kernel name: [duration ns of every launch]} of the tls_spline kernels in a rocprofv3 --kernel-trace directory."""
    out = {}
    for path in glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for rec in csv.DictReader(fh):
                name = rec.get("Kernel_Name", "")
                if "tls_spline" in name:
                    out.setdefault("pick" if "pick" in name else "fit", []).append(float(rec["End_Timestamp"]) - float(rec["Start_Timestamp"]))
    return out


def gpu_step(name, res, under_profiler=False):
    """Runs `--step name` as a child under its time limit and merges the JSON line it prints; False where it failed."""
    command = [sys.executable, os.path.abspath(__file__), str(n_rows), "--step", name]
    work = None
    if under_profiler:
        rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if not os.path.exists(rocprof):
            res["kernel"] = "not measured: no rocprofv3"
            return True
        work = tempfile.mkdtemp(prefix="spline_time_")
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
            fits = launches.get("fit", [])
            if len(fits) == 3 * CALLS:                       # CALLS calls of one launch, then CALLS calls of two
                res["kernel_ms_one_spacing"] = min(fits[:CALLS]) / 1e6
                pairs = [fits[CALLS + 2 * k] + fits[CALLS + 2 * k + 1] for k in range(CALLS)]
                res["kernel_ms_eight_spacings"] = min(pairs) / 1e6
                res["pick_kernel_ms"] = min(launches.get("pick", [float("nan")])) / 1e6
            else:
                res["kernel"] = "not measured: %d fit launches in the trace, %d expected" % (len(fits), 3 * CALLS)
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
    t, flux, kw, ladder = rows_of("k2_90d")
    ctx = _lib.Context(0)
    res = {}
    if name == "kernel":       # (the profiled child: CALLS calls with one spacing, then CALLS with eight)
        for spacing in (SPACING, ladder):
            for _ in range(CALLS):
                survey.spline_batch(t, flux, spacing, n_iter=N_ITER, context=ctx)
    elif name == "call":
        survey.spline_batch(t, flux[:2], ladder, context=ctx)         # (warm: code objects)
        for label, spacing in (("one_spacing", SPACING), ("eight_spacings", ladder)):
            best, every, flat = best_of_three(lambda: survey.spline_batch(t, flux, spacing, n_iter=N_ITER, context=ctx))
            res["spline_batch_%s_s" % label], res["spline_batch_%s_every_s" % label] = best, every
            res["rms_flat_" + label] = float(numpy.std(flat))
        res["rms_raw"] = float(numpy.std(flux / flux.mean(axis=1, keepdims=True)))
    elif name == "search":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            survey.power_batch(t, flux[:64], detrend=survey.Spline(SPACING), context=ctx, **kw)
            for label, spacing in (("one_spacing", SPACING), ("eight_spacings", ladder)):
                flat = survey.spline_batch(t, flux, spacing, n_iter=N_ITER, context=ctx)
                detrend = survey.Spline(spacing if numpy.ndim(spacing) == 0 else tuple(spacing), n_iter=N_ITER)
                with_step = best_of_three(lambda: survey.power_batch(t, flux, detrend=detrend, context=ctx, **kw))[1]
                on_flat = best_of_three(lambda: survey.power_batch(t, flat, context=ctx, **kw))[1]
                res["power_batch_%s_every_s" % label] = {"detrend_spline": with_step, "on_flat_rows": on_flat}
                res["detrend_rate_ratio_" + label] = min(on_flat) / min(with_step)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    if step:
        child(step)
        sys.exit(0)
    t, flux, kw, ladder = rows_of("k2_90d")
    res = {"rows": n_rows, "n": len(t), "spacing": SPACING, "ladder": ladder.tolist(), "n_iter": N_ITER,
           "serial_factorisation_share": "not measured"}
    if host:
        bounds = numpy.linspace(0, n_rows, PROCESSES + 1).astype(int)
        with multiprocessing.get_context("fork").Pool(PROCESSES) as pool:
            for label, spacing in (("one_spacing", SPACING), ("eight_spacings", ladder)):
                jobs = [(t, flux[a:b], spacing) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
                for name, work in (("numpy_statement", statement_rows), ("make_lsq_spline_loop", scipy_rows)):
                    res["%s_%d_processes_%s_s" % (name, PROCESSES, label)] = best_of_three(lambda: pool.map(work, jobs))[0]
    ok = True
    for name, wanted, under in (("kernel", profile, True), ("call", True, False), ("search", search, False)):
        if ok and wanted:
            ok = gpu_step(name, res, under)
    for label in ("one_spacing", "eight_spacings"):
        call = res.get("spline_batch_%s_s" % label)
        for name in ("numpy_statement", "make_lsq_spline_loop"):
            host_s = res.get("%s_%d_processes_%s_s" % (name, PROCESSES, label))
            if call and host_s:
                res["speedup_over_%s_%s" % (name, label)] = host_s / call
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0 if ok else 1)
