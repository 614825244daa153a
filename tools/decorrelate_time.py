"""Developer tool: regression detrending on 1024 k2_90d rows that follow a six-hour centroid roll, the five columns of
centroid_regressors(order=2) a row, with and without two shared columns, n_iter = 3, best of three runs of each in one process:
(a) kernel time per call, from a rocprofv3 --kernel-trace run of this tool's --kernel mode (a child process of its own,
    started before this process opens the GPU);
(b) the whole survey.decorrelate_batch call with its host round trip against the numpy statement (tests/decorrelate_spec.py)
    and against a plain numpy.linalg.lstsq loop with the same clip rounds, both on 16 host processes (started and finished
    before this process opens the GPU);
(c) survey.power_batch(detrend=Decorrelate(...)) against survey.power_batch on the rows decorrelated beforehand.
Usage: python tools/decorrelate_time.py [n_rows=1024] [--json OUT] [--no-profile] [--no-search] [--no-host]"""
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
from tls_amd import _lib, survey, synthetic  # noqa: E402
import decorrelate_spec  # noqa: E402

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
kernel_mode = _flag("--kernel")           # the profiled child
profile = not _flag("--no-profile")
search = not _flag("--no-search")
host = not _flag("--no-host")
n_rows = int(args[0]) if args else 1024
N_ITER = 3
CALLS = 3                                  # of the profiled child
PROCESSES = 16


def rows_of(name):
    """n_rows copies of the seed-0 light curve of a configuration, each with noise of its own, a roll of its own phase and
    its own response to it; and two shared profiles (a ramp and a 6-day sawtooth) every row carries."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + rng.uniform(2e-4, 6e-4, (n_rows, 1)) * rng.standard_normal(f.shape)
    phase = ((t - t[0])[None, :] / 0.25 + rng.uniform(0.0, 1.0, (n_rows, 1))) % 1.0
    cx = 0.22 * (2.0 * phase - 1.0) + 0.005 * rng.standard_normal(f.shape)
    cy = 0.3 * cx + 0.1 * numpy.sin(2.0 * numpy.pi * t / 3.1)[None, :] + 0.005 * rng.standard_normal(f.shape)
    a, b, c = (rng.normal(0.0, s, (n_rows, 1)) for s in (0.01, 0.03, 0.004))
    f *= 1.0 + a * cx + b * cx * cx + c * cy
    shared = numpy.stack([(t - t.mean()) / (t.max() - t.min()), ((t - t[0]) % 6.0) / 6.0 - 0.5])
    f *= 1.0 + rng.normal(0.0, 3e-3, (n_rows, 2)) @ shared
    return t, f, survey.centroid_regressors(cx, cy, order=2), shared, kw


def lstsq_rows(job):
    """The plain fit of a slice of rows: numpy.linalg.lstsq on the standardised columns, N_ITER clip rounds at 5 sigma."""
    y, own, shared = job
    flat = numpy.empty_like(y)
    for i in range(len(y)):
        X = own[i] if shared is None else numpy.concatenate([shared, own[i]])
        keep = numpy.ones(y.shape[1], dtype=bool)
        for _ in range(N_ITER + 1):
            mu = y[i][keep].mean()
            z = y[i] / mu - 1.0
            mean, scale = X[:, keep].mean(axis=1), X[:, keep].std(axis=1)
            u = ((X - mean[:, None]) / scale[:, None]).T
            coef = numpy.linalg.lstsq(u[keep], z[keep], rcond=None)[0]
            r = z - u @ coef
            out = keep & (numpy.abs(r) > 5.0 * numpy.sqrt(numpy.mean(r[keep] ** 2)))
            if not out.any():
                break
            keep &= ~out
        flat[i] = y[i] / (mu * (1.0 + u @ coef))
    return flat


def statement_rows(job):
    y, own, shared = job
    return decorrelate_spec.fit(y, shared=shared, own=own, n_iter=N_ITER)["flat"]


def kernel_launches():
    """[duration ns of every tls_decorrelate_kernel launch] of a rocprofv3 --kernel-trace run of `--kernel`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="decorrelate_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        out = []
        for path in glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    if "tls_decorrelate_kernel" in rec.get("Kernel_Name", ""):
                        out.append(float(rec["End_Timestamp"]) - float(rec["Start_Timestamp"]))
        return out or None
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    t, flux, own, shared, kw = rows_of("k2_90d")
    n = len(t)
    if kernel_mode:   # (the profiled child: CALLS calls without and CALLS with the shared columns, in that order)
        ctx = _lib.Context(0)
        for columns in (None, shared):
            for _ in range(CALLS):
                survey.decorrelate_batch(flux, own=own, shared=columns, n_iter=N_ITER, context=ctx)
        ctx.close()
        sys.exit(0)

    res = {"rows": n_rows, "n": n, "own_columns": own.shape[1], "shared_columns": len(shared), "n_iter": N_ITER}
    if profile:
        launches = kernel_launches()
        if launches and len(launches) % (2 * CALLS) == 0:
            per_call = len(launches) // (2 * CALLS)
            calls = [sum(launches[i * per_call:(i + 1) * per_call]) / 1e6 for i in range(2 * CALLS)]
            res["kernel_launches_per_call"] = per_call
            res["kernel_ms_per_call_own_only"], res["kernel_ms_per_call_with_shared"] = min(calls[:CALLS]), min(calls[CALLS:])
    if host:   # (before this process opens the GPU: the workers are forked)
        bounds = numpy.linspace(0, n_rows, PROCESSES + 1).astype(int)
        with multiprocessing.get_context("fork").Pool(PROCESSES) as pool:
            for label, columns in (("own_only", None), ("with_shared", shared)):
                jobs = [(flux[a:b], own[a:b], columns) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
                for name, work in (("numpy_statement", statement_rows), ("lstsq_loop", lstsq_rows)):
                    every = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        parts = pool.map(work, jobs)
                        every.append(time.perf_counter() - t0)
                    res["%s_%d_processes_%s_s" % (name, PROCESSES, label)] = min(every)
                    if name == "numpy_statement":
                        res["statement_" + label] = numpy.concatenate(parts)

    ctx = _lib.Context(0)
    survey.decorrelate_batch(flux[:2], own=own[:2], shared=shared, context=ctx)   # (warm: code objects)
    flat = None
    for label, columns in (("own_only", None), ("with_shared", shared)):
        every = []
        for _ in range(3):
            t0 = time.perf_counter()
            flat = survey.decorrelate_batch(flux, own=own, shared=columns, n_iter=N_ITER, context=ctx)
            every.append(time.perf_counter() - t0)
        res["decorrelate_batch_%s_s" % label], res["decorrelate_batch_%s_every_s" % label] = min(every), every
        want = res.pop("statement_" + label, None)
        if want is not None:
            res["equals_statement_" + label] = bool(want.tobytes() == flat.tobytes())
            res["speedup_over_statement_" + label] = res["numpy_statement_%d_processes_%s_s" % (PROCESSES, label)] / min(every)
            res["speedup_over_lstsq_" + label] = res["lstsq_loop_%d_processes_%s_s" % (PROCESSES, label)] / min(every)
    res["rms_raw"] = float(numpy.std(flux / flux.mean(axis=1, keepdims=True)))
    res["rms_flat"] = float(numpy.std(flat))
    if search:
        step = survey.Decorrelate(own=own, shared=shared, n_iter=N_ITER)
        runs = {"power_batch_detrend_decorrelate": lambda: survey.power_batch(t, flux, detrend=step, context=ctx, **kw),
                "power_batch_on_flat_rows": lambda: survey.power_batch(t, flat, context=ctx, **kw)}
        every = {k: [] for k in runs}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            survey.power_batch(t, flux[:64], detrend=survey.Decorrelate(own=own[:64], shared=shared), context=ctx, **kw)
            for rep in range(3):
                for name, run in runs.items():
                    t0 = time.perf_counter()
                    run()
                    every[name].append(time.perf_counter() - t0)
        res["power_batch_every_s"] = every
        res["detrend_rate_ratio"] = min(every["power_batch_on_flat_rows"]) / min(every["power_batch_detrend_decorrelate"])
    ctx.close()
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
