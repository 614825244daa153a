"""Developer tool: SysRem on 1024 k2_90d rows with two shared systematics, K = 2, best of three runs of each in one process:
(a) kernel time per call and per iteration, from a rocprofv3 --kernel-trace run of this tool's --kernel mode (a child process
    of its own, started before this process opens the GPU), with the achieved bytes/s of the columns and rows passes against
    their algorithmic bytes;
(b) the whole survey.sysrem_batch call with its host round trip against a plain vectorised numpy version of the same
    iteration (matrix-vector products on the host's BLAS threads; not the bit-exact restatement), run for the iterations the
    device ran;
(c) survey.power_batch(detrend=SysRem(2)) against survey.power_batch on the rows detrended beforehand.
Usage: python tools/sysrem_time.py [n_rows=1024] [--json OUT] [--no-profile] [--no-search]"""
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tls_amd import _lib, survey, synthetic  # noqa: E402

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
kernel_out = _option("--kernel")          # the profiled child: where it writes the iterations it ran
profile = not _flag("--no-profile")
search = not _flag("--no-search")
n_rows = int(args[0]) if args else 1024
K = 2
CALLS = 3                                  # of the profiled child


def rows_of(name):
    """n_rows copies of the seed-0 light curve of a configuration, each with noise of its own and its own share of two
    systematics all rows carry: a ramp and a 6-day sawtooth, coefficients of a few 1e-3."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + rng.uniform(2e-4, 6e-4, (n_rows, 1)) * rng.standard_normal(f.shape)
    ramp = (t - t.mean()) / (t.max() - t.min())
    saw = ((t - t[0]) % 6.0) / 6.0 - 0.5
    f *= 1.0 + rng.normal(0.0, 3e-3, (n_rows, 1)) * ramp + rng.normal(0.0, 3e-3, (n_rows, 1)) * saw
    return t, f, kw


def numpy_sysrem(y, iters):
    """The same fit in plain numpy, iters[k] iterations of component k: one weight a row, so both reductions are
    matrix-vector products."""
    m = y.mean(axis=1)
    x = y / m[:, None] - 1.0
    w = 1.0 / numpy.mean(x * x, axis=1)
    s = numpy.zeros_like(x)
    for n_iter in iters:
        c = numpy.ones(len(y))
        for _ in range(int(n_iter)):
            cw = c * w
            a = (cw @ x) / (cw @ c)
            c = (x @ a) / (a @ a)
        term = numpy.outer(c, a)
        x -= term
        s += term
    return y / (m[:, None] * (1.0 + s))


def kernel_launches(iters_path):
    """{kernel name: [duration ns of every launch]} of a rocprofv3 --kernel-trace run of `--kernel`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="sysrem_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", iters_path], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        out = {}
        for path in glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    name = rec.get("Kernel_Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                    if name.startswith("tls_sysrem"):
                        out.setdefault(name, []).append(float(rec["End_Timestamp"]) - float(rec["Start_Timestamp"]))
        return out or None
    finally:
        shutil.rmtree(work, ignore_errors=True)


t, flux, kw = rows_of("k2_90d")
n = len(t)
if kernel_out:   # (the profiled child: CALLS calls, the first one warms)
    ctx = _lib.Context(0)
    for _ in range(CALLS):
        iters = survey.sysrem_batch(flux, K, return_components=True, context=ctx)[1][2]
    ctx.close()
    with open(kernel_out, "w") as fh:
        json.dump([int(v) for v in iters], fh)
    sys.exit(0)

res = {"rows": n_rows, "n": n, "components": K}
if profile:
    iters_file = tempfile.NamedTemporaryFile(suffix=".json", delete=False)
    iters_file.close()
    launches = kernel_launches(iters_file.name)
    if launches:
        with open(iters_file.name) as fh:
            ran = sum(json.load(fh))
        chunks = -(-n_rows // _lib.SYSREM_ROW_CHUNK)
        algorithmic = {"tls_sysrem_columns": 8.0 * (n_rows * n + n_rows + 2 * chunks * n),   # x, c, and the partials written
                       "tls_sysrem_rows": 8.0 * (n_rows * n + n)}                            # x and a
        kernels = {}
        for name, ns in sorted(launches.items()):
            rec = {"launches_per_call": len(ns) / CALLS, "ms_per_call": sum(ns) / CALLS / 1e6}
            if name in ("tls_sysrem_columns", "tls_sysrem_epochs", "tls_sysrem_rows"):
                # the launches that ran an iteration are the long ones; the others returned on the flag
                ns = sorted(ns, reverse=True)
                active, idle = ns[:ran * CALLS], ns[ran * CALLS:]
                rec["us_per_iteration"] = sum(active) / len(active) / 1e3
                rec["us_per_returning_launch"] = sum(idle) / len(idle) / 1e3 if idle else None
                if name in algorithmic:
                    rec["algorithmic_bytes"] = algorithmic[name]
                    rec["achieved_GB_per_s"] = algorithmic[name] / (sum(active) / len(active))
            kernels[name] = rec
        res["iterations_run"] = ran
        res["kernels"] = kernels
        res["kernel_ms_per_call"] = sum(r["ms_per_call"] for r in kernels.values())
        res["kernel_us_per_iteration"] = sum(r.get("us_per_iteration", 0.0) for r in kernels.values())
    os.unlink(iters_file.name)

ctx = _lib.Context(0)
flat, (c, a, iters) = survey.sysrem_batch(flux, K, return_components=True, context=ctx)   # (warm: device buffers, code objects)
host = numpy_sysrem(flux, iters)
res["iters"] = [int(v) for v in iters]
res["max_abs_difference_numpy_vs_device"] = float(numpy.max(numpy.abs(host - flat)))
runs = {
    "sysrem_batch": lambda: survey.sysrem_batch(flux, K, context=ctx),
    "numpy_same_iterations": lambda: numpy_sysrem(flux, iters),
}
if search:
    SR = survey.SysRem(K)
    runs.update({
        "power_batch_sysrem": lambda: survey.power_batch(t, flux, detrend=SR, context=ctx, **kw),
        "power_batch_detrended_rows": lambda: survey.power_batch(t, flat, context=ctx, **kw),
    })
best = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    if search:
        survey.power_batch(t, flux[:64], detrend=survey.SysRem(K), context=ctx, **kw)
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
res["best_s"] = best
res["ratio_numpy_vs_sysrem_batch"] = best["numpy_same_iterations"] / best["sysrem_batch"]
if search:
    res["ratio_power_batch_sysrem_vs_detrended_rows"] = best["power_batch_detrended_rows"] / best["power_batch_sysrem"]
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
