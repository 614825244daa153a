"""Developer tool: what the single-transit search of survey mode costs (the method of tools/phase_scan_time.py: best of three
runs of each call in one process, the calls taking turns).

For 1024 k2_90d rows and 1024 tess_27d rows, each on its default width grid (survey.single_transit_widths):
  * the statistic kernel's time, from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process of
    its own, started before this process opens the GPU; no counters in that run), as window steps per second -- a step is one
    tap of one window, n * sum(widths) of them a curve -- and as a fraction of the bound of 16 steps a clock and CU that both
    the LDS pipe (16 bytes a step of 256 a clock) and the fp64 pipe (4 operations a step of 64 a clock) set, at the nominal
    256 CUs and 2.4 GHz;
  * the whole call survey.single_transits against the statement's vectorised numpy form (tests/single_transit_spec.py) in 16
    host processes (forked before this process opens the GPU; the statement's selection is a plain Python loop), timed on
    --spec-rows rows (default 32, two a process) and scaled to the batch;
and for the k2_90d rows power_batch(detrend=25) followed by single_transits(detrend=25) against power_batch(detrend=25) alone:
what adding the search to a survey pass costs.

Usage: python tools/single_transit_time.py [n_rows=1024] [--json OUT] [--no-profile] [--spec-rows N] [--configs k2_90d,tess_27d]"""
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
kernel_mode = option("--kernel")                      # a configuration's name: the profiled child
spec_rows = int(option("--spec-rows") or 32)
configs = (option("--configs") or "k2_90d,tess_27d").split(",")
profile = "--no-profile" not in args and not kernel_mode
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
STATISTIC, SELECT = "tls_single_statistic_kernel", "tls_single_select_kernel"
BOUND_STEPS_PER_S = 16 * 256 * 2.4e9                  # 16 steps a clock and CU, 256 CUs, 2.4 GHz
HOST_PROCESSES = 16
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


def kernel_ns(name):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel name`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="single_transit_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", name], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    kernel = rec.get("Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                    calls, total = out.get(kernel, (0, 0.0))
                    out[kernel] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
        return out or None
    finally:
        shutil.rmtree(work, ignore_errors=True)


CHILD_CALLS = 3
if kernel_mode:   # (the profiled child: the call, CHILD_CALLS times)
    t, flux, kw = rows_of(kernel_mode, n_rows)
    ctx = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(CHILD_CALLS):
            survey.single_transits(t, flux, context=ctx)
    ctx.close()
    sys.exit(0)

kernels = {name: kernel_ns(name) for name in configs} if profile else {}
import single_transit_spec as spec  # noqa: E402

SPEC = {}                                             # what a worker process reads (set before the fork)


def spec_part(part):
    return spec.expected(SPEC["t"], SPEC["y"][part], SPEC["dy"][part], SPEC["widths"], SPEC["shapes"], SPEC["span"])


# the statement first, in processes forked while this one has not opened the GPU
spec_runs = {}
for name in configs:
    t, flux, kw = rows_of(name, spec_rows)
    widths = survey.single_transit_widths(t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, None, dict(oversampling_factor=1))
    dt = float(numpy.median(numpy.diff(t)))
    SPEC.update(t=t, y=y_rows, dy=dy_rows, widths=widths, shapes=spec.shapes_of(widths, **inp["shape"]),
                span=[(int(L) - 1) * dt * 1.5 for L in widths])
    per = max(1, spec_rows // HOST_PROCESSES)
    parts = [slice(i, i + per) for i in range(0, spec_rows, per)]
    with multiprocessing.get_context("fork").Pool(HOST_PROCESSES) as pool:
        pool.map(spec_part, parts[:1])                # (the workers are up)
        t0 = time.perf_counter()
        want = pool.map(spec_part, parts)
        spec_runs[name] = (time.perf_counter() - t0, want)

ctx = _lib.Context(0)
res = {"rows": n_rows, "bound_steps_per_s": BOUND_STEPS_PER_S, "configs": {}}
for name in configs:
    t, flux, kw = rows_of(name, n_rows)
    widths = survey.single_transit_widths(t)
    spec_s, want = spec_runs[name]
    steps = float(n_rows) * len(t) * float(widths.sum())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = survey.single_transits(t, flux, context=ctx)       # (warm: device buffers, code objects, the shapes)
        best = float("inf")
        for rep in range(3):
            t0 = time.perf_counter()
            got = survey.single_transits(t, flux, context=ctx)
            best = min(best, time.perf_counter() - t0)
    same = all(numpy.array_equal(numpy.concatenate([w[0][f] for w in want]), got[0][f][:spec_rows], equal_nan=True)
               for f in spec.FIELDS)
    ev = got[0]
    rec = {"n": len(t), "widths": len(widths), "width_max": int(widths[-1]), "sum_widths": int(widths.sum()), "steps": steps,
           "call_best_s": best, "spec_rows": spec_rows, "spec_s": spec_s, "spec_s_scaled_to_batch": spec_s * n_rows / spec_rows,
           "device_equals_spec_on_those_rows": bool(same), "events_median": float(numpy.median(got[1])),
           "rank1_ses_median": float(numpy.nanmedian(ev["ses"][:, 0])), "rank2_ses_median": float(numpy.nanmedian(ev["ses"][:, 1]))}
    rec["call_over_spec"] = rec["spec_s_scaled_to_batch"] / best
    k = kernels.get(name)
    if k:
        rec["kernel_ns"] = {a: b for a, b in sorted(k.items())}
        stat = [v for a, v in k.items() if STATISTIC in a]
        sel = [v for a, v in k.items() if SELECT in a]
        if stat:
            per_call = sum(v[1] for v in stat) / 1e9 / CHILD_CALLS
            rec.update(statistic_kernel_s_per_call=per_call, statistic_launches_per_call=sum(v[0] for v in stat) / CHILD_CALLS,
                       steps_per_s=steps / per_call, fraction_of_bound=steps / per_call / BOUND_STEPS_PER_S)
        if sel:
            rec["select_kernel_s_per_call"] = sum(v[1] for v in sel) / 1e9 / CHILD_CALLS
    res["configs"][name] = rec

if "k2_90d" in configs:
    t, flux, kw = rows_of("k2_90d", n_rows)
    runs = {"power_batch_detrend25": lambda: survey.power_batch(t, flux, detrend=25, context=ctx, **kw),
            "power_batch_then_single_transits_detrend25": lambda: (survey.power_batch(t, flux, detrend=25, context=ctx, **kw),
                                                                   survey.single_transits(t, flux, detrend=25, context=ctx))}
    best = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for run in runs.values():
            run()
        for rep in range(3):
            for name, run in runs.items():
                t0 = time.perf_counter()
                run()
                best[name] = min(best.get(name, float("inf")), time.perf_counter() - t0)
    res["survey_pass_k2_90d"] = dict(best, added_s=best["power_batch_then_single_transits_detrend25"] - best["power_batch_detrend25"],
                                     added_fraction=best["power_batch_then_single_transits_detrend25"] / best["power_batch_detrend25"] - 1)
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
ctx.close()
