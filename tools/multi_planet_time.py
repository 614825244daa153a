"""Developer tool: what the multi-planet search costs on 1024 k2_90d rows, best of three runs of each in one process.  The rows
are white noise of 2e-4; 5 % of them (every 20th) carry two planets (rp 0.08 at 4.3 d and rp 0.05 at 9.7 d).
(1) survey.remove_transits with the pass-0 fit of every row (1024 candidates), and its kernel from a rocprofv3
--kernel-trace --stats run of this tool on itself (--kernels: that one call), (2) survey.power_batch_multi(sde_min=9,
n_planets=3) against pass 0 alone (power_batch(peaks=1, peak_fits=True, transit_fit=True)): about one plus the continuing
share is expected, (3) plain survey.power_batch, for runs against another build (--only-plain times nothing else).
Usage: python tools/multi_planet_time.py [n_rows=1024] [--json OUT] [--only-plain] [--no-trace]"""
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
from tls_amd import _lib, survey, synthetic, transit_model  # noqa: E402

args = sys.argv[1:]
out_path = None
if "--json" in args:
    i = args.index("--json")
    out_path = args[i + 1]
    del args[i:i + 2]
flags = {a for a in args if a.startswith("--")}
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
SDE_MIN = 9.0
U = [0.4804, 0.1867]
KERNELS = ("tls_remove_transits_kernel",)


def rows_of(name):
    """n_rows rows of white noise on the time stamps of a configuration, every 20th with two planets."""
    t, _, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = 1.0 + 2e-4 * rng.standard_normal((n_rows, len(t)))
    two = transit_model.light_curve(t, t[0] + 1.1, 4.3, 0.08, 11.0, 90, 0, 90, U, "quadratic") \
        * transit_model.light_curve(t, t[0] + 2.3, 9.7, 0.05, 19.0, 90, 0, 90, U, "quadratic")
    f[::20] *= two
    return t, f, kw


def kernel_ns():
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernels`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="multi_planet_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernels"], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for rec in csv.DictReader(fh):
                    name = rec.get("Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                    calls, total = out.get(name, (0, 0.0))
                    out[name] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
        return {k: v for k, v in out.items() if k in KERNELS} or None
    except subprocess.SubprocessError as e:           # (no trace: the other measurements are taken all the same)
        print("kernel trace failed: %r" % (e,), file=sys.stderr)
        return None
    finally:
        shutil.rmtree(work, ignore_errors=True)


ctx = _lib.Context(0)
t, rows, kw = rows_of("k2_90d")
runs = {"power_batch": lambda: survey.power_batch(t, rows, context=ctx, **kw)}
res = {"rows": n_rows, "n": len(t), "two_planet_rows": len(rows[::20])}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    if "--kernels" not in flags:                      # (warm: plan, device buffers, code objects; the trace counts whole calls only)
        survey.power_batch(t, rows[:64], context=ctx, **kw)
    if "--only-plain" not in flags:
        first = survey.power_batch(t, rows, peaks=1, peak_fits=True, transit_fit=True, context=ctx, **kw)
        planets = first[-1]["peaks"]
        if "--kernels" in flags:
            survey.remove_transits(t, rows, planets, context=ctx)
            sys.exit(0)
        status = survey.remove_transits(t, rows, planets, return_status=True, context=ctx)[1]
        found, info = survey.power_batch_multi(t, rows, SDE_MIN, n_planets=3, context=ctx, **kw)
        res.update(candidates=int(planets.size), candidates_divided_out=int((status == 0).sum()),
                   searched_by_pass=[len(s) for s in info["searched"]],
                   n_found_two_planet_rows=info["n_found"][::20].tolist(), n_found_other_rows_max=int(numpy.delete(
                       info["n_found"], numpy.arange(0, n_rows, 20)).max()) if n_rows > 1 else 0)
        runs.update({
            "remove_transits": lambda: survey.remove_transits(t, rows, planets, context=ctx),
            "pass_0_alone": lambda: survey.power_batch(t, rows, peaks=1, peak_fits=True, transit_fit=True, context=ctx, **kw),
            "power_batch_multi": lambda: survey.power_batch_multi(t, rows, SDE_MIN, n_planets=3, context=ctx, **kw),
        })
    every = {}
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            every.setdefault(name, []).append(time.perf_counter() - t0)
    best = {k: min(v) for k, v in every.items()}
res.update(best_s=best, every_s=every)
if "--only-plain" not in flags:
    res["ratio_multi_vs_pass_0"] = best["power_batch_multi"] / best["pass_0_alone"]
    res["expected_ratio"] = float(sum(res["searched_by_pass"])) / n_rows
    if "--no-trace" not in flags:
        ctx.close()
        trace = kernel_ns()
        res["kernel_ms"] = None if trace is None else {k: {"calls": c, "total_ms": ns / 1e6} for k, (c, ns) in sorted(trace.items())}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
