"""Developer tool: what the ephemeris match of survey mode costs (the method of tools/phase_scan_time.py: warm calls in one
process, the calls of a comparison taking turns).

In one run:
  - survey.ephemeris_match at M = 4096 and M = 32768 random candidates (1024 stars of 4 and of 32 peaks): the median of the
    warm calls, host clock around the whole call (copies in, both kernels, copy out, synchronise), and next to it the numpy
    statement tests/ephemeris_match_spec.py on the CPU, records compared field by field.  The statement is timed at M = 4096;
    its time at 32768 is that time scaled by (32768 / 4096)^2 = 64 unless --full-baseline runs it;
  - the two kernels' time per call at both M, from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child
    process of its own, started before this process opens the GPU), and the pairs a second that is;
  - survey.power_batch(peaks=8, peak_fits=True) on 1024 k2_90d rows with and without ephemeris_match=True, the calls taking
    turns: what the keyword adds, and the spread of the call without it.  The results are compared byte for byte on the way.

Usage: python tools/ephemeris_match_time.py [n_rows=1024] [--json OUT] [--no-profile] [--no-pipeline] [--full-baseline]"""
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
kernel_mode = option("--kernel")                      # "match": the profiled child
profile = "--no-profile" not in args and not kernel_mode
pipeline = "--no-pipeline" not in args
full_baseline = "--full-baseline" in args
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
K = 8
SIZES = (4096, 32768)
STARS = 1024
SPAN = 80.0
CALLS = 9
KERNELS = ("tls_match_pairs_kernel", "tls_match_combine_kernel")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tls_amd import _lib, survey, synthetic  # noqa: E402
import ephemeris_match_spec as spec  # noqa: E402


def candidates(m):
    """m random candidates, m / STARS peaks on each of STARS stars: periods of 0.5 to 40 d, epochs anywhere in the period,
    durations of 1 to 8 hours; one star in 32 repeats the ephemeris of another, so that matches exist."""
    rng = numpy.random.default_rng(m)
    star = numpy.repeat(numpy.arange(STARS), m // STARS)
    period = numpy.exp(rng.uniform(numpy.log(0.5), numpy.log(40.0), m))
    T0 = rng.uniform(0.0, 1.0, m) * period
    duration = rng.uniform(1.0, 8.0, m) / 24.0
    strength = rng.uniform(1e-4, 2e-2, m)
    copies = rng.choice(m, m // 32, replace=False)
    source = rng.integers(0, m, len(copies))
    period[copies] = period[source] * (1 + 1e-4 * rng.uniform(-1, 1, len(copies)))
    T0[copies] = T0[source] + 0.01 * rng.uniform(-1, 1, len(copies))
    return star, period, T0, duration, strength, SPAN


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns():
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel match`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    out = {}
    for m in SIZES:
        work = tempfile.mkdtemp(prefix="ephemeris_match_time_")
        try:
            subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                            os.path.abspath(__file__), "--kernel", str(m)], check=True, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, timeout=600)
            for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as fh:
                    for rec in csv.DictReader(fh):
                        name = rec.get("Name", "").split("(")[0].split("<")[0].replace("void ", "").replace("tlsdev::", "")
                        calls, total = out.get((m, name), (0, 0.0))
                        out[(m, name)] = (calls + int(rec["Calls"]), total + float(rec["TotalDurationNs"]))
        finally:
            shutil.rmtree(work, ignore_errors=True)
    return out or None


if kernel_mode:   # (the profiled child: CALLS calls at one M)
    ctx = _lib.Context(0)
    a = candidates(int(kernel_mode))
    for _ in range(CALLS):
        survey.ephemeris_match(*a, context=ctx)
    ctx.close()
    sys.exit(0)

kernels = kernel_ns() if profile else None
ctx = _lib.Context(0)
res = {"root": ROOT, "device": ctx.name, "stars": STARS, "calls": CALLS, "sizes": {}}
baseline_small = None
for m in SIZES:
    a = candidates(m)
    survey.ephemeris_match(*a, context=ctx)           # (warm: code objects, device buffers)
    times = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        got = survey.ephemeris_match(*a, context=ctx)
        times.append(time.perf_counter() - t0)
    entry = {"device_call_s_median": float(numpy.median(times)), "device_call_s_min": min(times), "device_call_s_max": max(times),
             "chunks": len(_lib.match_chunks(m)) - 1, "pairs": m * m,
             "matched": int((got["n_match"] > 0).sum()), "period_matched": int((got["n_period"] > 0).sum())}
    if m == SIZES[0] or full_baseline:
        t0 = time.perf_counter()
        want = spec.match(*a)
        entry["numpy_statement_s"] = time.perf_counter() - t0
        entry["numpy_statement_is"] = "measured"
        entry["equal_to_the_statement"] = all(numpy.array_equal(got[k], want[k], equal_nan=True) for k in spec.FIELDS)
        if m == SIZES[0]:
            baseline_small = entry["numpy_statement_s"]
    else:
        entry["numpy_statement_s"] = baseline_small * (m / SIZES[0]) ** 2
        entry["numpy_statement_is"] = "the time at M = %d scaled by (M / %d)^2, not measured" % (SIZES[0], SIZES[0])
    entry["numpy_over_device"] = entry["numpy_statement_s"] / entry["device_call_s_median"]
    if kernels:
        for name in KERNELS:
            found = [v for (mm, k), v in kernels.items() if mm == m and name in k]
            if found:
                entry[name + "_us_per_call"] = sum(v[1] for v in found) / 1e3 / sum(v[0] for v in found)
        if KERNELS[0] + "_us_per_call" in entry:
            entry["pairs_per_s"] = m * m / (entry[KERNELS[0] + "_us_per_call"] * 1e-6)
    res["sizes"][str(m)] = entry

if pipeline:
    t, flux, kw = rows_of("k2_90d", n_rows)
    runs = {
        "power_batch_peaks8_peak_fits": lambda: survey.power_batch(t, flux, peaks=K, peak_fits=True, context=ctx, **kw),
        "power_batch_peaks8_peak_fits_ephemeris_match": lambda: survey.power_batch(t, flux, peaks=K, peak_fits=True,
                                                                                   ephemeris_match=True, context=ctx, **kw),
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
    plain, matched = (last["power_batch_peaks8_peak_fits" + s] for s in ("", "_ephemeris_match"))
    same = plain[0].tobytes() == matched[0].tobytes() and all(plain[2]["peaks"][k].tobytes() == matched[2]["peaks"][k].tobytes()
                                                             for k in plain[2]["peaks"].dtype.names)
    p = matched[2]["peaks"]
    without, with_match = (seen["power_batch_peaks8_peak_fits" + s] for s in ("", "_ephemeris_match"))
    res["pipeline"] = {"rows": n_rows, "n": len(t), "k": K, "calls_s": seen,
                       "median_s": {k: float(numpy.median(v)) for k, v in seen.items()},
                       "added_by_ephemeris_match_s": float(numpy.median(with_match) - numpy.median(without)),
                       "added_over_the_call": float(numpy.median(with_match) / numpy.median(without) - 1),
                       "spread_of_the_call_without": float((max(without) - min(without)) / numpy.median(without)),
                       "results_equal_without_the_match": bool(same),
                       "candidates": int((p["match_status"] == 0).sum()), "matched": int((p["match_n_match"] > 0).sum()),
                       "largest_n_same": float(numpy.nanmax(p["match_n_same"]))}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
ctx.close()
