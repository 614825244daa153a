"""Developer tool: what transit-protected detrending costs on 1024 k2_90d rows, best of three runs of each in one process:
(1) survey.transit_mask for 8 candidates a curve (8192 at 1024 rows), (2) survey.biweight_batch at 0.5 d unmasked, with an
empty mask and with the pass-1 mask (the fitted peak of every curve with SDE >= 7 out of power_batch(detrend=Biweight(0.5))),
(3) survey.prewhiten_batch with dy (three pulsations a row, K = 3) unmasked and with that mask, (4)
survey.power_batch_protected against two plain power_batch(detrend=Biweight(0.5)) calls.  Kernel times come from a
rocprofv3 --kernel-trace --stats run of this tool on itself (--kernels: one call of each of (1) to (3)).
--only-unmasked times the calls that exist without the feature (biweight_batch, prewhiten_batch, power_batch(detrend=)) and
nothing else, for runs against an older build.
Usage: python tools/transit_protect_time.py [n_rows=1024] [--json OUT] [--only-unmasked] [--no-trace]"""
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
out_path = None
if "--json" in args:
    i = args.index("--json")
    out_path = args[i + 1]
    del args[i:i + 2]
flags = {a for a in args if a.startswith("--")}
args = [a for a in args if not a.startswith("--")]
n_rows = int(args[0]) if args else 1024
BW = survey.Biweight(0.5)
SDE_MIN = 7.0
SIGNALS = ((5.37, 5e-3), (7.91, 3e-3), (11.13, 2e-3))
KERNELS = ("tls_transit_mask_kernel", "tls_biweight_detrend", "tls_biweight_detrend_masked", "tls_biweight_fill",
           "tls_biweight_detrend_fallback", "tls_gls_prologue_kernel", "tls_gls_prologue_masked_kernel", "tls_nudft_kernel",
           "tls_gls_epilogue_kernel", "tls_prewhiten_step_kernel", "tls_prewhiten_step_masked_kernel",
           "tls_prewhiten_finish_kernel")


def rows_of(name):
    """n_rows copies of the seed-0 light curve of a configuration, each with noise and a slow trend of its own."""
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (n_rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    f *= 1.0 + 0.01 * numpy.sin(t[None, :] / rng.uniform(2.0, 6.0, (n_rows, 1)) + rng.uniform(0, 6.3, (n_rows, 1)))
    return t, f, kw


def pulsating(t, f):
    rng = numpy.random.default_rng(7)
    out = f.copy()
    for freq, amp in SIGNALS:
        nu = freq * rng.uniform(0.9, 1.1, (len(f), 1))
        out *= 1.0 + amp * numpy.sin(2.0 * numpy.pi * (nu * (t - t[0]) + rng.uniform(size=(len(f), 1))))
    return out, rng.uniform(2e-4, 4e-4, f.shape)


def kernel_ns():
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernels`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="transit_protect_time_")
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
t, k2, kw = rows_of("k2_90d")
puls, dy = pulsating(t, k2)
freqs = survey.variability_frequencies(t)
low = survey.gls_power_threshold(len(t), len(freqs), survey.PREWHITEN_FAP)
runs = {
    "biweight_batch": lambda: survey.biweight_batch(t, k2, 0.5, context=ctx),
    "prewhiten_batch_dy": lambda: survey.prewhiten_batch(t, puls, 3, 1, low, frequencies=freqs, dy_batch=dy, context=ctx),
    "power_batch_biweight": lambda: survey.power_batch(t, k2, detrend=BW, context=ctx, **kw),
}
res = {"rows": n_rows, "n": len(t), "n_freq": len(freqs)}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    if "--kernels" not in flags:                      # (warm: plan, device buffers, code objects; the trace counts whole calls only)
        survey.power_batch(t, k2[:64], detrend=BW, context=ctx, **kw)
    if "--only-unmasked" not in flags:
        first = survey.power_batch(t, k2, detrend=BW, peaks=1, peak_fits=True, context=ctx, **kw)
        summary, peaks = first[0], first[-1]["peaks"]
        use = (summary["SDE"] >= SDE_MIN)[:, None] & (peaks["status"] == 0)
        curve = numpy.broadcast_to(numpy.arange(n_rows)[:, None], use.shape)[use]
        pass1 = (peaks["period"][use], peaks["T0"][use], peaks["duration_days"][use], curve, n_rows)
        mask = survey.transit_mask(t, *pass1, context=ctx)
        empty = numpy.zeros_like(mask)
        rng = numpy.random.default_rng(3)
        many = (rng.uniform(1.0, 30.0, 8 * n_rows), t[0] + rng.uniform(0.0, 1.0, 8 * n_rows), rng.uniform(0.05, 0.4, 8 * n_rows),
                numpy.repeat(numpy.arange(n_rows), 8), n_rows)
        res.update(protected_curves=int(mask.any(axis=1).sum()), protected_fraction=float(mask.mean()),
                   candidates=8 * n_rows)
        masked = {
            "transit_mask_8_a_curve": lambda: survey.transit_mask(t, *many, context=ctx),
            "biweight_batch_empty_mask": lambda: survey.biweight_batch(t, k2, 0.5, mask=empty, context=ctx),
            "biweight_batch_pass1_mask": lambda: survey.biweight_batch(t, k2, 0.5, mask=mask, context=ctx),
            "prewhiten_batch_dy_pass1_mask": lambda: survey.prewhiten_batch(t, puls, 3, 1, low, frequencies=freqs, dy_batch=dy,
                                                                            mask=mask, context=ctx),
        }
        if "--kernels" in flags:
            for run in list(masked.values()) + [runs["biweight_batch"], runs["prewhiten_batch_dy"]]:
                run()
            sys.exit(0)
        runs.update(masked)
        runs.update({
            "power_batch_protected": lambda: survey.power_batch_protected(t, k2, BW, SDE_MIN, context=ctx, **kw),
            "power_batch_biweight_twice": lambda: [survey.power_batch(t, k2, detrend=BW, context=ctx, **kw) for _ in range(2)],
        })
    best, every = {}, {}
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            run()
            every.setdefault(name, []).append(time.perf_counter() - t0)
    best = {k: min(v) for k, v in every.items()}
res.update(best_s=best, every_s=every)
if "--only-unmasked" not in flags:
    res["ratio_biweight_empty_mask_vs_unmasked"] = best["biweight_batch_empty_mask"] / best["biweight_batch"]
    res["ratio_biweight_pass1_mask_vs_unmasked"] = best["biweight_batch_pass1_mask"] / best["biweight_batch"]
    res["ratio_prewhiten_masked_vs_dy"] = best["prewhiten_batch_dy_pass1_mask"] / best["prewhiten_batch_dy"]
    res["ratio_protected_vs_two_plain"] = best["power_batch_protected"] / best["power_batch_biweight_twice"]
    if "--no-trace" not in flags:
        ctx.close()
        trace = kernel_ns()
        res["kernel_ms"] = None if trace is None else {k: {"calls": c, "total_ms": ns / 1e6} for k, (c, ns) in sorted(trace.items())}
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
