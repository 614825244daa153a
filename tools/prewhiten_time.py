"""Developer tool: what iterative pre-whitening costs on 1024 k2_90d rows with three pulsations each (the method of
tools/lomb_scargle_time.py: best of three runs of each call in one process, the calls taking turns).

In one run, with K = 3 terms and H = 1:
  1. survey.prewhiten_batch against the composition existing calls allow: K rounds of survey.lomb_scargle(with_arrays=True)
     with the pick, the parabola, the weighted fit and the subtraction vectorised in numpy on the host (the same arithmetic,
     sums in numpy's order);
  2. survey.power_batch(detrend=Prewhiten(3)) against survey.power_batch on the rows pre-whitened beforehand;
  3. the kernels' times from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process of its own,
     started before this process opens the GPU; no counters are collected in it): the share of the product and of the step
     kernel in the device loop.

Usage: python tools/prewhiten_time.py [n_rows=1024] [--json OUT] [--no-profile] [--no-search]"""

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
K, H = 3, 1
KERNELS = ("tls_nudft_kernel", "tls_gls_prologue_kernel", "tls_gls_epilogue_kernel", "tls_prewhiten_step_kernel",
           "tls_prewhiten_finish_kernel")
SIGNALS = ((5.37, 5e-3), (7.91, 3e-3), (11.13, 2e-3))
TWO_PI = 6.283185307179586


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise and three pulsations of its own."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    for freq, amp in SIGNALS:
        nu = freq * rng.uniform(0.9, 1.1, (rows, 1))
        f *= 1.0 + amp * numpy.sin(TWO_PI * (nu * (t - t[0]) + rng.uniform(size=(rows, 1))))
    return t, f, kw


def kernel_ns(n_rows):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel times`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="prewhiten_time_")
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


def best_of(run, reps=3):
    every, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = run()
        every.append(time.perf_counter() - t0)
    return min(every), every, last


def host_composition(ctx, t, flux, freqs):
    """K rounds of the device's periodogram, everything else in numpy: (flat, the frequencies fitted [rows, K])."""
    from tls_amd import survey
    r = flux.copy()
    trend = numpy.zeros_like(r)
    lead = t - t[0]
    rows = numpy.arange(len(r))
    w = 1.0 / r.shape[1]
    mean0 = None
    fitted = []
    for _ in range(K):
        out = survey.lomb_scargle(t, r, freqs, with_arrays=True, context=ctx)
        if mean0 is None:
            mean0 = out["mean"]
        power = out["power"]
        k = numpy.argmax(power, axis=1)
        inner = numpy.clip(k, 1, len(freqs) - 2)
        left, peak, right = power[rows, inner - 1], power[rows, inner], power[rows, inner + 1]
        den = left - 2.0 * peak + right
        ok = (k == inner) & (den < 0.0)
        half = 0.5 * (freqs[inner + 1] - freqs[inner - 1])
        with numpy.errstate(all="ignore"):
            fstar = numpy.where(ok, freqs[inner] + 0.5 * half * (left - right) / den, freqs[k])
        fitted.append(fstar)
        x = fstar[:, None] * lead[None, :]
        phi = TWO_PI * (x - numpy.floor(x))
        c1, s1 = numpy.cos(phi), numpy.sin(phi)
        x2 = (2.0 * fstar)[:, None] * lead[None, :]
        phi2 = TWO_PI * (x2 - numpy.floor(x2))
        d = r - (w * r).sum(axis=1, keepdims=True)
        a = w * d
        YC, YS = (a * c1).sum(axis=1), (a * s1).sum(axis=1)
        C, S = w * c1.sum(axis=1), w * s1.sum(axis=1)
        C2, S2 = w * numpy.cos(phi2).sum(axis=1), w * numpy.sin(phi2).sum(axis=1)
        CC, SS, CS = 0.5 * (1.0 + C2) - C * C, 0.5 * (1.0 - C2) - S * S, 0.5 * S2 - C * S
        D = CC * SS - CS * CS
        ca, sa = (YC * SS - YS * CS) / D, (YS * CC - YC * CS) / D
        q = ca[:, None] * (c1 - C[:, None]) + sa[:, None] * (s1 - S[:, None])
        r -= q
        trend += q
    return flux / (mean0[:, None] + trend), numpy.array(fitted).T


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
    profile = "--no-profile" not in args and not kernel_mode
    search = "--no-search" not in args
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    t, flux, kw = rows_of("k2_90d", n_rows)
    freqs = survey.variability_frequencies(t)

    def device(ctx):
        return survey.prewhiten_batch(t, flux, K, H, 0.0, frequencies=freqs, return_terms=True, context=ctx)

    if kernel_mode:   # (the profiled child: the call once warm and once more)
        ctx = _lib.Context(0)
        for _ in range(2):
            device(ctx)
        ctx.close()
        return
    kernels = kernel_ns(n_rows) if profile else None
    ctx = _lib.Context(0)
    res = {"rows": n_rows, "n": len(t), "frequencies": len(freqs), "n_terms": K, "harmonics": H}
    survey.prewhiten_batch(t, flux[:2], K, H, 0.0, frequencies=freqs, context=ctx)       # (warm: code objects)
    survey.lomb_scargle(t, flux[:2], freqs, context=ctx)
    runs = {"prewhiten_batch": lambda: device(ctx), "host_composition": lambda: host_composition(ctx, t, flux, freqs)}
    every, last = {}, {}
    for rep in range(3):
        for name, run in runs.items():
            t0 = time.perf_counter()
            last[name] = run()
            every.setdefault(name, []).append(time.perf_counter() - t0)
    res["prewhiten_batch_s"], res["prewhiten_batch_every_s"] = min(every["prewhiten_batch"]), every["prewhiten_batch"]
    res["host_composition_s"], res["host_composition_every_s"] = min(every["host_composition"]), every["host_composition"]
    res["speedup_over_host_composition"] = res["host_composition_s"] / res["prewhiten_batch_s"]
    flat, info = last["prewhiten_batch"]
    host_flat, host_f = last["host_composition"]
    res["iterations_run"] = int(info["n_iterations"].sum())
    res["rms_before"], res["rms_after"] = float(numpy.std(flux, axis=1).mean()), float(numpy.std(flat, axis=1).mean())
    res["max_flat_difference_from_host_composition"] = float(numpy.abs(flat - host_flat).max())
    res["max_frequency_difference_from_host_composition"] = float(numpy.abs(info["terms"]["frequency"][:, :, 0] - host_f).max())
    res["one_periodogram_s"] = best_of(lambda: survey.lomb_scargle(t, flux, freqs, context=ctx))[0]
    if kernels:
        res["kernel_ns"] = {k: v for k, v in sorted(kernels.items())}
        total = 0.0
        for name in KERNELS:
            found = [v for k, v in kernels.items() if name in k]
            if found:   # (the child runs the call twice)
                res[name + "_us_per_call"] = sum(v[1] for v in found) / 2e3
                res[name + "_launches_per_call"] = sum(v[0] for v in found) / 2.0
                total += res[name + "_us_per_call"]
        res["kernels_us_per_call"] = total
        if total:
            res["product_share_of_kernel_time"] = res.get("tls_nudft_kernel_us_per_call", 0.0) / total
            res["step_share_of_kernel_time"] = res.get("tls_prewhiten_step_kernel_us_per_call", 0.0) / total
    if search:
        step = survey.Prewhiten(K, H, 0.0)
        runs = {"power_batch_detrend_prewhiten": lambda: survey.power_batch(t, flux, detrend=step, context=ctx, **kw),
                "power_batch_on_flat_rows": lambda: survey.power_batch(t, flat, context=ctx, **kw)}
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
        res["best_s"], res["every_s"] = best, every
        a, b = last["power_batch_detrend_prewhiten"][0], last["power_batch_on_flat_rows"][0]
        res["results_equal"] = bool(all(a[k].tobytes() == b[k].tobytes() for k in b.dtype.names))
        res["detrend_rate_ratio"] = best["power_batch_on_flat_rows"] / best["power_batch_detrend_prewhiten"]
    ctx.close()
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
