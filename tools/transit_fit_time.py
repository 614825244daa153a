"""Developer tool: what the transit-fit stage of survey mode costs on 1024 k2_90d rows with K = 8 (the method of
tools/shape_fit_time.py: best of three runs of each call in one process, the calls taking turns).

In one run: survey.power_batch(peaks=8, statistics=True, peak_fits=True) -- the call without the stage -- and the same with
transit_fit=dict(window=1.5); the time the stage adds and where it goes: Context.transit_fit (upload, kernels, copy back) and
the assembly of the result.  survey.transit_fit alone on the same candidates, against the statement's vectorised form
(tests/transit_fit_spec.py) on 16 host processes that never open the GPU, on a sample of the candidates, scaled.  The
kernels' time a slab and a candidate comes from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child
process of its own, started before this process opens the GPU), and with the member-unit-sub-sample steps of the candidates
-- n_points * units * n_sub * passes -- the steps a second.  The results with and without the stage are compared byte for byte
on the way.

Usage: python tools/transit_fit_time.py [n_rows=1024] [--json OUT] [--no-profile] [--host-sample 64]"""

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
KERNELS = ("tls_transit_fit_kernel", "tls_times_pairs_kernel")
REQUEST = dict(window=1.5)       # (room for half an exposure beside the shortest duration of the grid)
HOST_PROCESSES = 16


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns(n_rows):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel times`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="transit_fit_time_")
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
    import transit_fit_spec as spec
    t, y_rows, dy_rows, tables, curve, period, T0, duration, rows = job
    return spec.transit_fit_batch(t, y_rows, dy_rows, period, T0, duration, curve, rows, *tables, window=REQUEST["window"])[:, 5]


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
    host_sample = int(option("--host-sample") or 64)
    profile = "--no-profile" not in args and not kernel_mode
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    t, flux, kw = rows_of("k2_90d", n_rows)
    with_shapes = dict(peaks=K, statistics=True, peak_fits=True, transit_fit=REQUEST)
    if kernel_mode:   # (the profiled child: one call, once warm and once more)
        ctx = _lib.Context(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                survey.power_batch(t, flux, context=ctx, **with_shapes, **kw)
        ctx.close()
        return
    kernels = kernel_ns(n_rows) if profile else None
    ctx = _lib.Context(0)
    runs = {
        "power_batch_peaks8_statistics_peak_fits": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=True,
                                                                              context=ctx, **kw),
        "power_batch_peaks8_statistics_peak_fits_transit_fit": lambda: survey.power_batch(t, flux, context=ctx, **with_shapes, **kw),
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
        fits, shaped = (last["power_batch_peaks8_statistics_peak_fits" + s] for s in ("", "_transit_fit"))
        same = fits[0].tobytes() == shaped[0].tobytes() and all(fits[2]["peaks"][k].tobytes() == shaped[2]["peaks"][k].tobytes()
                                                                for k in fits[2]["peaks"].dtype.names)
        # the stage's parts, on the candidates of the call
        p = shaped[2]["peaks"]
        curve, rank = numpy.nonzero(p["status"] == 0)
        period, T0, duration = p["period"][curve, rank], p["T0"][curve, rank], p["duration_days"][curve, rank]
        depth = 1.0 - p["depth"][curve, rank]
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, None, dict(kw))
        template = {k: kw[k] for k in ("u", "limb_dark", "transit_template") if k in kw}
        setup = survey._transit_fit_setup(t, None, None, None, None, 5, REQUEST["window"], 3, 1.0, None, template)
        tables = tuple(setup[k] for k in ("k_rows", "profile", "impact", "ratio", "shift", "sub"))
        rows = survey._seed_rows(setup["k_rows"], depth)
        device_s, raw = best_of(lambda: ctx.transit_fit(inp["t"], y_rows, dy_rows, period, T0, duration, rows, *tables,
                                                        curve=curve, window=REQUEST["window"]))
        alone_s, alone = best_of(lambda: survey.transit_fit(t, flux, period, T0, duration, depth, curve=curve, context=ctx,
                                                            **REQUEST, **kw))
    added = best["power_batch_peaks8_statistics_peak_fits_transit_fit"] - best["power_batch_peaks8_statistics_peak_fits"]
    units = len(tables[2]) * len(tables[3]) * len(tables[4])
    passes = 1.0 + (raw["row"] != raw["row_first"])
    steps = float(numpy.sum(numpy.nan_to_num(raw["n_points"] * passes)) * units * len(tables[5]))
    res = {"root": ROOT, "rows": n_rows, "n": len(t), "k": K, "best_s": best, "every_s": every, "candidates": int(len(curve)),
           "units": units, "members_mean": float(numpy.nanmean(raw["n_points"])), "members_max": float(numpy.nanmax(raw["n_points"])),
           "n_sub": int(len(tables[5])), "added_by_transit_fit_s": added, "results_equal_without_the_stage": bool(same),
           "context_transit_fit_s": device_s, "assembly_s": added - device_s, "survey_transit_fit_alone_s": alone_s,
           "second_passes": int((raw["row"] != raw["row_first"]).sum()),
           "member_unit_sub_sample_steps": steps, "fitted_candidates": int((raw["status"] == 0).sum()),
           "record_bytes": int(raw.nbytes)}
    if kernels:
        res["kernel_ns"] = {k: v for k, v in sorted(kernels.items())}
        for name in KERNELS:
            found = [v for k, v in kernels.items() if name in k]
            if found:   # (the child runs the call twice; the pairs kernel also serves the other stages' calls there: none here)
                res[name + "_launches_per_call"] = sum(v[0] for v in found) / 2
                res[name + "_us_per_call"] = sum(v[1] for v in found) / 2e3
        if KERNELS[0] + "_us_per_call" in res:
            us = res[KERNELS[0] + "_us_per_call"]
            res["kernel_us_per_slab"] = us / res[KERNELS[0] + "_launches_per_call"]
            res["kernel_us_per_candidate"] = us / max(1, len(curve))
            res["member_unit_sub_sample_steps_per_s"] = steps / (us * 1e-6)
    ctx.close()
    # the statement on HOST_PROCESSES fresh processes, on a sample of the candidates, scaled to all of them
    if host_sample > 0 and len(curve):
        import concurrent.futures
        import multiprocessing
        take = numpy.linspace(0, len(curve) - 1, min(host_sample, len(curve))).astype(int)
        parts = numpy.array_split(take, HOST_PROCESSES)
        jobs = [(inp["t"], y_rows, dy_rows, tables, curve[i], period[i], T0[i], duration[i], rows[i]) for i in parts if len(i)]
        with concurrent.futures.ProcessPoolExecutor(HOST_PROCESSES, mp_context=multiprocessing.get_context("spawn")) as pool:
            list(pool.map(host_part, [j[:4] + tuple(a[:1] for a in j[4:]) for j in jobs]))   # (warm: interpreters, imports)
            t0 = time.perf_counter()
            ses = numpy.concatenate(list(pool.map(host_part, jobs)))
            host_s = time.perf_counter() - t0
        res["host_statement_sample"] = int(len(take))
        res["host_statement_sample_s"] = host_s
        res["host_statement_all_s"] = host_s * len(curve) / len(take)
        res["host_statement_agrees"] = bool(numpy.array_equal(ses, raw["ses"][take], equal_nan=True))
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
