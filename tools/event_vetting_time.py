"""Developer tool: what the event-vetting stage of survey mode costs on 1024 k2_90d rows with K = 8 (the method of
tools/transit_times_time.py: best of three runs of each call in one process, the calls taking turns).

In one run: survey.power_batch(peaks=8, statistics=True) -- the call without the peak-fit stage --, the same with
peak_fits=True and the same with peak_fits=True, event_vetting=True; the time the peak-fit stage adds and the time the event
vetting adds behind it, and where that time goes: the rows and shapes formed on the host, Context.event_vetting (upload, kernels,
copy back) and the assembly of the result.  survey.event_vetting alone on the same candidates, against the statement's
vectorised form (tests/event_vetting_spec.py) on 16 host processes that never open the GPU, on a sample of the candidates.

The kernels' time comes from rocprofv3 --kernel-trace --stats runs of this tool's --kernel mode (child processes of their own,
started before this process opens the GPU).  The child runs power_batch(..., transit_times=True, event_vetting=True), so
tls_transit_times_kernel and tls_event_vetting_kernel see the same candidates in the same trace.  A second trace runs the same
call with a guard beyond every chase reach, so no chase window is left: the difference of tls_event_vetting_kernel's two times
is the chase pass.  Its taps are counted exactly from the records (the sum of n_chased * L); the transit-times kernel's taps are
its window steps, n_epochs * (2 reach + 1) * L, the statement's upper bound (windows outside the series are counted though not
walked), so its rate is an upper estimate.  The results with and without the stage are compared byte for byte on the way.

Usage: python tools/event_vetting_time.py [n_rows=1024] [--json OUT] [--no-profile] [--host-sample 512]"""
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
KERNELS = ("tls_event_vetting_kernel", "tls_transit_times_kernel", "tls_times_pairs_kernel")
HOST_PROCESSES = 16
NO_CHASE_GUARD = 1e6                                  # durations: beyond every chase reach


def rows_of(name, rows):
    """`rows` copies of the seed-0 light curve of a configuration, each with noise of its own."""
    from tls_amd import synthetic
    t, f0, kw = synthetic.config(name, seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    return t, f, kw


def kernel_ns(n_rows, mode):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel mode`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="event_vetting_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", mode], check=True, stdout=subprocess.DEVNULL,
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
    import event_vetting_spec as spec
    t, y_rows, dy_rows, curve, period, T0, row, reach, chase_reach, guard, chase_span, shapes, span_max, max_epochs = job
    return spec.expected(t, y_rows, dy_rows, curve, period, T0, row, reach, chase_reach, guard, chase_span, shapes, span_max,
                         max_epochs=max_epochs)[0]["n_good"]


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
    kernel_mode = option("--kernel")                  # "chase" / "nochase": the profiled children
    host_sample = int(option("--host-sample") or 512)
    profile = "--no-profile" not in args and not kernel_mode
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    from tls_amd.template import reference_transit
    t, flux, kw = rows_of("k2_90d", n_rows)
    with_events = dict(peaks=K, statistics=True, peak_fits=True, event_vetting=True)
    if kernel_mode:   # (a profiled child: one call, once warm and once more)
        ctx = _lib.Context(0)
        more = dict(event_vetting_guard=NO_CHASE_GUARD) if kernel_mode == "nochase" else {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                survey.power_batch(t, flux, context=ctx, transit_times=True, **with_events, **more, **kw)
        ctx.close()
        return
    kernels = kernel_ns(n_rows, "chase") if profile else None
    bare = kernel_ns(n_rows, "nochase") if profile else None
    ctx = _lib.Context(0)
    runs = {
        "power_batch_peaks8_statistics": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, context=ctx, **kw),
        "power_batch_peaks8_statistics_peak_fits": lambda: survey.power_batch(t, flux, peaks=K, statistics=True, peak_fits=True,
                                                                              context=ctx, **kw),
        "power_batch_peaks8_statistics_peak_fits_event_vetting": lambda: survey.power_batch(t, flux, context=ctx, **with_events, **kw),
    }
    best, last, every = {}, {}, {name: [] for name in runs}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for run in runs.values():   # (warm: plan, device buffers, code objects)
            run()
        for rep in range(3):
            for name, run in runs.items():
                t0 = time.perf_counter()
                last[name] = run()
                every[name].append(time.perf_counter() - t0)
                best[name] = min(every[name])
        fits, vetted = (last["power_batch_peaks8_statistics_peak_fits" + s] for s in ("", "_event_vetting"))
        same = fits[0].tobytes() == vetted[0].tobytes() and all(fits[2]["peaks"][k].tobytes() == vetted[2]["peaks"][k].tobytes()
                                                                for k in fits[2]["peaks"].dtype.names)
        # the stage's parts, on the candidates of the call
        p = vetted[2]["peaks"]
        curve, rank = numpy.nonzero(p["status"] == 0)
        period, T0, duration = p["period"][curve, rank], p["T0"][curve, rank], p["duration_days"][curve, rank]
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, None, dict(kw))
        max_epochs = vetted[2]["events"].shape[2]

        def rows_and_shapes():
            rows = survey.event_vetting_rows(inp["t"], period, duration)
            return rows + ([1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in rows[0]],)

        rows_s, (widths, span_max, row, reach, chase_reach, guard, chase_span, shapes) = best_of(rows_and_shapes)
        device_s, raw = best_of(lambda: ctx.event_vetting(inp["t"], y_rows, dy_rows, period, T0, row, reach, chase_reach, guard,
                                                          chase_span, widths, shapes, span_max, curve=curve, max_epochs=max_epochs))
        alone_s, alone = best_of(lambda: survey.event_vetting(t, flux, period, T0, duration, curve=curve, max_epochs=max_epochs,
                                                              context=ctx, **kw))
    added = best["power_batch_peaks8_statistics_peak_fits_event_vetting"] - best["power_batch_peaks8_statistics_peak_fits"]
    window_steps = float(numpy.sum(numpy.nan_to_num(raw[0]["n_epochs"]) * (2 * reach + 1) * widths[row]))
    chase_taps = float(numpy.sum(numpy.nansum(raw[1]["n_chased"], axis=1) * widths[row]))
    res = {"root": ROOT, "rows": n_rows, "n": len(t), "k": K, "best_s": best, "every_s": every, "candidates": int(len(curve)),
           "max_epochs": int(max_epochs), "widths": [int(widths.min()), int(widths.max())],
           "chase_reach": [int(chase_reach.min()), int(chase_reach.max())],
           "added_by_peak_fits_s": best["power_batch_peaks8_statistics_peak_fits"] - best["power_batch_peaks8_statistics"],
           "added_by_event_vetting_s": added, "results_equal_without_the_stage": bool(same),
           "rows_and_shapes_s": rows_s, "context_event_vetting_s": device_s, "assembly_s": added - rows_s - device_s,
           "survey_event_vetting_alone_s": alone_s, "window_steps": window_steps, "chase_taps": chase_taps,
           "held_events": int(numpy.nansum(raw[0]["n_held"])), "good_events": int(numpy.nansum(raw[0]["n_good"])),
           "candidates_all_good": int((raw[0]["n_good"] == raw[0]["n_held"]).sum()),
           "record_bytes": int(raw[0].nbytes + raw[1].nbytes)}
    res["event_vetting_over_peak_fits"] = res["added_by_event_vetting_s"] / res["added_by_peak_fits_s"]
    if kernels:
        res["kernel_ns"] = {k: v for k, v in sorted(kernels.items()) if any(name in k for name in KERNELS)}
        for name in KERNELS:
            found = [v for k, v in kernels.items() if name in k]
            if found:   # (the child runs the call twice)
                res[name + "_launches_per_call"] = sum(v[0] for v in found) / 2
                res[name + "_us_per_call"] = sum(v[1] for v in found) / 2e3
        if KERNELS[0] + "_us_per_call" in res:
            us = res[KERNELS[0] + "_us_per_call"]
            res["kernel_us_per_slab"] = us / res[KERNELS[0] + "_launches_per_call"]
            res["kernel_us_per_candidate"] = us / max(1, len(curve))
            res["kernel_taps_per_s"] = (window_steps + chase_taps) / (us * 1e-6)
        if KERNELS[1] + "_us_per_call" in res:
            res["transit_times_window_steps_per_s"] = window_steps / (res[KERNELS[1] + "_us_per_call"] * 1e-6)
        found = [v for k, v in (bare or {}).items() if KERNELS[0] in k]
        if found and KERNELS[0] + "_us_per_call" in res:
            res["kernel_without_chase_us_per_call"] = sum(v[1] for v in found) / 2e3
            res["chase_pass_us_per_call"] = res[KERNELS[0] + "_us_per_call"] - res["kernel_without_chase_us_per_call"]
            if res["chase_pass_us_per_call"] > 0:
                res["chase_taps_per_s"] = chase_taps / (res["chase_pass_us_per_call"] * 1e-6)
    ctx.close()
    # the statement on HOST_PROCESSES fresh processes, on a sample of the candidates, scaled to all of them
    if host_sample > 0 and len(curve):
        import concurrent.futures
        import multiprocessing
        take = numpy.linspace(0, len(curve) - 1, min(host_sample, len(curve))).astype(int)
        parts = numpy.array_split(take, HOST_PROCESSES)
        jobs = [(inp["t"], y_rows, dy_rows, curve[i], period[i], T0[i], row[i], reach[i], chase_reach[i], guard[i], chase_span[i],
                 shapes, span_max, max_epochs) for i in parts if len(i)]
        with concurrent.futures.ProcessPoolExecutor(HOST_PROCESSES, mp_context=multiprocessing.get_context("spawn")) as pool:
            list(pool.map(host_part, [j[:3] + tuple(a[:1] for a in j[3:11]) + j[11:] for j in jobs]))   # (warm: interpreters, imports)
            t0 = time.perf_counter()
            n_good = numpy.concatenate(list(pool.map(host_part, jobs)))
            host_s = time.perf_counter() - t0
        res["host_statement_sample"] = int(len(take))
        res["host_statement_sample_s"] = host_s
        res["host_statement_all_s"] = host_s * len(curve) / len(take)
        res["host_statement_agrees"] = bool(numpy.array_equal(n_good, raw[0]["n_good"][take], equal_nan=True))
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
