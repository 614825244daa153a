"""Developer tool: what the event-period stage of survey mode costs (the method of tools/transit_times_time.py: best of three
runs of each call in one process).

The workload: 1024 k2_90d rows (90 d at 30 min cadence), three transits of 9 samples injected into each at days 12, 47 and 82,
the three pairs of them a curve on the default width grid, period_min = 0.25 d and max_aliases = 512: 3072 pairs of 140 to 280
aliases each.  In one run:
  * the kernels' time from a rocprofv3 --kernel-trace --stats run of this tool's --kernel mode (a child process of its own,
    started before this process opens the GPU; no counters in that run), a call, a pair and an (alias, epoch) look;
  * survey.event_periods and Context.event_periods (upload, kernels, copy back) on the whole batch;
  * the statement's vectorised numpy form (tests/event_periods_spec.py) on 16 host processes that never open the GPU, on a
    sample of the pairs, scaled to all of them;
  * the only other device route: the same aliases expanded into survey.transit_times candidates (period dT / k, T0 = t[index_a],
    the row's duration), on a sample of the pairs, scaled to all of them.

Usage: python tools/event_periods_time.py [n_rows=1024] [--json OUT] [--no-profile] [--host-sample 64] [--times-sample 8]"""
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
KERNELS = ("tls_event_aliases_kernel", "tls_alias_plane_kernel", "tls_times_pairs_kernel")
HOST_PROCESSES = 16
PERIOD_MIN, MAX_ALIASES, WIDTH, DEPTH = 0.25, 512, 9, 1.5e-3
EVENT_DAYS = (12.0, 47.0, 82.0)


def workload(rows):
    """(t, flux, pairs, power_kwargs): `rows` copies of the seed-0 k2_90d light curve, each with noise of its own and three
    transits of WIDTH samples, and the three pairs of them a curve on the rows of survey.single_transit_widths(t)."""
    from tls_amd import survey, synthetic
    from tls_amd.planning import search_inputs
    from tls_amd.template import reference_transit
    t, f0, kw = synthetic.config("k2_90d", seed=0)
    rng = numpy.random.default_rng(len(t))
    f = numpy.tile(f0, (rows, 1))
    f *= 1.0 + 2e-4 * rng.standard_normal(f.shape)
    shape = search_inputs(t, f[0], None, oversampling_factor=1, **kw)["shape"]
    b = 1.0 - numpy.asarray(reference_transit(WIDTH, **shape))
    centres = [int(numpy.argmin(numpy.abs(t - t[0] - day))) for day in EVENT_DAYS]
    for c in centres:
        f[:, c - (WIDTH - 1) // 2: c - (WIDTH - 1) // 2 + WIDTH] -= DEPTH * b
    widths = survey.single_transit_widths(t)
    row = int(numpy.searchsorted(widths, WIDTH))
    assert widths[row] == WIDTH
    a, b_, c = centres
    curve = numpy.repeat(numpy.arange(rows), 3)
    pairs = (curve, numpy.tile([a, b_, a], rows), numpy.tile([b_, c, c], rows), numpy.full(3 * rows, row))
    return t, f, pairs, kw


def kernel_ns(n_rows):
    """{kernel name: (calls, total ns)} of a rocprofv3 --kernel-trace --stats run of `--kernel aliases`, or None."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    work = tempfile.mkdtemp(prefix="event_periods_time_")
    try:
        subprocess.run([rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable,
                        os.path.abspath(__file__), str(n_rows), "--kernel", "aliases"], check=True, stdout=subprocess.DEVNULL,
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
    """The statement's vectorised form on a share of the pairs (a process that never opens the GPU)."""
    import event_periods_spec as spec
    t, y_rows, dy_rows, curve, ia, ib, row, reach, offset, shapes, span_max = job
    return spec.expected(t, y_rows, dy_rows, curve, ia, ib, row, reach, offset, shapes, span_max, PERIOD_MIN, MAX_ALIASES)[0]


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
    kernel_mode = option("--kernel")                  # "aliases": the profiled child
    host_sample = int(option("--host-sample") or 64)
    times_sample = int(option("--times-sample") or 8)
    profile = "--no-profile" not in args and not kernel_mode
    rest = [a for a in args if not a.startswith("--")]
    n_rows = int(rest[0]) if rest else 1024
    from tls_amd import _lib, survey
    from tls_amd.template import reference_transit
    t, flux, pairs, kw = workload(n_rows)
    call = dict(pairs=pairs, period_min=PERIOD_MIN, max_aliases=MAX_ALIASES)
    if kernel_mode:   # (the profiled child: one call, once warm and once more)
        ctx = _lib.Context(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                survey.event_periods(t, flux, context=ctx, **call, **kw)
        ctx.close()
        return
    kernels = kernel_ns(n_rows) if profile else None
    ctx = _lib.Context(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        survey.event_periods(t, flux, context=ctx, **call, **kw)       # (warm: device buffers, code objects)
        survey_s, (records, aliases) = best_of(lambda: survey.event_periods(t, flux, context=ctx, **call, **kw))
        bare_s, _ = best_of(lambda: survey.event_periods(t, flux, context=ctx, with_aliases=False, **call, **kw))
        inp, y_rows, dy_rows = survey._batch_inputs(t, flux, None, dict(kw, oversampling_factor=1))
        widths = survey.single_transit_widths(inp["t"])
        dt = float(numpy.median(numpy.diff(inp["t"])))
        shapes = [1.0 - numpy.asarray(reference_transit(int(L), **inp["shape"])) for L in widths]
        span_max = [(int(L) - 1) * dt * 1.5 for L in widths]
        curve, ia, ib, row = pairs
        reach, offset = records["reach"], records["offset"]
        device_s, raw = best_of(lambda: ctx.event_periods(inp["t"], y_rows, dy_rows, curve, ia, ib, row, reach, offset, widths,
                                                          shapes, span_max, PERIOD_MIN, MAX_ALIASES))
        same = all(numpy.array_equal(raw[0][f], records[f], equal_nan=True) for f in raw[0].dtype.names)
        looks = float(numpy.nansum(raw[1]["n_epochs"]))
        n_pairs = len(curve)
        res = {"root": ROOT, "rows": n_rows, "n": len(t), "pairs": n_pairs, "period_min": PERIOD_MIN, "max_aliases": MAX_ALIASES,
               "aliases": float(records["n_evaluated"].sum()), "aliases_per_pair": [float(records["n_evaluated"].min()),
                                                                                     float(records["n_evaluated"].max())],
               "alias_epoch_looks": looks, "status_0": int((records["status"] == 0).sum()),
               "allowed": float(records["n_allowed"].sum()), "survey_event_periods_s": survey_s,
               "survey_event_periods_without_aliases_s": bare_s, "context_event_periods_s": device_s,
               "context_equals_survey": bool(same), "record_bytes": int(raw[0].nbytes + raw[1].nbytes)}
        # the other device route, on a sample of the pairs: every alias a candidate of survey.transit_times
        take = numpy.linspace(0, n_pairs - 1, min(times_sample, n_pairs)).astype(int)
        k = [numpy.arange(1, int(records["n_evaluated"][f]) + 1) for f in take]
        period = numpy.concatenate([records["dT"][f] / kk for f, kk in zip(take, k)])
        T0 = numpy.concatenate([numpy.full(len(kk), inp["t"][ia[f]]) for f, kk in zip(take, k)])
        cand_curve = numpy.concatenate([numpy.full(len(kk), curve[f]) for f, kk in zip(take, k)])
        duration = numpy.full(len(period), WIDTH * dt)
        survey.transit_times(t, flux, period[:8], T0[:8], duration[:8], curve=cand_curve[:8], context=ctx, **kw)   # (warm)
        times_s, _ = best_of(lambda: survey.transit_times(t, flux, period, T0, duration, curve=cand_curve, context=ctx, **kw))
        res.update(transit_times_sample_pairs=int(len(take)), transit_times_sample_candidates=int(len(period)),
                   transit_times_sample_s=times_s, transit_times_all_s=times_s * n_pairs / len(take))
        res["transit_times_over_event_periods"] = res["transit_times_all_s"] / survey_s
    if kernels:
        res["kernel_ns"] = {k: v for k, v in sorted(kernels.items())}
        total = 0.0
        for name in KERNELS:
            found = [v for k, v in kernels.items() if name in k]
            if found:   # (the child runs the call twice)
                res[name + "_launches_per_call"] = sum(v[0] for v in found) / 2
                res[name + "_us_per_call"] = sum(v[1] for v in found) / 2e3
                total += res[name + "_us_per_call"]
        res["kernels_us_per_call"] = total
        if KERNELS[0] + "_us_per_call" in res:
            us = res[KERNELS[0] + "_us_per_call"]
            res["alias_kernel_us_per_pair"] = us / n_pairs
            res["alias_kernel_ns_per_look"] = us * 1e3 / max(looks, 1.0)
    ctx.close()
    # the statement on HOST_PROCESSES fresh processes, on a sample of the pairs, scaled to all of them
    if host_sample > 0:
        import concurrent.futures
        import multiprocessing
        take = numpy.linspace(0, n_pairs - 1, min(host_sample, n_pairs)).astype(int)
        parts = [i for i in numpy.array_split(take, HOST_PROCESSES) if len(i)]
        jobs = [(inp["t"], y_rows, dy_rows, curve[i], ia[i], ib[i], row[i], reach[i], offset[i], shapes, span_max) for i in parts]
        with concurrent.futures.ProcessPoolExecutor(HOST_PROCESSES, mp_context=multiprocessing.get_context("spawn")) as pool:
            list(pool.map(host_part, [j[:3] + tuple(a[:1] for a in j[3:9]) + j[9:] for j in jobs]))   # (warm: interpreters, imports)
            t0 = time.perf_counter()
            found = numpy.concatenate(list(pool.map(host_part, jobs)))
            host_s = time.perf_counter() - t0
        res["host_statement_sample"] = int(len(take))
        res["host_statement_sample_s"] = host_s
        res["host_statement_all_s"] = host_s * n_pairs / len(take)
        res["host_statement_over_event_periods"] = res["host_statement_all_s"] / survey_s
        res["host_statement_agrees"] = bool(all(numpy.array_equal(found[f], raw[0][f][take], equal_nan=True)
                                                for f in found.dtype.names))
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
