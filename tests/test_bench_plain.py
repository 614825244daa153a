"""bench.py: a plain run does only what the headline needs -- it launches nothing after the timed steps -- and --full adds
the counted pass and the roofline.  A recording stand-in for the context; no GPU."""
import json
import sys

import numpy

import bench
from tls_amd import _lib


class RecordingContext(object):
    name = "stand-in"

    def __init__(self, device=0):
        self.n, self.calls = 0, []
        RecordingContext.last = self

    def prepare(self, t, y, dy, periods, table, params):
        self.n = len(periods)
        self.calls.append("prepare")

    def execute(self, count_work=False):
        self.calls.append("execute_counted" if count_work else "execute")

    def execute_timed(self, reps=1):
        self.calls.append("execute_timed")
        return 1.0

    def synchronize(self):
        pass

    def kernel_timing(self, reset=True):
        self.calls.append("kernel_timing")
        return 2.0, 2

    def fetch(self, with_counters=False):
        out = (numpy.arange(self.n, 0, -1, dtype=numpy.float64), numpy.arange(self.n, dtype=numpy.int64) % 7,
               numpy.full(self.n, 0.999))
        counters = {"grid_cells": 10 * self.n, "evaluated_cells": 3 * self.n, "inner_steps": 7 * self.n, "issued_fma": 9 * self.n}
        return out + (counters,) if with_counters else out

    def plan_info(self):
        return {"grid_cells": 10 * self.n, "lds_bytes": 1, "n_blocks": 2, "resident": True}

    def last_kernel(self):
        return "slim"

    def close(self):
        pass


def run_bench(monkeypatch, capsys, *argv):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(_lib, "Context", RecordingContext)
    monkeypatch.setattr(_lib, "device_count", lambda: 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"] + list(argv))
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    calls = RecordingContext.last.calls
    after = calls[len(calls) - calls[::-1].index("kernel_timing"):]   # what follows the read-out of the timed steps
    return line, calls, after


def test_a_plain_run_launches_nothing_after_the_timed_steps(monkeypatch, capsys, tmp_path):
    line, calls, after = run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path))
    assert calls.count("execute") == 2 + 3 and "execute_counted" not in calls   # warm-up and timed steps only
    assert after == []
    n = RecordingContext.last.n
    assert line["metric"] == "trial cells/sec (period x duration x T0)" and line["unit"] == "trial cells/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    numpy.testing.assert_allclose(line["value"] * line["ms_per_step"], 1e3 * 10 * n, rtol=1e-12)   # the same K steps
    assert "roofline" not in line and "cpu_baseline" not in line and "value_one_shot" not in line
    numpy.testing.assert_array_equal(numpy.load(str(tmp_path / "chi2.npy")), numpy.arange(n, 0, -1))


def test_full_adds_the_counted_pass_and_the_roofline(monkeypatch, capsys):
    line, calls, after = run_bench(monkeypatch, capsys, "--full", "--no-extras", "--no-cpu-baseline")
    assert after == ["prepare", "execute_counted"]
    n = RecordingContext.last.n
    assert line["config"]["inner_steps"] == 7 * n and line["config"]["evaluated_cells"] == 3 * n
    assert line["roofline"]["bound"] == "fp64" and line["roofline"]["kernel_ms"] == 1.0
    assert line["argmin_period_index"] == n - 1 and "cpu_baseline" not in line
