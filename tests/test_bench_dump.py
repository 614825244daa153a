"""bench.py --dump-outputs: the writer of the timed path's outputs (float64 .npy files, at most 64 MB in all).  No GPU."""
import os

import numpy

import bench


def test_outputs_are_written_whole_in_float64(tmp_path):
    chi2 = numpy.linspace(1.0, 2.0, 1000)
    row = numpy.arange(1000, dtype=numpy.int64) % 17
    depth = numpy.full(1000, 0.999)
    names = bench.dump_outputs(str(tmp_path / "out"), {"chi2": chi2, "row": row, "depth": depth})
    assert names == ["chi2", "depth", "row"]
    for k, want in (("chi2", chi2), ("row", row), ("depth", depth)):
        got = numpy.load(str(tmp_path / "out" / (k + ".npy")))
        assert got.dtype == numpy.float64
        numpy.testing.assert_array_equal(got, want)
    assert not os.path.exists(str(tmp_path / "out" / "index.npy"))


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 4 * 100)
    n = 1000
    outputs = {"chi2": numpy.arange(n, dtype=numpy.float64), "row": numpy.arange(n, dtype=numpy.int64)}
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    for d in dirs:
        assert bench.dump_outputs(d, outputs) == ["chi2", "index", "row"]
    total = sum(os.path.getsize(os.path.join(dirs[0], f)) - 128 for f in os.listdir(dirs[0]))   # (128 B .npy header)
    assert total <= bench.DUMP_LIMIT_BYTES
    index = numpy.load(os.path.join(dirs[0], "index.npy"))
    assert len(index) == bench.DUMP_LIMIT_BYTES // 24 and numpy.all(numpy.diff(index) > 0)   # 3 arrays of 8 B per entry
    for k in ("chi2", "row"):
        numpy.testing.assert_array_equal(numpy.load(os.path.join(dirs[0], k + ".npy")), index)
    for f in ("chi2.npy", "index.npy", "row.npy"):   # the same sample from run to run
        numpy.testing.assert_array_equal(numpy.load(os.path.join(dirs[0], f)), numpy.load(os.path.join(dirs[1], f)))


def test_host_gathered_results_are_every_rank_in_rank_order():
    """The host-channel fallback of the survey layout (N > 1, no RCCL): what each rank fetched, rank after rank."""
    def triple(n, base):
        return (numpy.arange(n) + base + 0.5, numpy.arange(n, dtype=numpy.int64) + int(base), numpy.full(n, base / 10.0))

    ranks = [triple(5, 0.0), triple(5, 100.0), triple(3, 200.0)]

    class Context(object):
        def fetch(self):
            return ranks[0]

    class Channel(object):
        def allgather_bytes(self, mine):
            assert mine == b"".join(a.tobytes() for a in ranks[0])
            return [b"".join(a.tobytes() for a in t) for t in ranks]

    class Harness(object):
        channel = Channel()

    got = bench._host_gathered_results(Harness(), Context())
    for g, want, dtype in zip(got, zip(*ranks), (numpy.float64, numpy.int64, numpy.float64)):
        assert g.dtype == dtype
        numpy.testing.assert_array_equal(g, numpy.concatenate(want))
