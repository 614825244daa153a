#!/usr/bin/env python3
"""Records tests/golden/slim_tap_broadcast_parent.npz: (chi2, row, depth) and the work counters of every case of
tests/test_slim_tap_broadcast.py as the library in use computes them.  Run it on the GPU with the PARENT commit's library
(make -C tls_amd/csrc variant NAME=parent on the parent's sources; TLS_AMD_DEBUG=1 TLS_AMD_LIB=.../libtls_amd_parent.so):

    python tools/record_slim_tap_broadcast.py [OUT.npz]
"""
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_slim_tap_broadcast as cases  # noqa: E402
from tls_amd import _lib  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
gpu = _lib.Context(0)
store = {}
for name in cases.CASES:
    got = cases.run_case(gpu, name)
    for value, part in zip(got, ("chi2", "row", "depth", "counters")):
        store["%s/%s" % (name, part)] = numpy.ascontiguousarray(value)
    print("%-24s %4d values, counters %s" % (name, got[0].size, dict(zip(cases.COUNTERS, got[3].tolist()))))
gpu.close()
numpy.savez_compressed(out, **store)
print("wrote %s: %d bytes, library %s" % (out, os.path.getsize(out), _lib.LIB_PATH))
