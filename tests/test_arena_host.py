"""Device-memory bookkeeping without a GPU (tls_amd/csrc/tls_arena.h): the arena that cuts one allocation into typed
regions and the pool that owns every buffer, in a stand-alone host program built with the address and undefined-behaviour
sanitizers (tests/host/arena_sweep.cpp), malloc and free standing in for the device allocator."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_and_pool_under_sanitizers(tmp_path):
    """Element mixes taken from the survey stages (16-byte pairs, doubles, blocks of 1, 3 and 5 int columns, 16-byte and
    24-byte records, bytes, 64-bit counts, optional regions of count 0) at counts from 0 to 4097 over three backing element
    types: every region at its type's alignment, disjoint and in declaration order, the last one inside the bound capacity,
    the total the sum of the padded regions, a count of 0 a null pointer; every element written, AddressSanitizer the judge.
    The arenas of tls_transit_times, tls_folded_views and reserve_peak_fits come out at their closed-form sizes, odd slab
    lengths included.  The pool: registration order, grow-only reserve, byte count, the walk by kind, a failed allocation,
    release and scope exit, LeakSanitizer over what is left.  Host code only: no device, nothing preloaded."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the arena sweep is part of the suite")
    exe = str(tmp_path / "arena_sweep")
    build = subprocess.run([hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "host", "arena_sweep.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "arenas checked" in run.stdout and "pool clean" in run.stdout
