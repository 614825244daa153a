#!/usr/bin/env python
"""Writes tests/golden/peak_stages_host.npz: what power_batch's host chain returns on the stand-in context of
tests/peak_stages_fake.py, with tls_amd imported from the checkout given as the first argument.

    git worktree add /tmp/parent <commit>
    python tools/gen_peak_stages_golden.py /tmp/parent [out.npz]

The file pins tests/test_peak_stages_host.py to that checkout: it was made from the commit before survey.py got its peak-stage
table.  It needs no device and no built library.
"""
import os
import sys

import numpy

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    checkout = os.path.abspath(argv[1])
    out = argv[2] if len(argv) > 2 else os.path.join(HERE, "..", "tests", "golden", "peak_stages_host.npz")
    sys.path[:0] = [checkout, os.path.join(HERE, "..", "tests")]
    import peak_stages_fake
    from tls_amd import survey
    assert os.path.abspath(survey.__file__).startswith(checkout + os.sep), survey.__file__
    numpy.savez_compressed(out, **peak_stages_fake.golden(survey))
    print("%s: %d bytes from %s" % (out, os.path.getsize(out), checkout))


if __name__ == "__main__":
    main(sys.argv)
