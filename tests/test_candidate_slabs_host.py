"""How the per-candidate survey stages cut their candidates into slabs (tls_amd/csrc/tls_candidate_slabs.h through
tls_debug_candidate_slabs, no GPU): against a restatement of the rule, at its edges, and by its invariants."""
import numpy
import pytest

from tls_amd import _lib


def rule(curve, n_fits, max_curves, max_fits):
    """Slots in order of first appearance; a candidate whose curve is new when every slot is taken, or that is one more than
    max_fits, opens the next slab; a slab copies its curves in runs, and a run grows only by the curve after its last one."""
    slab, slot, runs, f = [], [], [], 0
    while f < n_fits:
        slots, follows, count = {}, None, 0
        runs.append(0)
        while f < n_fits and count < max_fits:
            c = f if curve is None else int(curve[f])
            if c not in slots:
                if len(slots) == max_curves:
                    break
                slots[c] = len(slots)
                runs[-1] += c != follows
                follows = c + 1
            slab.append(len(runs) - 1)
            slot.append(slots[c])
            f, count = f + 1, count + 1
    return slab, slot, runs


def check(curve, n_fits, max_curves, max_fits):
    got = _lib.candidate_slabs(curve, n_fits, max_curves, max_fits)
    want = rule(curve, n_fits, max_curves, max_fits)
    for g, w, what in zip(got, want, ("slab", "slot", "runs")):
        assert g.dtype == numpy.int64 and g.tolist() == w, (what, curve, max_curves, max_fits)
    return [g.tolist() for g in got]


def test_no_candidates():
    assert check(None, 0, 3, 3) == [[], [], []]
    assert check([], 0, 1, 1) == [[], [], []]


def test_candidate_f_reads_curve_f():
    slab, slot, runs = check(None, 5, 2, 4)
    assert slab == [0, 0, 1, 1, 2] and slot == [0, 1, 0, 1, 0] and runs == [1, 1, 1]


def test_cut_by_the_candidate_limit():
    """Exactly max_fits candidates are one slab; one more opens a second."""
    assert check([0, 1, 0, 1], 4, 8, 4) == [[0, 0, 0, 0], [0, 1, 0, 1], [1]]
    assert check([0, 1, 0, 1, 0], 5, 8, 4) == [[0, 0, 0, 0, 1], [0, 1, 0, 1, 0], [1, 1]]


def test_cut_by_the_curve_slots():
    """The third distinct curve finds both slots taken while max_fits is not reached: it opens the next slab in slot 0."""
    slab, slot, runs = check([5, 9, 5, 2, 9, 2], 6, 2, 100)
    assert slab == [0, 0, 0, 1, 1, 1] and slot == [0, 1, 0, 0, 1, 0] and runs == [2, 2]


def test_repeated_curves_take_no_new_slot():
    assert check([4, 4, 4, 4], 4, 1, 100) == [[0, 0, 0, 0], [0, 0, 0, 0], [1]]


def test_runs():
    assert check([3, 4, 5, 6], 4, 8, 8)[2] == [1]                       # ascending, consecutive: one copy
    assert check([6, 5, 4, 3], 4, 8, 8)[2] == [4]                       # descending: one each
    slab, slot, runs = check([3, 4, 4, 5, 3, 7], 6, 8, 8)               # {3, 4, 5} and {7}
    assert slab == [0] * 6 and slot == [0, 1, 1, 2, 0, 3] and runs == [2]


def test_random_candidates_and_the_invariants():
    rng = numpy.random.RandomState(5)
    n_fits, max_curves, max_fits = 2000, 7, 16
    # stretches of 50 candidates on 1 to 12 neighbouring curves: some are cut by the candidate limit, some by the slots
    stretch = numpy.arange(n_fits) // 50
    curve = (rng.randint(0, 40, 40)[stretch] + rng.randint(0, 1 << 30, n_fits) % rng.randint(1, 13, 40)[stretch]) % 40
    slab, slot, runs = (numpy.array(a) for a in check(curve, n_fits, max_curves, max_fits))
    # slabs are contiguous, in order and non-empty
    assert slab[0] == 0 and set(numpy.diff(slab).tolist()) <= {0, 1} and slab[-1] == len(runs) - 1
    assert (slot >= 0).all() and (slot < max_curves).all()
    for s in range(len(runs)):
        f = numpy.flatnonzero(slab == s)
        assert 1 <= len(f) <= max_fits
        first = {}
        for c, k in zip(curve[f].tolist(), slot[f].tolist()):
            assert first.setdefault(c, k) == k                          # one slot a curve
        assert sorted(first.values()) == list(range(len(first)))        # ... and one curve a slot
        assert list(first.values()) == list(range(len(first)))          # numbered by first appearance
        assert 1 <= runs[s] <= len(first)
        if f[-1] + 1 < n_fits:                                          # every cut is forced
            assert len(f) == max_fits or (len(first) == max_curves and int(curve[f[-1] + 1]) not in first)
    assert (numpy.bincount(slab) < max_fits).any() and (numpy.bincount(slab) == max_fits).any()   # both kinds of cut occur


def test_argument_errors():
    for args in ((None, -1, 1, 1), (None, 3, 0, 1), (None, 3, 1, 0)):
        with pytest.raises(RuntimeError, match="tls_debug_candidate_slabs"):
            _lib.candidate_slabs(*args)
