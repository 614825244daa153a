"""Picks (period, T0, fractional duration) whose odd or even in-transit COUNT is one where the two forms of k ** 0.5 that
power() takes of a count differ, chosen on the host before any device call.

stats._mean_and_err, like the reference, divides the odd and the even depth error by numpy.sum(len(x)) ** 0.5, the power of a
numpy integer scalar; snr and the pink noise take float(k) ** 0.5.  The two differ by one ulp at the counts D (about one k in
twenty under numpy 2 on an AVX-512 host: 19, 51, 63, 75, 76, 78, 107, ...; the set belongs to the numpy build and the CPU it
dispatches for, and may be empty).  A device that read one table for both would be wrong at exactly these counts, and only
there, so the tests that use this module steer their picks onto them: D is formed at run time with the running numpy and
joined with FIXED, and a lattice of picks over the time stamps of TIME is walked for the first pick whose odd count, and the
first whose even count, is a given member.  Counts depend on the time stamps and the pick alone, not on the flux.
"""
import numpy

from tls_amd.stats import (_intransit_fluxes, all_transit_times, calculate_fill_factor, calculate_transit_duration_in_days)

FIXED = (19, 51, 63, 75, 76, 78, 107)     # the first counts of D under numpy 2.2.6 with AVX-512


def dense_gapped_time():
    """30 d at 30 min with a gap of 4.5 d (tests/test_power_batch_statistics.py gapped_time() twice as dense): 1224 stamps."""
    t = numpy.linspace(3.0, 33.0, 1440)
    return t[(t < 14.0) | (t > 18.5)]


TIME = dense_gapped_time()
PERIODS = numpy.arange(1.5, 9.0, 0.07)           # 108
DURATIONS = numpy.arange(0.004, 0.2, 0.004)      # 49 fractional durations


def disagreeing_counts(n):
    """D: the counts k <= n at which the running numpy's numpy.sum(k) ** 0.5 is not float(k) ** 0.5."""
    return [k for k in range(1, n + 1) if float(numpy.sum(k) ** 0.5) != float(k) ** 0.5]


def lattice():
    """(period, T0, index into DURATIONS) of all 5292 picks, periods outermost."""
    return [(float(p), 3.0 + 0.37 * float(p), j) for p in PERIODS for j in range(len(DURATIONS))]


def counts(t, period, T0, duration):
    """(odd count, even count, per-transit counts) of a pick, as power() forms them (even = epochs 0, 2, 4, ...)."""
    transit_times = all_transit_times(T0, t, period)
    d = calculate_transit_duration_in_days(t, period, transit_times, duration, fill_factor=calculate_fill_factor(t))
    sizes = numpy.array([len(c) for c in _intransit_fluxes(t, t, transit_times, d)])
    return int(sizes[1::2].sum()), int(sizes[0::2].sum()), sizes


def lattice_counts(t=TIME):
    """[5292, 2]: odd and even count of every lattice pick (1 s on the host)."""
    return numpy.array([counts(t, p, T0, DURATIONS[j])[:2] for p, T0, j in lattice()])


def covering(targets, table):
    """The first lattice pick whose odd count is m and the first whose even count is m, for every m of `targets`: (indices
    into lattice() in lattice order, members reached as odd counts, members reached as even counts)."""
    keep, reached = set(), (set(), set())
    for side in (0, 1):
        for m in targets:
            hit = numpy.flatnonzero(table[:, side] == m)
            if len(hit):
                keep.add(int(hit[0]))
                reached[side].add(int(m))
    return sorted(keep), reached[0], reached[1]


def duration_tables(n_rows):
    """The lattice's durations as row_duration tables of n_rows entries (a plan has fewer template rows than the lattice has
    durations): table i holds DURATIONS[i * n_rows :], padded with its last; (tables, table of duration j, row of j)."""
    tables = []
    for lo in range(0, len(DURATIONS), n_rows):
        part = DURATIONS[lo:lo + n_rows]
        tables.append(numpy.concatenate([part, numpy.full(n_rows - len(part), part[-1])]))
    j = numpy.arange(len(DURATIONS))
    return tables, j // n_rows, j % n_rows
