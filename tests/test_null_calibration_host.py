"""False-alarm calibration without a GPU: the tls_null_rows declarations against their bindings, a pure-Python Philox4x64-10
and the stream layout against numpy, fap_table / empirical_fap against the reference's stats.FAP on a synthetic null, the
lookup rule on hand-made nulls, sde_threshold against empirical_fap, and every argument error of null_sde, fap_table and
sde_threshold."""
import ctypes
import os
import re

import numpy
import pytest

from tls_amd import _lib, stats, survey
from conftest import REPO

MASK = (1 << 64) - 1
M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


# ---- numpy mirrors of tls_null.hip.h (imported by test_null_calibration.py)

def philox_block(counter, key):
    """Philox4x64-10 of a 4-word counter under a 2-word key (Random123's rounds, Python ints)."""
    c, k = list(counter), list(key)
    for r in range(10):
        if r:
            k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 64) ^ c[3] ^ k[1], p0 & MASK]
    return c


def trial_words(n, seed, R, block=None):
    """(words, W, trial R's W words from numpy.random.Philox) of the white-noise layout (block None) or the bootstrap's."""
    words = 2 * n if block is None else -(-n // block)
    W = 4 * (-(-words // 4))
    return words, W, numpy.random.Philox(key=seed, counter=R * W // 4).random_raw(W)


def white_z(w):
    """z of every point from a trial's words (w[2i], w[2i + 1]), numpy's restatement of the device's Box-Muller."""
    ua = (w[0::2] >> numpy.uint64(11)).astype(numpy.float64) * 2.0 ** -53
    ub = (w[1::2] >> numpy.uint64(11)).astype(numpy.float64) * 2.0 ** -53
    return numpy.sqrt(-2.0 * numpy.log(1.0 - ua)) * numpy.cos(6.283185307179586 * ub)


def white_rows(n, n_rows, seed, first_trial, sigma):
    sigma = numpy.broadcast_to(numpy.asarray(sigma, dtype=numpy.float64), (n_rows,))
    out = numpy.empty((n_rows, n))
    for r in range(n_rows):
        _, _, w = trial_words(n, seed, first_trial + r)
        out[r] = 1.0 + sigma[r] * white_z(w[:2 * n])
    return out


def bootstrap_rows(n, n_rows, seed, first_trial, source, L):
    """The bootstrap's rows with Python-int umulhi: block b of trial R copies source row R mod n_src from
    (w[b] (n - L + 1)) >> 64."""
    source = numpy.atleast_2d(numpy.asarray(source, dtype=numpy.float64))
    out = numpy.empty((n_rows, n))
    for r in range(n_rows):
        R = first_trial + r
        words, _, w = trial_words(n, seed, R, L)
        s = R % len(source)
        for b in range(words):
            start = (int(w[b]) * (n - L + 1)) >> 64
            lo, hi = b * L, min(n, (b + 1) * L)
            out[r, lo:hi] = source[s, start:start + hi - lo]
    return out


# ---- header and binding

def _header():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", ["tls_null_rows", "tls_debug_null_words"])
def test_declaration_matches_argtypes(name):
    m = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, "%s is not declared" % name
    c_types = {"tls_ctx *": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
               "const double *": _lib._c_double_p, "double *": _lib._c_double_p,
               "uint64_t *": ctypes.POINTER(ctypes.c_uint64)}
    want = []
    for p in m.group(1).split(","):
        p = " ".join(p.replace("*", " * ").split())
        ctype = p.rsplit(" ", 1)[0].replace(" *", " *")
        want.append(c_types[ctype])
    fn = getattr(_lib.load(), name)
    assert list(fn.argtypes) == want
    assert fn.restype == ctypes.c_int
    assert name in _lib.SYMBOLS


def test_abi_version_is_8():
    assert _lib.ABI_VERSION == 8 == _lib.load().tls_abi_version()


# ---- the random stream

def test_python_philox_is_numpy_philox():
    for seed in (0, 1, 12345, 2 ** 64 - 1):
        want = numpy.random.Philox(key=seed).random_raw(24)
        got = [philox_block(((j // 4 + 1) & MASK, (j // 4 + 1) >> 64, 0, 0), (seed, 0))[j % 4] for j in range(24)]
        assert [int(x) for x in want] == got, seed


def test_stream_layout():
    """Philox(key=s, counter=c) starts at word 4c of Philox(key=s)'s stream, so trial R's words are its own stretch."""
    for seed in (0, 7, 2 ** 64 - 1):
        stream = numpy.random.Philox(key=seed).random_raw(4 * 40)
        for n, block in ((5, None), (6, None), (10, 3), (9, 9)):
            for R in range(3):
                _, W, w = trial_words(n, seed, R, block)
                numpy.testing.assert_array_equal(w, stream[R * W:(R + 1) * W])
    # u = (w >> 11) 2^-53 is Generator.random()
    w = numpy.random.Philox(key=3).random_raw(1000)
    u = (w >> numpy.uint64(11)).astype(numpy.float64) * 2.0 ** -53
    numpy.testing.assert_array_equal(u, numpy.random.Generator(numpy.random.Philox(key=3)).random(1000))


def test_mirrors_depend_on_trial_only():
    src = 1.0 + 0.01 * numpy.random.RandomState(0).rand(2, 23)
    whole = bootstrap_rows(23, 9, 5, 100, src, 4)
    numpy.testing.assert_array_equal(whole[4:], bootstrap_rows(23, 5, 5, 104, src, 4))
    w = white_rows(11, 6, 5, 100, 0.01)
    numpy.testing.assert_array_equal(w[2:], white_rows(11, 4, 5, 102, 0.01))
    # every bootstrap block is a contiguous stretch of its source row
    row = bootstrap_rows(23, 1, 9, 3, src, 5)[0]
    for b in range(5):
        piece = row[5 * b: 5 * b + 5]
        assert any(numpy.array_equal(piece, src[1, s:s + len(piece)]) for s in range(23 - 5 + 1))


# ---- fap_table / empirical_fap against the reference's table

def _synthetic_null():
    """The reference table's 1251 finite thresholds plus 11244 values below its smallest one, shuffled: n = 12495."""
    _, thr = stats._fap_table()
    top = thr[:-1]
    assert len(top) == 1251 and top[0] == 5.651
    rng = numpy.random.RandomState(1)
    low = rng.uniform(0.0, 5.651, 11244)
    low = low[low < 5.651]
    assert len(low) == 11244
    x = numpy.concatenate([top, low])
    rng.shuffle(x)
    return x


def test_synthetic_null_reproduces_reference_table():
    ref_fap, ref_thr = stats._fap_table()
    table = survey.fap_table(_synthetic_null())
    fap, thr, n = table
    assert n == 12495 and len(fap) == len(thr) == 1252
    numpy.testing.assert_array_equal(thr, ref_thr)
    numpy.testing.assert_array_equal(numpy.round(fap, 9), ref_fap)
    top = ref_thr[:-1]
    probes = numpy.concatenate([top, (top[:-1] + top[1:]) / 2, [top[0] - 1e-9, 5.65, 3.0, 0.0, -1.0],
                                [9.1, numpy.nextafter(9.1, numpy.inf), 9.2, 50.0, numpy.inf, numpy.nextafter(5.651, 0)]])
    assert len(probes) >= 2506
    got = numpy.round(survey.empirical_fap(probes, table), 9)
    want = numpy.array([stats.FAP(x) for x in probes])
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want))
    ok = ~numpy.isnan(want)
    assert numpy.array_equal(got[ok].view(numpy.uint64), want[ok].view(numpy.uint64))
    assert numpy.isnan(survey.empirical_fap(numpy.inf, table))
    assert survey.empirical_fap(9.1, table) == 1.0 / 12495
    # the reference's lookup rule, literally, on the calibrated table
    numpy.testing.assert_array_equal(survey.empirical_fap(probes, table), [fap[numpy.argmax(thr > x)] for x in probes])


def test_reference_shaped_thresholds():
    table = survey.fap_table(_synthetic_null())
    # (fap[1] = 1250 / 12495 is just above 0.1: the threshold for 0.1 is the second kept value)
    assert survey.sde_threshold(table, 0.1) == 5.652
    assert survey.sde_threshold(table, table[0][1]) == 5.651
    assert (survey.sde_threshold(table, 0.01), survey.sde_threshold(table, 0.001)) == (6.98, 8.319)
    # (at the top two thresholds share the floor 1/n: the second largest null SDE already meets it)
    assert survey.sde_threshold(table, 1.0 / 12495) == table[1][-3]
    for target in (0.01, 0.001):
        x = survey.sde_threshold(table, target)
        assert stats.FAP(x) <= target < stats.FAP(numpy.nextafter(x, -numpy.inf))


# ---- the rule on hand-made nulls

def _brute(table, x):
    fap, thr, _ = table
    return fap[numpy.argmax(thr > x)]


def test_ties_floor_and_nan_region():
    table = survey.fap_table([1.0, 2.0, 3.0, 2.0, 2.0], max_fap=0.5)
    fap, thr, n = table
    assert n == 5
    numpy.testing.assert_array_equal(thr, [2.0, 2.0, 2.0, 3.0, numpy.inf])
    numpy.testing.assert_array_equal(fap[1:], [3 / 5, 2 / 5, 1 / 5, 1 / 5])
    assert numpy.isnan(fap[0])
    probes = numpy.array([-1.0, 1.0, 1.999, 2.0, 2.5, 2.999, 3.0, 3.5, 1e300, numpy.inf, numpy.nan])
    got = survey.empirical_fap(probes, table)
    numpy.testing.assert_array_equal(got, [numpy.nan, numpy.nan, numpy.nan, 1 / 5, 1 / 5, 1 / 5, 1 / 5, 1 / 5, 1 / 5,
                                           numpy.nan, numpy.nan])
    # (scalars in, scalars out; shapes kept)
    assert numpy.ndim(survey.empirical_fap(2.5, table)) == 0
    assert survey.empirical_fap(numpy.full((2, 3), 2.5), table).shape == (2, 3)


def test_m_capped_at_n():
    table = survey.fap_table([4.0, 1.0, 2.5], max_fap=1.0)
    fap, thr, n = table
    numpy.testing.assert_array_equal(thr, [1.0, 2.5, 4.0, numpy.inf])
    numpy.testing.assert_array_equal(fap[1:], [2 / 3, 1 / 3, 1 / 3])
    assert survey.fap_table([4.0], max_fap=0.01)[1].tolist() == [4.0, numpy.inf]
    assert survey.fap_table(numpy.arange(100.0), max_fap=0.05)[1].tolist() == list(numpy.arange(94.0, 100.0)) + [numpy.inf]


@pytest.mark.parametrize("null,max_fap", [([1.0, 2.0, 3.0, 2.0, 2.0], 0.5), ([4.0, 1.0, 2.5], 1.0),
                                          (list(numpy.random.RandomState(2).gamma(9.0, 0.7, 997)), 0.1),
                                          (list(numpy.round(numpy.random.RandomState(3).gamma(9.0, 0.7, 400), 1)), 0.2),
                                          ([0.0] * 50 + [6.0, 7.0], 0.1)])
def test_lookup_rule_and_threshold_consistency(null, max_fap):
    table = survey.fap_table(null, max_fap)
    fap, thr, n = table
    fin = thr[:-1]
    probes = numpy.concatenate([fin, (fin[:-1] + fin[1:]) / 2, numpy.nextafter(fin, -numpy.inf),
                                numpy.nextafter(fin, numpy.inf), [fin[0] - 1.0, fin[-1] + 1.0, numpy.inf]])
    got = survey.empirical_fap(probes, table)
    want = numpy.array([_brute(table, x) for x in probes])
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want))
    numpy.testing.assert_array_equal(got, want)
    targets = numpy.unique(numpy.concatenate([fap[1:], (fap[1:-1] + fap[2:]) / 2, [1.0 / n]]))
    targets = targets[(targets >= 1.0 / n) & (targets <= fap[1])]
    for target in targets:
        x = survey.sde_threshold(table, target)
        assert survey.empirical_fap(x, table) <= target
        below = survey.empirical_fap(numpy.nextafter(x, -numpy.inf), table)
        assert numpy.isnan(below) or below > target, (target, x, below)


# ---- argument errors (all raised before any device work: no GPU needed)

def _t(n=60):
    return numpy.linspace(0.0, 10.0, n)


@pytest.mark.parametrize("kwargs,match", [
    (dict(sigma=0.0), "sigma"), (dict(sigma=-0.01), "sigma"), (dict(sigma=0.2), "sigma"), (dict(sigma=numpy.nan), "sigma"),
    (dict(sigma=numpy.inf), "sigma"), (dict(sigma=[0.01, 0.02]), "sigma"), (dict(sigma=[[0.01] * 4]), "sigma"),
    (dict(sigma=[0.01, 0.01, 0.0, 0.01]), "sigma"), (dict(), "needs sigma"), (dict(sigma=0.01, block=3), "block"),
    (dict(source=numpy.ones(60)), "block"), (dict(source=numpy.ones(60), block=0), "block"),
    (dict(source=numpy.ones(60), block=61), "block"), (dict(source=numpy.ones(60), block=2.5), "block"),
    (dict(source=numpy.ones(60), block=3, sigma=0.01), "sigma"), (dict(source=numpy.ones(59), block=3), "source"),
    (dict(source=numpy.ones((2, 61)), block=3), "source"), (dict(source=numpy.ones((2, 3, 60)), block=3), "source"),
    (dict(source=numpy.ones((0, 60)), block=3), "source"),
    (dict(source=numpy.where(numpy.arange(60) == 7, 0.0, 1.0), block=3), "non-positive"),
    (dict(source=numpy.where(numpy.arange(60) == 7, -1.0, 1.0), block=3), "non-positive"),
    (dict(source=numpy.where(numpy.arange(60) == 7, numpy.nan, 1.0), block=3), "non-finite"),
    (dict(source=numpy.where(numpy.arange(60) == 7, numpy.inf, 1.0), block=3), "non-finite"),
    (dict(sigma=0.01, seed=-1), "seed"), (dict(sigma=0.01, seed=2 ** 64), "seed"), (dict(sigma=0.01, seed=1.5), "seed"),
    (dict(sigma=0.01, first_trial=-1), "first_trial"), (dict(sigma=0.01, first_trial=2 ** 62), "counter"),
    (dict(sigma=0.01, chunk=0), "chunk"), (dict(sigma=0.01, dy=numpy.ones(59)), "dy"),
    (dict(sigma=0.01, dy=numpy.ones((3, 60))), "dy"),
    (dict(sigma=0.01, dy=numpy.zeros(60)), "dy"), (dict(sigma=0.01, dy=numpy.full((4, 60), numpy.nan)), "dy"),
])
def test_null_sde_argument_errors(kwargs, match):
    with pytest.raises(ValueError, match=match):
        survey.null_sde(_t(), 4, **kwargs)


def test_null_sde_trials_and_series_errors():
    for n_trials in (0, -3, 2.0, None):
        with pytest.raises(ValueError, match="n_trials"):
            survey.null_sde(_t(), n_trials, sigma=0.01)
    for t in (numpy.zeros((2, 30)), numpy.zeros(0)):
        with pytest.raises(ValueError, match="t must"):
            survey.null_sde(t, 4, sigma=0.01)
    with pytest.raises(ValueError, match="ascending"):
        survey.null_sde(_t()[::-1], 4, sigma=0.01, statistics=True)
    # (the counter bound is the C entry's: the last trial's last block stays below 2^64)
    n = 60
    blocks = -(-2 * n // 4)
    last = (2 ** 64 - 2) // blocks
    with pytest.raises(ValueError, match="counter"):
        survey.null_sde(_t(n), 4, sigma=0.01, first_trial=last - 3)


def test_fap_table_errors():
    for bad in ([1.0, numpy.nan], [1.0, numpy.inf], [-numpy.inf, 2.0]):
        with pytest.raises(ValueError, match="non-finite"):
            survey.fap_table(bad)
    for bad in ([], [[1.0, 2.0]], 3.0):
        with pytest.raises(ValueError, match="1-d"):
            survey.fap_table(bad)
    for max_fap in (0.0, -0.1, 1.5, numpy.nan):
        with pytest.raises(ValueError, match="max_fap"):
            survey.fap_table([1.0, 2.0], max_fap)


def test_sde_threshold_errors():
    table = survey.fap_table(numpy.arange(1000.0), 0.1)
    assert survey.sde_threshold(table, 0.001) == 998.0
    assert survey.sde_threshold(table, 0.1) == 899.0
    for target in (0.0009, 0.102, 0.5, -1.0, numpy.nan):
        with pytest.raises(ValueError, match="target_fap"):
            survey.sde_threshold(table, target)
    fap, thr, n = table
    with pytest.raises(ValueError, match="fap_table"):
        survey.sde_threshold((fap[:-1], thr, n), 0.01)
    with pytest.raises(ValueError, match="fap_table"):
        survey.empirical_fap(5.0, (fap, thr[::-1], n))
