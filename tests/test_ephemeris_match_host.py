"""The ephemeris match without a GPU: the numpy statement (tests/ephemeris_match_spec.py) by hand at every edge, its symmetry,
and what it is for -- a diluted copy of an eclipsing binary on a neighbouring star is found and named a child; tls_match_record
in the header and its mirrors; the entry in the header, the binding and the library; the argument checks of
survey.ephemeris_match and survey.power_batch(ephemeris_match=True) before any device work."""
import ctypes
import os
import re

import numpy
import pytest

import ephemeris_match_spec as spec
from conftest import REPO
from tls_amd import _lib, survey

T = numpy.linspace(3.0, 43.0, 1920)
FLUX = numpy.ones((2, 1920))
# seeds of spec.field for which the statement alone reports no match among the independent stars (checked below; of seeds 0 to
# 19, seeds 5 and 16 have a chance match and are left out)
SEEDS = (0, 1, 2, 3, 4, 6, 7, 8)


def same(got, want):
    for k in spec.FIELDS:
        numpy.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.fixture
def no_device(monkeypatch):
    """Creating a context, or loading the library, fails the test."""
    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    monkeypatch.setattr(_lib, "load", no_context)
    monkeypatch.setattr(survey._search, "default_context", no_context)


@pytest.mark.parametrize("case", spec.by_hand(), ids=lambda c: c[0])
def test_statement_by_hand(case):
    """Dyadic numbers, so every comparison is exact: drift at plim and one ulp beyond, dt at elim and one ulp beyond, rint on a
    half (2.5 -> 2, 3.5 -> 4), m at max_ratio and above, one star, equal strengths, equal periods, a bad candidate of each
    kind."""
    name, kw, want = case
    same(spec.match(**kw), want)


def test_the_edges_are_edges():
    """One ulp decides: what the by-hand cases claim of the pairs themselves."""
    by_name = {name: kw for name, kw, want in spec.by_hand()}
    pm, match = spec.relation(**by_name["drift edge"])
    assert pm[0, 1] and pm[1, 0] and not pm[0, 2] and not pm[2, 0]
    assert not pm[1, 2] and not pm[2, 1]                                  # (one star: a ulp apart, never matched)
    pm, match = spec.relation(**by_name["epoch edge"])
    assert pm[0, 1] and match[0, 1] and pm[0, 2] and not match[0, 2] and match[1, 2] and match[2, 1]
    pm, match = spec.relation(**by_name["max_ratio"])
    assert pm[0, 1] and not pm[0, 2]
    assert numpy.rint(2.5) == 2 and numpy.rint(3.5) == 4


@pytest.mark.parametrize("seed", range(4))
def test_the_relation_is_symmetric(seed):
    args = spec.clustered(seed, 300)
    pm, match = spec.relation(*args)
    assert match.sum() > 300 and pm.sum() > match.sum()
    numpy.testing.assert_array_equal(pm, pm.T)
    numpy.testing.assert_array_equal(match, match.T)
    rec = spec.match(*args)
    numpy.testing.assert_array_equal(rec["n_match"], match.sum(axis=0))
    numpy.testing.assert_array_equal(rec["n_period"], pm.sum(axis=0))
    assert rec["n_match"].sum() == match.sum() and match.sum() % 2 == 0
    # the best of f is a match of f, and no match of f is stronger
    f = numpy.flatnonzero(rec["best"] >= 0)
    best = rec["best"][f].astype(int)
    assert match[f, best].all()
    strength = args[4]
    assert (numpy.where(match[f], strength[None, :], -numpy.inf).max(axis=1) == strength[best]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_a_diluted_binary_is_found_and_named_a_child(seed):
    args, members = spec.field(seed)
    rec = spec.match(*args)
    source, second, double = members
    others = numpy.setdiff1d(numpy.arange(len(rec)), members)
    assert (rec["status"] == 0).all()
    assert (rec["n_match"][others] == 0).all() and (rec["best"][others] == -1).all()     # the condition on the seeds
    assert (rec["n_match"][members] == 2).all()
    assert rec["best"][second] == source and rec["best"][double] == source and rec["best"][source] == second
    assert rec["child"][second] == 1 and rec["child"][double] == 1 and rec["child"][source] == 0
    assert abs(rec["best_ratio"][second]) == 1 and rec["best_ratio"][double] == -2 and abs(rec["best_ratio"][source]) == 1
    assert rec["best_strength"][double] == 0.05 and rec["best_dt"][double] <= 0.02
    for groups in (spec.groups(rec), survey.ephemeris_groups(rec)):
        assert (groups[members] == source).all()
        numpy.testing.assert_array_equal(groups[others], others)


def test_groups_follow_a_chain():
    """best need not be the root: 0 <- 1 <- 2 by `best`, and 3 whose best is weaker than itself."""
    rec = numpy.zeros(5, dtype=spec.DTYPE)
    rec["best"] = [1, 2, 4, 0, -1]
    rec["child"] = [1, 1, 1, 0, numpy.nan]
    numpy.testing.assert_array_equal(survey.ephemeris_groups(rec), [4, 4, 4, 3, 4])
    numpy.testing.assert_array_equal(spec.groups(rec), [4, 4, 4, 3, 4])
    assert survey.ephemeris_groups(rec).dtype == numpy.int64 and len(survey.ephemeris_groups(rec[:0])) == 0


def test_tls_match_record_is_ten_doubles():
    assert ctypes.sizeof(_lib.MatchRecord) == 10 * 8 == _lib.MATCH_DTYPE.itemsize
    assert tuple(n for n, _ in _lib.MatchRecord._fields_) == _lib.MATCH_FIELDS == spec.FIELDS == _lib.MATCH_DTYPE.names
    assert survey.ephemeris_match_fields() == spec.FIELDS
    assert [_lib.MATCH_DTYPE.fields[k][1] for k in _lib.MATCH_DTYPE.names] == list(range(0, 80, 8))
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct tls_match_record \{(.*?)\} tls_match_record;", code, flags=re.S).group(1)
    declared = [n.strip() for line in body.split(";") if line.strip() for n in line.replace("double", "").split(",")]
    assert tuple(declared) == _lib.MATCH_FIELDS
    assert (_lib.MATCH_MATCHED, _lib.MATCH_BAD) == (spec.MATCHED, spec.BAD) == (0, 1)
    assert "#define TLS_MATCH_MAX_CANDIDATES %d" % _lib.MATCH_MAX_CANDIDATES in text and _lib.MATCH_MAX_CANDIDATES == 2 ** 20
    assert "#define TLS_MATCH_MAX_RATIO %d" % _lib.MATCH_MAX_RATIO in text and _lib.MATCH_MAX_RATIO == 64
    kernel = open(os.path.join(REPO, "tls_amd", "csrc", "tls_match.hip.h")).read()
    assert "constexpr int kMatchTile = %d;" % _lib.MATCH_TILE in kernel
    assert "constexpr int kMatchTargetGroups = %d;" % _lib.MATCH_TARGET_GROUPS in kernel
    assert "constexpr int kMatchMaxChunks = %d;" % _lib.MATCH_MAX_CHUNKS in kernel
    assert "constexpr int kMatchWords = 10;" in kernel and "#pragma clang fp contract(off)" in kernel


def test_the_chunks_of_the_other_side():
    T_ = _lib.MATCH_TILE
    assert _lib.match_chunks(0) == [0] and _lib.match_chunks(1) == [0, 1] and _lib.match_chunks(T_) == [0, T_]
    assert _lib.match_chunks(3 * T_ + 5) == [0, T_, 2 * T_, 3 * T_, 3 * T_ + 5]          # a tile a chunk
    edges = _lib.match_chunks(17 * T_ + 5)                                               # 18 tiles in 16 chunks
    assert len(edges) == 17 and edges[-1] == 17 * T_ + 5 and sorted(set(numpy.diff(edges[:-1]))) == [T_, 2 * T_]
    assert len(_lib.match_chunks(32768)) == 9 and len(_lib.match_chunks(2 ** 20)) == 2   # enough workgroups without a split
    for n in (1, 255, 257, 4096, 4357, 9000, 32768, 100000, 2 ** 20):
        edges = _lib.match_chunks(n)
        assert edges[0] == 0 and edges[-1] == n and all(b > a for a, b in zip(edges, edges[1:])), n
        assert all(e % T_ == 0 for e in edges[:-1]) and len(edges) - 1 <= _lib.MATCH_MAX_CHUNKS


def test_header_binding_and_library_declare_the_entry():
    text = open(os.path.join(REPO, "include", "tls_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    name = "tls_ephemeris_match"
    assert re.search(r"\bint\s+%s\s*\(" % name, code) and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "(8: %s)" % name in text.split("#define TLS_AMD_ABI_VERSION")[0]       # (the version comment lists the entry)
    assert "#define TLS_AMD_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8 == lib.tls_abi_version()
    squeeze = lambda s: re.sub(r"\s*,\s*", ", ", re.sub(r"\s+", " ", s)).strip()
    declared = squeeze(re.search(r"\bint\s+%s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
    assert declared == ("tls_ctx *ctx, const int64_t *star, const double *period, const double *T0, const double *duration, "
                        "const double *strength, int64_t n, double span, double drift_tolerance, double epoch_tolerance, "
                        "int64_t max_ratio, tls_match_record *out")
    assert len(lib.tls_ephemeris_match.argtypes) == declared.count(",") + 1 == 12


GOOD = ([0, 1], [3.0, 3.0], [4.0, 4.0], [0.1, 0.1], [2.0, 1.0], 40.0)


@pytest.mark.parametrize("kw", [dict(span=0.0), dict(span=-1.0), dict(span=numpy.inf), dict(span=numpy.nan), dict(span="1"),
                                dict(span=True), dict(drift_tolerance=-0.5), dict(drift_tolerance=numpy.inf),
                                dict(drift_tolerance=numpy.nan), dict(epoch_tolerance=-1e-9), dict(epoch_tolerance=numpy.nan),
                                dict(epoch_tolerance=None), dict(max_ratio=0), dict(max_ratio=65), dict(max_ratio=2.0),
                                dict(max_ratio=True), dict(max_ratio=-3)], ids=str)
def test_bad_arguments_raise(no_device, kw):
    a = dict(zip(("star", "period", "T0", "duration", "strength", "span"), GOOD))
    a.update(kw)
    with pytest.raises(ValueError, match="ephemeris match"):
        survey.ephemeris_match(**a)
    with pytest.raises(ValueError, match="ephemeris match"):
        _lib.ephemeris_match_arguments(**a)
    names = dict(drift_tolerance="ephemeris_match_drift", epoch_tolerance="ephemeris_match_epoch", max_ratio="ephemeris_match_max_ratio")
    if "span" not in kw:
        with pytest.raises(ValueError, match="ephemeris match"):
            survey.power_batch(T, FLUX, peaks=4, peak_fits=True, ephemeris_match=True, **{names[k]: v for k, v in kw.items()})


def test_bad_shapes_raise(no_device):
    star, period, T0, duration, strength, span = GOOD
    with pytest.raises(ValueError, match=r"\[M\]"):
        survey.ephemeris_match(star, period, T0[:1], duration, strength, span)
    with pytest.raises(ValueError, match=r"\[M\]"):
        survey.ephemeris_match([star], [period], [T0], [duration], [strength], span)
    with pytest.raises(ValueError, match="integers"):
        survey.ephemeris_match([0.5, 1.0], period, T0, duration, strength, span)
    with pytest.raises(ValueError, match="numbers"):
        survey.ephemeris_match(star, ["a", "b"], T0, duration, strength, span)
    many = numpy.zeros(_lib.MATCH_MAX_CANDIDATES + 1)
    with pytest.raises(ValueError, match="at most"):
        survey.ephemeris_match(many.astype(numpy.int64), many, many, many, many, span)
    a = _lib.ephemeris_match_arguments(numpy.array([7, -2], dtype=numpy.int32), period, T0, duration, strength, 40, max_ratio=numpy.int64(5))
    assert a["star"].dtype == numpy.int64 and list(a["star"]) == [7, -2] and a["span"] == 40.0 and a["max_ratio"] == 5
    assert (a["drift_tolerance"], a["epoch_tolerance"]) == (0.5, 0.5)


def test_ephemeris_match_without_peak_fits_raises(no_device):
    with pytest.raises(ValueError, match="peak_fits"):
        survey.power_batch(T, FLUX, ephemeris_match=True)
    with pytest.raises(ValueError, match="peak_fits"):
        survey.power_batch(T, FLUX, peaks=4, ephemeris_match=True)
    with pytest.raises(ValueError, match="peaks"):
        survey.power_batch(T, FLUX, peak_fits=True, ephemeris_match=True)


def test_fields_of_the_widened_peaks_array():
    """The records of the fitted peaks land on their (curve, rank); best becomes (match_curve, match_rank)."""
    names = survey.ephemeris_match_peak_fields()
    assert names == ("match_status", "match_n_same", "match_n_period", "match_n_match", "match_curve", "match_rank", "match_ratio",
                     "match_dt", "match_drift", "match_strength", "match_child")
    fits = numpy.zeros((3, 2), dtype=_lib.PEAK_FIT_DTYPE)
    fits["status"] = [[0, 1], [0, 0], [2, 0]]
    records = survey._with_fits(survey._with_duration(numpy.zeros((3, 2), dtype=_lib.PEAK_DTYPE), None), fits, 1.0)
    at = numpy.flatnonzero(fits["status"].reshape(-1) == 0)
    assert list(at) == [0, 2, 3, 5]
    found = numpy.zeros(4, dtype=_lib.MATCH_DTYPE)
    found["best"] = [3, -1, 0, 1]                    # candidate 3 is peak (2, 1), candidate 0 peak (0, 0), candidate 1 peak (1, 0)
    found["n_match"] = [1, 0, 2, 1]
    found["best_ratio"] = [2, numpy.nan, -2, 1]
    found["child"] = [0, numpy.nan, 1, 1]
    out = survey._with_matches(records, (found, at, (3, 2)))
    assert out.dtype.names == records.dtype.names + names and out.shape == (3, 2)
    numpy.testing.assert_array_equal(out["match_status"], [[0, 1], [0, 0], [1, 0]])
    numpy.testing.assert_array_equal(out["match_curve"], [[2, -1], [-1, 0], [-1, 1]])
    numpy.testing.assert_array_equal(out["match_rank"], [[1, -1], [-1, 0], [-1, 0]])
    numpy.testing.assert_array_equal(out["match_n_match"], [[1, numpy.nan], [0, 2], [numpy.nan, 1]])
    numpy.testing.assert_array_equal(out["match_ratio"], [[2, numpy.nan], [numpy.nan, -2], [numpy.nan, 1]])
    numpy.testing.assert_array_equal(out["match_child"], [[0, numpy.nan], [numpy.nan, 1], [numpy.nan, 1]])
    assert out["match_curve"].dtype == out["match_rank"].dtype == numpy.int64
    numpy.testing.assert_array_equal(out["status"], fits["status"])
