"""The coverage of tests/test_stage_memory.py, checked without a GPU: every device buffer of a context is either smeared by
tls_debug_poison_lds (its kind where it is declared is scratch) or kept for a reason stated here (state), every Context method that launches a stage kernel has a case, and the
pairs of cases lie on the two sides of the constants that separate their memory paths.  A stage added without a case, or a
buffer added without a decision, fails here."""
import ast
import os
import re

import pytest

import stage_memory_cases as cases
from tls_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tls_amd", "csrc", "tls_amd.hip")

# the DevBufs of tls_ctx that tls_debug_poison_lds leaves alone: what they hold between two calls is state by design
KEPT = {
    "d_plan": "the plan: tls_prepare fills it once, every launch of the plan reads it",
    "d_perm_table": "the plan's table of folded orders: the plan's first four-slot launch stores it, every later one reads it",
    "d_band": "the band prefix of the plan's width table, kept while band_sigma / band_eps (the host's cache key) stay",
    "d_out": "the results: tls_fetch and tls_spectra without chi2 read what the last search wrote (Context.holds)",
    "d_stage": "results staged slot by slot (tls_comm_stage_results) for a later tls_comm_allgather_staged",
    "d_gather": "gathered results a later tls_comm_fetch_gathered / tls_comm_fetch_staged copies out",
    "d_queue": "a queue counter whose zero state between launches is the kernels' own invariant",
    "d_squeue": "the search kernel's self-rewinding queue: zero between launches by the kernel's own last step",
    "d_pqueues": "the T0-fit queues of tls_power_batch: zero between launches by the kernels' own last step",
    "d_tiles_done": "the tiles-done counters of the two-role plan: zero between launches (tls_kernels.hip.h)",
    "d_check": "the bound-check counters of a checked build: they accumulate over the session (tls_debug_check_counts)",
    "d_phase": "the phase clock: tls_debug_phase_cycles reads what the last execute left",
    "d_sysrem_state": "SysRem's state words (flags and iteration counts), zeroed by tls_sysrem in front of its launches",
    "d_curve_S0": "a survey batch's per-curve inputs (the batch slots' d_S0 stands in for it through over_S0)",
    "d_curve_w0": "a survey batch's per-curve inputs (the batch slots' d_w0 stands in for it through over_w0)",
}

# Context methods that launch a stage kernel and have no case in stage_memory_cases
EXEMPT = {
    "folded_views": "tests/test_folded_views.py::test_poisoned_lds_and_reused_scratch runs it behind poison and reused scratch",
}

STAGE_METHODS_FIRST, STAGE_METHODS_LAST = "inject_transits", "ephemeris_match"
CHAIN_METHODS = ("power_batch", "power_batch_stats", "debug_peak_fits", "debug_transit_stats", "debug_transit_models", "spectra",
                 "pink_noise", "t0_fit_residuals")


def _braces(text, start):
    """The text between the brace at or behind `start` and its partner."""
    open_at = text.index("{", start)
    depth = 0
    for i in range(open_at, len(text)):
        depth += text[i] == "{"
        depth -= text[i] == "}"
        if depth == 0:
            return text[open_at + 1:i]
    raise AssertionError("unbalanced braces")


def _without_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _registered():
    """{member: kind} of every DevBuf<...> member of struct tls_ctx, the BatchSlot members apart: each is constructed against
    the context's pool with its own name and its kind, where it is declared."""
    text = _without_comments(open(SOURCE).read())
    body = _braces(text, text.index("struct tls_ctx {"))
    slot = _braces(body, body.index("struct BatchSlot"))
    assert "DevBuf<" in slot
    body = body.replace(slot, "")
    found = {}
    for members in re.findall(r"DevBuf<[^>]+>\s+([^;]+);", body):
        parts = re.findall(r'(\w+)\{pool, "(\w+)", (kScratch|kState)\}', members)
        assert len(parts) == members.count("{") == members.count("}") == members.count("},") + 1, members   # no bare member
        for member, name, kind in parts:
            assert member == name and member not in found, member
            found[member] = kind
    assert all(re.fullmatch(r"d_\w+", n) for n in found), sorted(found)
    assert len(found) > 50
    return found


def declared_buffers():
    return set(_registered())


def smeared_buffers():
    """tls_debug_poison_lds walks the context's pool and smears the buffers of kind scratch, and those alone."""
    text = _without_comments(open(SOURCE).read())
    body = _braces(text, text.index("int tls_debug_poison_lds(tls_ctx* ctx, uint32_t word)"))
    assert "ctx->pool.first" in body and "b->kind == kScratch" in body and "ctx->d_" not in body
    return {name for name, kind in _registered().items() if kind == "kScratch"}


def test_every_device_buffer_is_smeared_or_kept_for_a_reason():
    declared, smeared = declared_buffers(), smeared_buffers()
    assert not smeared & set(KEPT), sorted(smeared & set(KEPT))
    assert smeared | set(KEPT) == declared, (sorted(declared - smeared - set(KEPT)), sorted((smeared | set(KEPT)) - declared))
    assert all(len(reason) > 20 for reason in KEPT.values())
    # the stage buffers the invariant was never enforced for, by name
    for name in ("d_pfit d_pfep d_pfres d_pfstats d_pfranges d_scan d_single d_times d_vetting d_shape d_centroid d_gls d_match "
                 "d_tstats d_tranges d_models d_spec d_pink d_peaks d_peak_mask d_detrend d_windows d_sysrem d_inject d_null").split():
        assert name in smeared, name
    # ... the buffers smeared before stay smeared
    for name in "d_scratch d_lists d_perm d_split d_park d_fscratch d_frot d_frperm d_views".split():
        assert name in smeared, name
    # ... and the queues and counters the issue of the kernels' zero state names are kept
    for name in "d_queue d_squeue d_pqueues d_tiles_done d_check d_phase d_sysrem_state".split():
        assert name in KEPT, name


def stage_methods():
    """The Context methods that launch a stage kernel: the public ones from inject_transits to ephemeris_match in definition
    order, and the post-search chain's."""
    tree = ast.parse(open(os.path.join(REPO, "tls_amd", "_lib.py")).read())
    context = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Context")
    names = [n.name for n in context.body if isinstance(n, ast.FunctionDef)]
    first, last = names.index(STAGE_METHODS_FIRST), names.index(STAGE_METHODS_LAST)
    assert first < last
    stages = [n for n in names[first:last + 1] if not n.startswith("_")]
    chain = [n for n in names if n.startswith("power_batch")] + [n for n in CHAIN_METHODS if not n.startswith("power_batch")]
    assert set(CHAIN_METHODS) <= set(names) and set(chain) == set(CHAIN_METHODS), sorted(set(chain) ^ set(CHAIN_METHODS))
    return stages + chain


def test_every_stage_method_has_a_case():
    covered = {case.method for case in cases.CASES.values()}
    methods = stage_methods()
    assert len(methods) >= 26
    for name in methods:
        assert (name in covered) != (name in EXEMPT), name
    assert covered <= set(methods), sorted(covered - set(methods))
    for name, case in cases.CASES.items():
        assert case.entry in _lib.SYMBOLS and hasattr(_lib.Context, case.method), name
    entries = {case.entry for case in cases.CASES.values()}
    for entry in ("tls_spectra tls_t0_fit tls_pink_noise tls_power_batch tls_power_batch_stats tls_power_batch_models "
                  "tls_power_batch_peaks tls_debug_peak_fits tls_debug_transit_stats tls_debug_transit_models tls_find_peaks "
                  "tls_phase_scan tls_single_transits tls_transit_times tls_event_vetting tls_shape_fit tls_centroid_test tls_nudft "
                  "tls_lomb_scargle tls_sine_test tls_prewhiten tls_ephemeris_match tls_medfilt_detrend tls_biweight_detrend "
                  "tls_sysrem tls_inject_transits tls_null_rows").split():
        assert entry in entries, entry


def test_the_tables_name_cases():
    for stage, constant, low, high, side in cases.PAIRS:
        assert cases.CASES[low].stage == cases.CASES[high].stage == stage, (stage, low, high)
    for stage, (large, small) in cases.BEHIND.items():
        assert large in cases.CASES and small in cases.CASES and large != small, stage
        assert cases.CASES[large].run is not cases.CASES[small].run
    paired = {cases.CASES[k].stage for pair in cases.BEHIND.values() for k in pair}
    assert {case.stage for case in cases.CASES.values()} - paired == set(), "a stage without a small call behind a large one"


@pytest.mark.parametrize("pair", cases.PAIRS, ids=lambda p: "%s-%s" % (p[2], p[3]))
def test_the_pairs_straddle_their_constants(pair):
    stage, constant, low, high, side = pair
    assert side(cases.CASES[low].size(), constant) == (True, False), (low, cases.CASES[low].size(), constant)
    assert side(cases.CASES[high].size(), constant) == (False, True), (high, cases.CASES[high].size(), constant)


def test_the_periodogram_shapes_fill_no_tile():
    """F is no multiple of GLS_FREQ_TILE and n none of GLS_CHUNK in every periodogram case; dy and no dy on both sides of the
    small product kernel."""
    names = [k for k, c in cases.CASES.items() if c.stage in ("lomb_scargle", "nudft")]
    assert len(names) == 6
    for name in names:
        size = cases.CASES[name].size()
        assert size["F"] % _lib.GLS_FREQ_TILE and size["n"] % _lib.GLS_CHUNK, (name, size)
    for rows in ("3_rows", "40_rows"):
        assert {"lomb_scargle_" + rows, "lomb_scargle_" + rows + "_dy"} <= set(names)


def test_the_windows_and_kernels_are_the_smallest_and_the_largest():
    small, large = (cases.CASES["biweight_%s_window" % k].size() for k in ("smallest", "largest"))
    assert small == 1 and large == 256                      # (below one cadence: the point alone; longer than the row: all of it)
    small, large = (cases.CASES["medfilt_%s_kernel" % k].size() for k in ("smallest", "largest"))
    assert small == 1 and 1 < large <= 256


_STATED = [k for k, c in cases.CASES.items() if c.want is not None and not c.want_on_device]


@pytest.mark.parametrize("name", _STATED)
def test_the_statement_of_a_case_runs_on_the_cpu(name):
    want = cases.CASES[name].want()
    assert want is not None and len(cases.arrays(want)) > 0


def test_the_cases_without_a_cpu_statement_are_the_power_batch_entries():
    rest = sorted(k for k in cases.CASES if k not in _STATED)
    assert rest == ["peak_fits_general_kernel_15", "peak_fits_rotation_path_17", "power_batch_models_one_row", "power_batch_one_row",
                    "power_batch_peaks_five_rows", "power_batch_stats_one_row"]
    assert all(cases.CASES[k].want_on_device for k in rest[:2]) and cases.CASES["power_batch_peaks_five_rows"].compare is not None
