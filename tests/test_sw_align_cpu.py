"""Alignment coordinates without a GPU: the checker itself (tests/sw_align_ref.py) against hand-worked cases, the
oracle's scores and an independent statement of what a span is; the new C-ABI on a plan-only batch; the locating
kernels' resources as the code objects state them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (0, -1, -1, -1, -1)


# (a, b, expected (score, a_begin, a_end, b_begin, b_end)) under the reference scoring +1 / -1 / -3 / -1, worked by hand
HAND = {
    # ACGT sits once in b, at 2..5
    "unique": (b"ACGT", b"TTACGTCC", (4, 0, 3, 2, 5)),
    # ACG twice in b: score 3 ends at b = 2 and at b = 7; the smaller b wins
    "two maxima, different rows": (b"ACG", b"ACGTTACG", (3, 0, 2, 0, 2)),
    # ACG twice in a: score 3 ends at a = 2 and a = 7 in the one row b = 2; the smaller a wins
    "two maxima, same row": (b"ACGTTACG", b"ACG", (3, 0, 2, 0, 2)),
    # H[i][j] = min(i, j) + 1: the maximum 3 stands in the cells (b 2, a 2) and (b 2, a 3); from (2, 2) backwards AAA x AAA
    "homopolymer, a longer": (b"AAAA", b"AAA", (3, 0, 2, 0, 2)),
    # ... and in (b 2..4, a 2)
    "homopolymer, b longer": (b"AAA", b"AAAAA", (3, 0, 2, 0, 2)),
    # 20 matches around one extra T in b: 20 - (3 + 1) = 16, more than either half alone (10)
    "gap": (b"ACGTACGTAC" b"GGTTGGTTGG", b"ACGTACGTAC" b"T" b"GGTTGGTTGG", (16, 0, 19, 0, 20)),
    # the two newlines align behind four matches: the newline pair is the end cell
    "newline pair carries the maximum": (b"ACGT\n", b"ACGT\n", (5, 0, 4, 0, 4)),
    # the copy ends in a's newline only: b's G cannot match it, the end cell stays on the T
    "one newline": (b"ACGT\n", b"ACGTG", (4, 0, 3, 0, 3)),
    # the begin takes the LATEST start: ends at (a 4, b 2) with score 3; backwards from there only CGT x CGT
    "begin inside a": (b"AACGT", b"CGT", (3, 2, 4, 0, 2)),
    "score 0": (b"AAAA", b"CCCC", NONE),
    "empty a": (b"", b"ACGT", NONE),
    "empty b": (b"ACGT", b"", NONE),
    "both empty": (b"", b"", NONE),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_checker_on_hand_worked_cases(name):
    a, b, want = HAND[name]
    assert ref.align_seqs([a, b], ref.SPANS) == [want]
    ends = ref.align_seqs([a, b], ref.ENDS)[0]
    assert ends == (want[0], -1, want[2], -1, want[4])


def test_checker_runtime_scoring_by_hand():
    # match 5, mismatch -4, first gap cell -10 - 1: ACGT x ACCT = 5 + 5 - 4 + 5 = 11 beats AC alone (10)
    assert ref.align_seqs([b"ACGT", b"ACCT"], ref.SPANS, (5, -4, -10, -1)) == [(11, 0, 3, 0, 3)]
    # mismatch -11: the mismatch no longer pays; AC (10) ends first at b = 1
    assert ref.align_seqs([b"ACGT", b"ACCT"], ref.SPANS, (5, -11, -10, -1)) == [(10, 0, 1, 0, 1)]


@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2), (5, -4, -10, -1)])
def test_checker_scores_equal_the_oracle(oracle, scoring):
    for seed, lo, hi, nl in ((11, 1, 90, True), (12, 20, 160, False)):
        b = synth.sw_pairs(1500, lo, hi, seed=seed, related_frac=0.5, newline=nl)
        got = ref.align(b, ref.ENDS, scoring)["score"]
        want = oracle.sw_batch(b) if scoring is None else oracle.sw_batch_scored(b, scoring)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2)])
def test_checker_spans_are_spans(scoring):
    """Independently of how the checker found them: the two substrings of a span align END TO END (global affine-gap
    score, no zero floor) with exactly the local score, their first and last symbols match, and ENDS agrees with SPANS."""
    b = synth.sw_pairs(1200, 1, 80, seed=21, related_frac=0.6, newline=True)
    hits = ref.align(b, ref.SPANS, scoring)
    ends = ref.align(b, ref.ENDS, scoring)
    assert np.array_equal(hits["score"], ends["score"]) and np.array_equal(hits["a_end"], ends["a_end"]) and np.array_equal(hits["b_end"], ends["b_end"])
    seen = 0
    for p, h in enumerate(hits):
        a, t = b.seq(2 * p), b.seq(2 * p + 1)
        if h["score"] == 0:
            assert tuple(h)[1:] == (-1, -1, -1, -1)
            continue
        seen += 1
        assert 0 <= h["a_begin"] <= h["a_end"] < len(a) and 0 <= h["b_begin"] <= h["b_end"] < len(t)
        sa, sb = a[h["a_begin"]:h["a_end"] + 1], t[h["b_begin"]:h["b_end"] + 1]
        assert sa[0] == sb[0] and sa[-1] == sb[-1]
        assert ref.global_score(sa, sb, scoring) == h["score"]
    assert seen > 1000


# ---- the C-ABI


def test_new_symbols_are_exported_and_the_version_moved():
    lib = C.CDLL(agx.LIB_PATH)
    for s in ("agx_sw_batch_create_align", "agx_sw_batch_hits", "agx_sw_align"):
        assert s in agx.SYMBOLS and hasattr(lib, s), s
    assert agx.SwHit.itemsize == 20
    assert b"0.3" in agx.lib().agx_version()


@pytest.mark.parametrize("what", [agx.SW_ALIGN_ENDS, agx.SW_ALIGN_SPANS])
def test_plan_only_align_batch(what):
    """ctx == NULL: the batch answers agx_sw_batch_info and nothing else."""
    b = synth.sw_pairs(300, 5, 200, seed=3, related_frac=0.5)
    dev = agx.SwBatch(None, b, align=what)
    try:
        i = dev.info()
        assert i.n_pairs == 300 and i.cells == b.cells() and i.padded_cells >= i.cells and i.n_waves > 0
        for call in (dev.launch, dev.hits, dev.scores, lambda: dev.bind_scores(None)):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_NODEVICE
    finally:
        dev.close()


def test_bad_what_and_bad_batch_are_argument_errors():
    b = synth.sw_pairs(4, 5, 20, seed=4)
    for what in (0, 3, -1):  # (the C entry point itself: align=0 means "score-only" in the Python view)
        h = C.c_void_p()
        rc = agx.lib().agx_sw_batch_create_align(None, None, what, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h))
        assert rc == agx.E_ARG and not h.value and b"what" in agx.lib().agx_last_error()
    plain = agx.SwBatch(None, b)  # a score-only batch has no hits
    try:
        with pytest.raises(agx.AgxError) as e:
            plain.hits()
        assert e.value.code == agx.E_ARG
    finally:
        plain.close()


def test_query_limit_is_on_the_role_not_on_the_shorter_side():
    """An align batch lays a (the query) across the lanes whichever is shorter: len(a) <= 2560 = 64 lanes x 40 columns."""
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    assert "#define AGX_SW_ALIGN_MAX_QUERY_LEN 2560" in hdr and "#define AGX_SW_ALIGN_MAX_TARGET_LEN 65535" in hdr
    assert agx.SW_ALIGN_MAX_QUERY_LEN == 2560 and agx.SW_ALIGN_MAX_TARGET_LEN == 65535
    rng = np.random.default_rng(5)
    seq = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()
    ok = synth.sw_from_seqs([seq(2560), seq(10), seq(10), seq(5000)])
    agx.SwBatch(None, ok, align=agx.SW_ALIGN_ENDS).close()
    too_long = synth.sw_from_seqs([seq(2561), seq(10)])  # the score-only planner would lay the 10 across the lanes
    agx.SwBatch(None, too_long).close()
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, too_long, align=agx.SW_ALIGN_ENDS)
    assert e.value.code == agx.E_LIMIT and "2560" in str(e.value)


def test_locating_kernels_resources():
    """Every locating kernel: no scratch, no AGPRs, at most 256 VGPRs, no LDS (tools/kernel_resources.py reads the code
    objects' own notes)."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.kernel_resources(agx.LIB_PATH)
    loc = {k: v for k, v in table.items() if k.startswith("sw_fill_loc<")}
    assert len(loc) == 19, sorted(loc)  # one per column class 4..40
    for k, r in loc.items():
        assert r["scratch"] == 0 and r["agpr"] == 0 and r["vgpr"] <= 256 and r["lds"] == 0, (k, r)
