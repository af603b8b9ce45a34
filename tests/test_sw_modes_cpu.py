"""Alignment modes (global, fit, extension) without a GPU: the checker itself (tests/sw_modes_ref.py) against a second,
independent formulation and against the inequalities that tie the modes together; the new C-ABI on plan-only batches;
the anchored kernels' resources as the code objects state them."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_align_ref as loc
from tests import sw_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -(10 ** 9)


def _table(a, b, sc, free):
    """D of include/agx.h by GAP-LENGTH ENUMERATION: a cell is reached by a diagonal move or by one whole gap of k cells
    (cost gap_open + k gap_extend) from any cell above it or left of it.  No E/F matrices."""
    match, mis, go, ge = sc
    la, lb = len(a), len(b)
    D = [[NEG] * (la + 1) for _ in range(lb + 1)]
    for i in range(lb + 1):
        for j in range(la + 1):
            if i == 0 and j == 0:
                D[i][j] = 0
                continue
            if j == 0 and free:
                D[i][j] = 0
                continue
            v = NEG
            if i and j:
                v = D[i - 1][j - 1] + (match if a[j - 1] == b[i - 1] else mis)
            for k in range(1, i + 1):
                v = max(v, D[i - k][j] + go + k * ge)
            for k in range(1, j + 1):
                v = max(v, D[i][j - k] + go + k * ge)
            D[i][j] = v
    return D


def _by_enumeration(a, b, sc, mode):
    """(score, a_begin, a_end, b_begin, b_end) with SPANS, straight from the table of include/agx.h."""
    la, lb = len(a), len(b)
    D = _table(a, b, sc, mode == ref.FIT)
    if mode == ref.GLOBAL:
        i, j = lb, la
    elif mode == ref.EXTEND:
        best = max(max(r) for r in D)
        i, j = next((i, j) for i in range(lb + 1) for j in range(la + 1) if D[i][j] == best)
        if best == 0:
            return (0, -1, -1, -1, -1)
    else:
        best = max(D[i][la] for i in range(lb + 1))
        i, j = next(i for i in range(lb + 1) if D[i][la] == best), la
    score, b_begin = D[i][j], 0
    if mode == ref.FIT and i > 0:  # the latest s whose PINNED alignment of a with b[s..i) reaches the score
        b_begin = max(s for s in range(i + 1) if _table(a, b[s:i], sc, False)[i - s][la] == score)
        assert b_begin < i  # b_end >= 0 means some of b is consumed: else the smaller i = 0 would have been reported
    return (score, 0, j - 1, b_begin, i - 1)


@pytest.mark.parametrize("scoring", [(1, -1, -3, -1), (2, -3, 0, -2), (1, 0, 0, 0)], ids=str)
def test_checker_against_gap_length_enumeration(scoring):
    """Every pair over {A, C} with lengths 0..5 (63 x 63 pairs), all four modes, all five fields."""
    words = [bytes(w) for n in range(6) for w in itertools.product(b"AC", repeat=n)]
    seqs = [s for a in words for b in words for s in (a, b)]
    for mode in ref.MODES:
        got = ref.align_seqs(seqs, mode, ref.SPANS, scoring)
        ends = ref.align_seqs(seqs, mode, ref.ENDS, scoring)
        for p, (h, e) in enumerate(zip(got, ends)):
            a, b = seqs[2 * p], seqs[2 * p + 1]
            assert h == _by_enumeration(a, b, scoring, mode), (ref.MODE_NAMES[mode], a, b)
            assert e == (h[0], -1, h[2], -1, h[4])


def test_hand_worked_cases():
    # reference scoring +1 / -1 / -3 / -1
    assert ref.align_seqs([b"ACGT", b"ACGT"], ref.GLOBAL) == [(4, 0, 3, 0, 3)]
    assert ref.align_seqs([b"", b"ACGT"], ref.GLOBAL) == [(-7, 0, -1, 0, 3)]  # one gap of four: -3 + 4 * -1
    assert ref.align_seqs([b"ACGT", b""], ref.GLOBAL) == [(-7, 0, 3, 0, -1)]
    assert ref.align_seqs([b"", b""], ref.GLOBAL) == [(0, 0, -1, 0, -1)]
    assert ref.align_seqs([b"ACG", b"TTACGTTACG"], ref.FIT) == [(3, 0, 2, 2, 4)]  # the first of two placements
    assert ref.align_seqs([b"ACG", b""], ref.FIT) == [(-6, 0, 2, 0, -1)]
    assert ref.align_seqs([b"", b"ACG"], ref.FIT) == [(0, 0, -1, 0, -1)]
    assert ref.align_seqs([b"ACGTTT", b"ACGAAA"], ref.EXTEND) == [(3, 0, 2, 0, 2)]
    assert ref.align_seqs([b"TTT", b"AAA"], ref.EXTEND) == [(0, -1, -1, -1, -1)]
    assert ref.align_seqs([b"ACG", b"ACGAAA"], ref.EXTEND_QUERY) == [(3, 0, 2, 0, 2)]
    assert ref.align_seqs([b"ACG", b"TTT"], ref.EXTEND_QUERY) == [(-3, 0, 2, 0, 2)]  # three mismatches beat a gap of three (-6)


@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2), (1, 0, 0, 0)], ids=str)
def test_checker_global_equals_the_span_checkers_global(scoring):
    b = synth.sw_pairs(400, 1, 60, seed=41, related_frac=0.5)
    got = ref.align(b, ref.GLOBAL, ref.ENDS, scoring)
    for p in range(b.n_pairs):
        assert got["score"][p] == loc.global_score(b.seq(2 * p), b.seq(2 * p + 1), scoring)


@pytest.mark.parametrize("scoring", [None, (3, -2, 0, -1)], ids=str)
def test_inequalities_between_the_modes(scoring):
    """Every mode restricts the one before it: local >= FIT >= EXTEND_QUERY >= GLOBAL, local >= EXTEND >= 0,
    EXTEND >= EXTEND_QUERY -- pair by pair."""
    b = synth.sw_pairs(2000, 1, 70, seed=42, related_frac=0.5)
    local = loc.align(b, loc.ENDS, scoring)["score"]
    s = {m: ref.align(b, m, ref.ENDS, scoring)["score"] for m in ref.MODES}
    assert np.all(local >= s[ref.FIT]) and np.all(s[ref.FIT] >= s[ref.EXTEND_QUERY]) and np.all(s[ref.EXTEND_QUERY] >= s[ref.GLOBAL])
    assert np.all(local >= s[ref.EXTEND]) and np.all(s[ref.EXTEND] >= 0)
    assert np.all(s[ref.EXTEND] >= s[ref.EXTEND_QUERY])
    assert np.any(local > s[ref.FIT]) and np.any(s[ref.FIT] > s[ref.EXTEND_QUERY]) and np.any(s[ref.EXTEND_QUERY] > s[ref.GLOBAL])


@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2)], ids=str)
def test_checker_fit_spans_are_spans(scoring):
    """a aligns END TO END with b[b_begin..b_end] at exactly the FIT score, and with no later begin."""
    b = synth.sw_pairs(600, 1, 50, seed=43, related_frac=0.6)
    hits = ref.align(b, ref.FIT, ref.SPANS, scoring)
    seen = 0
    for p, h in enumerate(hits):
        a, t = b.seq(2 * p), b.seq(2 * p + 1)
        assert h["a_begin"] == 0 and h["a_end"] == len(a) - 1 and -1 <= h["b_end"] < len(t)
        if h["b_end"] < 0:
            assert h["b_begin"] == 0
            continue
        seen += 1
        assert 0 <= h["b_begin"] <= h["b_end"]
        assert loc.global_score(a, t[h["b_begin"]:h["b_end"] + 1], scoring) == h["score"]
        for s in range(h["b_begin"] + 1, h["b_end"] + 1):
            assert loc.global_score(a, t[s:h["b_end"] + 1], scoring) < h["score"]
    assert seen > 500


# ---- the C-ABI


def test_new_symbols_are_exported():
    lib = C.CDLL(agx.LIB_PATH)
    for s in ("agx_sw_batch_create_align_mode", "agx_sw_align_mode"):
        assert s in agx.SYMBOLS and hasattr(lib, s), s
    assert agx.SwHit.itemsize == 20
    assert (agx.SW_MODE_LOCAL, agx.SW_MODE_GLOBAL, agx.SW_MODE_FIT, agx.SW_MODE_EXTEND, agx.SW_MODE_EXTEND_QUERY) == (0, 1, 2, 3, 4)
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    for k, name in enumerate(("LOCAL", "GLOBAL", "FIT", "EXTEND", "EXTEND_QUERY")):
        assert "#define AGX_SW_MODE_%s %d\n" % (name, k) in hdr
    v = agx.lib().agx_version()
    assert b"0.3." in v and v != b"agx 0.3 (gfx950)"


def test_bad_mode_is_an_argument_error():
    b = synth.sw_pairs(4, 5, 20, seed=4)
    for mode in (-1, 5, 99):
        h = C.c_void_p()
        rc = agx.lib().agx_sw_batch_create_align_mode(None, None, mode, agx.SW_ALIGN_ENDS, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len),
                                                      b.n_pairs, C.byref(h))
        assert rc == agx.E_ARG and not h.value and b"mode" in agx.lib().agx_last_error()
        out = np.empty(b.n_pairs, agx.SwHit)
        rc = agx.lib().agx_sw_align_mode(None, None, mode, agx.SW_ALIGN_ENDS, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, agx._ptr(out))
        assert rc == agx.E_ARG and b"mode" in agx.lib().agx_last_error()
    h = C.c_void_p()
    rc = agx.lib().agx_sw_batch_create_align_mode(None, None, agx.SW_MODE_FIT, 0, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h))
    assert rc == agx.E_ARG and not h.value and b"what" in agx.lib().agx_last_error()


@pytest.mark.parametrize("mode", range(5))
@pytest.mark.parametrize("what", [agx.SW_ALIGN_ENDS, agx.SW_ALIGN_SPANS])
def test_plan_only_batch_in_every_mode(mode, what):
    """ctx == NULL: the batch answers agx_sw_batch_info and nothing else."""
    b = synth.sw_from_seqs([b"ACGT" * 20, b"ACGT" * 30, b"", b"ACG", b"ACG", b""] + [b"ACGTT" * 7, b"GATTACA" * 9] * 40)
    h = C.c_void_p()
    rc = agx.lib().agx_sw_batch_create_align_mode(None, None, mode, what, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h))
    assert rc == agx.OK and h.value
    try:
        assert agx.lib().agx_sw_batch_launch(h) == agx.E_NODEVICE
        out = np.empty(b.n_pairs, agx.SwHit)
        assert agx.lib().agx_sw_batch_hits(h, agx._ptr(out)) == agx.E_NODEVICE
    finally:
        agx.lib().agx_sw_batch_destroy(h)
    dev = agx.SwBatch(None, b, align=what, mode=mode)
    try:
        i = dev.info()
        assert i.n_pairs == b.n_pairs and i.cells == b.cells() and i.padded_cells >= i.cells and i.n_waves > 0
        for call in (dev.launch, dev.hits, dev.scores):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_NODEVICE
    finally:
        dev.close()


@pytest.mark.parametrize("mode", range(5))
def test_query_limit_holds_in_every_mode(mode):
    rng = np.random.default_rng(5)
    seq = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()
    agx.SwBatch(None, synth.sw_from_seqs([seq(2560), seq(10), seq(10), seq(5000)]), align=agx.SW_ALIGN_ENDS, mode=mode).close()
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, synth.sw_from_seqs([seq(2561), seq(10)]), align=agx.SW_ALIGN_ENDS, mode=mode)
    assert e.value.code == agx.E_LIMIT and "2560" in str(e.value)
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, synth.sw_from_seqs([seq(10), seq(65536)]), align=agx.SW_ALIGN_ENDS, mode=mode)
    assert e.value.code == agx.E_LIMIT


def test_mode_needs_an_align_batch():
    b = synth.sw_pairs(4, 5, 20, seed=4)
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, b, mode=agx.SW_MODE_GLOBAL)
    assert e.value.code == agx.E_ARG


def test_anchored_kernels_resources():
    """Every anchored kernel: no scratch, no AGPRs, at most 256 VGPRs, no LDS (tools/kernel_resources.py reads the code
    objects' own notes).  Two captures (anywhere / the query's last column) for each of the 19 column classes 4..40."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.kernel_resources(agx.LIB_PATH)
    anch = {k: v for k, v in table.items() if k.startswith("sw_fill_anch<")}
    assert len(anch) == 38, sorted(anch)
    for k, r in anch.items():
        assert r["scratch"] == 0 and r["agpr"] == 0 and r["vgpr"] <= 256 and r["lds"] == 0, (k, r)
