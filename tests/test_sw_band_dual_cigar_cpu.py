"""CIGARs of batches banded around a diagonal under two-piece gap costs (include/agx.h, "CIGARs for batches banded around a
diagonal under two-piece gap costs") without a GPU: the new C-ABI on plan-only batches -- symbols, every argument error, the table
of band conditions on both sides of every edge, the plan's digest against the plain band-diag cigar batch's --, the by-definition
checker (tests/sw_band_dual_cigar_ref.py) against the one-piece cigar checker where one piece dominates and against a full-matrix
DP that takes the gap cost literally, the merged-run argument, the chunk bound, and the kernels' resources as the code objects
state them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_diag_cigar_ref as one_ref
from tests import sw_band_diag_ref as bd
from tests import sw_band_dual_cases as dc
from tests import sw_band_dual_cigar_cases as cc
from tests import sw_band_dual_cigar_ref as dcr
from tests import sw_band_dual_ref as du
from tests.test_sw_band_dual_cpu import _literal, _rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
MODES = pytest.mark.parametrize("mode", bd.MODES, ids=[bd.MODE_NAMES[m] for m in bd.MODES])
WHO = b"agx_sw_batch_create_align_band_diag_dual_cigar"


def _same(got, want, what=""):
    gh, go, gp = got
    wh, wo, wp = want
    for f in FIELDS:
        bad = np.nonzero(gh[f] != wh[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], gh[bad[0]], wh[bad[0]])
    bad = np.nonzero(np.asarray(go) != np.asarray(wo))[0]
    if bad.size == 0:
        assert np.array_equal(gp, wp), what
        return
    p = max(int(bad[0]) - 1, 0)
    assert False, "%s: pair %d: got %s, want %s" % (what, p, dcr.strings(go[p:p + 2] - go[p], gp[int(go[p]):int(go[p + 1])]),
                                                    dcr.strings(wo[p:p + 2] - wo[p], wp[int(wo[p]):int(wo[p + 1])]))


def _create(b, mode, w, diag=None, scoring=dc.S_MM2):
    h = C.c_void_p()
    d = agx._diag(diag, b.n_pairs)
    sc = C.byref(agx.SwScoringDual(*scoring)) if scoring is not None else None
    rc = agx.lib().agx_sw_batch_create_align_band_diag_dual_cigar(None, sc, mode, w, agx._ptr(d), agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len),
                                                                  b.n_pairs, C.byref(h))
    return rc, h


# ---- 1. the C-ABI on plan-only batches


def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(agx.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    for s in ("agx_sw_batch_create_align_band_diag_dual_cigar", "agx_sw_align_band_diag_dual_cigar", "agx_sw_cigar_rescore_dual"):
        assert s in agx.SYMBOLS and hasattr(lib, s) and ("int %s(" % s) in hdr, s
    s = "agx_sw_band_dual_cigar_bytes_bound"
    assert s in agx.SYMBOLS and hasattr(lib, s) and ("uint64_t %s(" % s) in hdr
    assert "CIGARs for batches banded around a diagonal under two-piece gap costs" in hdr


@MODES
def test_every_band_condition_on_both_sides_of_its_edge(mode):
    """Every (la, lb) in 0..6, w in 0..2 and c in -9..9: the create succeeds exactly where the table of "Banded alignment around a
    diagonal" admits the pair, empty sides included, and a refusal is AGX_E_ARG naming the pair."""
    rng = np.random.default_rng(1911)
    first = [_rand(rng, 9), _rand(rng, 9)]
    seen = [0, 0]
    for la in range(7):
        for lb in range(7):
            b = synth.sw_from_seqs(first + [_rand(rng, la), _rand(rng, lb)])
            for w in range(3):
                for c in range(-9, 10):
                    rc, h = _create(b, mode, w, [0, c])
                    msg = agx.lib().agx_last_error()
                    ok = bd.admits(mode, la, lb, c, w)
                    seen[int(ok)] += 1
                    if ok:
                        assert rc == agx.OK and h.value, (la, lb, w, c, msg)
                        agx.lib().agx_sw_batch_destroy(h)
                    else:
                        assert rc == agx.E_ARG and not h.value and b"pair 1:" in msg, (la, lb, w, c, rc, msg)
    assert seen[1] > 0 and (seen[0] > 0 or mode == bd.LOCAL)


def test_argument_errors():
    rng = np.random.default_rng(1912)
    short = [_rand(rng, 10), _rand(rng, 12)]
    b = synth.sw_from_seqs(short + short)
    err = agx.lib().agx_last_error
    for mode in bd.MODES:
        rc, h = _create(b, mode, 8, 0, scoring=None)  # no reference default for a second piece
        assert rc == agx.E_ARG and not h.value and WHO in err() and b"scoring is NULL" in err()
        rc, h = _create(b, mode, -1, 0)
        assert rc == agx.E_ARG and not h.value and b"band" in err() and WHO + b":" in err()
        rc, h = _create(b, mode, 1024, 0)  # 2w + 1 = 2049 > AGX_SW_BAND_MAX_WIDTH: the limit of every batch around a diagonal, no new one
        assert rc == agx.E_LIMIT and not h.value
        rc, h = _create(b, mode, 1023, 0)
        assert rc == agx.OK and h.value
        agx.lib().agx_sw_batch_destroy(h)
        for c in (65535 + 7 + 1, -(65535 + 7 + 1)):
            rc, h = _create(b, mode, 7, [0, c])
            assert rc == agx.E_ARG and not h.value and b"pair 1:" in err(), (mode, c)
        for k, (lo, hi) in enumerate(((1, 12), (None, 0), (-1000, 0), (-1000, 0), (-1000, 0), (-1000, 0))):
            for v, ok in ((lo, True), (hi, True), (hi + 1, False)) + (((lo - 1, False),) if lo is not None else ()):
                if v is None:
                    continue
                s = list(dc.S_MM2)
                s[k] = v
                rc, h = _create(b, mode, 8, 0, scoring=s)
                assert (rc == agx.OK and h.value) if ok else (rc == agx.E_LIMIT and not h.value and b"outside the supported range" in err()), (k, v, rc)
                if h.value:
                    agx.lib().agx_sw_batch_destroy(h)
    for mode in (-1, 5, 99):
        rc, h = _create(b, mode, 8, 0)
        assert rc == agx.E_ARG and not h.value and b"mode" in err()
    long = _rand(rng, 65536)
    rc, h = _create(synth.sw_from_seqs(short + [long, long[:65000]]), bd.FIT, 600, 0)
    assert rc == agx.E_LIMIT and not h.value and b"pair 1" in err()
    rc, h = _create(synth.sw_from_seqs(short + [long[:65535], long[1:]]), bd.GLOBAL, 1023, 0)  # the largest pair is planned, not refused
    assert rc == agx.OK and h.value
    agx.lib().agx_sw_batch_destroy(h)
    h = C.c_void_p(1)
    sc = C.byref(agx.SwScoringDual(*dc.S_MM2))
    rc = agx.lib().agx_sw_batch_create_align_band_diag_dual_cigar(None, sc, bd.FIT, 4, None, None, None, None, 3, C.byref(h))
    assert rc == agx.E_ARG and not h.value
    assert agx.lib().agx_sw_batch_create_align_band_diag_dual_cigar(None, sc, bd.FIT, 4, None, None, None, None, 0, None) == agx.E_ARG
    hits, off = np.empty(b.n_pairs, agx.SwHit), np.zeros(b.n_pairs + 1, np.uint64)
    assert agx.lib().agx_sw_align_band_diag_dual_cigar(None, sc, bd.FIT, 4, None, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs,
                                                       agx._ptr(hits), agx._ptr(off), None, 0) == agx.E_NODEVICE


@MODES
def test_plan_only_batch_answers_info_and_nothing_else(mode):
    rng = np.random.default_rng(1913)
    seqs = [b"ACGT" * 20, b"ACGT" * 20, b"", b"ACG", b"ACG", b"", b"", b""]
    for n in (1, 5, 150, 2000, 10000):
        a = _rand(rng, n)
        seqs += [a, a]
    b = synth.sw_from_seqs(seqs)
    for w in (4, 64, 700):
        dev = agx.SwBatch(None, b, mode=mode, band=w, diag=0, dual_cigar=dc.S_MM2)
        plain = agx.SwBatch(None, b, mode=mode, band=w, diag=0, cigar=True, scoring=dc.piece1(dc.S_MM2))
        try:
            i, j = dev.info(), plain.info()
            assert i.n_pairs == b.n_pairs and i.cells == b.cells()
            assert (i.n_waves, i.n_launches, i.padded_cells, i.input_bytes) == (j.n_waves, j.n_launches, j.padded_cells, j.input_bytes)
            ci = dev.cigar_info()
            assert (ci.n_traced, ci.n_chunks, ci.trace_cells, ci.trace_bytes_peak) == (0, 0, 0, 0)
            for call in (dev.launch, dev.hits, dev.scores, dev.cigars):
                with pytest.raises(agx.AgxError) as e:
                    call()
                assert e.value.code == agx.E_NODEVICE
            hits, stats = np.empty(b.n_pairs, agx.SwHit), np.empty(b.n_pairs, agx.SwStat)
            assert agx.lib().agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(stats)) == agx.E_ARG
            assert agx.lib().agx_sw_batch_zdrop_stops(dev._h, agx._ptr(np.zeros(b.n_pairs, np.int32))) == agx.E_ARG
        finally:
            dev.close()
            plain.close()
    for kw in (dict(stats=True), dict(cigar=True), dict(zdrop=5), dict(matrix=agx.SwMatrix()), dict(band_stats=True), dict(band=None),
               dict(scoring=(1, -1, -3, -1)), dict(dual=dc.S_MM2), dict(align=agx.SW_ALIGN_ENDS)):
        with pytest.raises(agx.AgxError) as e:
            agx.SwBatch(None, b, **dict(dict(mode=mode, band=4, diag=0, dual_cigar=dc.S_MM2), **kw))
        assert e.value.code == agx.E_ARG, kw
    with pytest.raises(agx.AgxError) as e:  # unchanged: dual= with cigar=True is no way to ask for this batch
        agx.SwBatch(None, b, mode=mode, band=4, diag=0, dual=dc.S_MM2, cigar=True)
    assert e.value.code == agx.E_ARG
    agx.SwBatch(None, b, mode=mode, band=4, dual_cigar=dc.S_MM2, align=agx.SW_ALIGN_SPANS).close()  # diag is optional: 0 for every pair


def test_plan_is_the_plain_cigar_batch_plan_digest_for_digest():
    """Lane tiling, waves, records, image and the tables a cigar batch keeps for its traced fills are those of
    agx_sw_batch_create_align_band_diag_cigar on the same pairs, band and diag under the first piece: every lane class has its
    traced two-piece build, so no plan over the narrower classes only was needed.  The AGX_TRACE_CREATE lines of the two creates
    are the same but for the kind."""
    got = cc.run_digests()
    assert sorted(got) == sorted(dc.DIGEST_CASES)
    for name, e in got.items():
        plain, dual = e["plain"], e["dual"]
        assert len(plain) == len(dual) == 4 and plain[0].startswith("kind: ") and " cigar 1 " in plain[0] and dual[0] == plain[0] + " dual", (name, plain, dual)
        assert plain[1].startswith("plan digest ") and plain[2].startswith("plan parts: ") and plain[3].startswith("image digest ")
        assert dual[1:] == plain[1:], (name, plain, dual)
        assert " 0 groups" not in plain[2]
    assert "launch K 32" in got["extend_query_w1023"]["dual"][2]  # the widest class is planned
    assert len({e["plain"][1] for e in got.values()}) == len(got)


# ---- 2. the checker

# piece 2 never beats piece 1 for any L >= 1: identical pieces; lower in both numbers
DOMINATED = [(2, -4, -4, -2, -4, -2), (2, -4, -4, -2, -6, -3), (1, -1, -3, -1, -3, -5), (1, 0, 0, 0, 0, 0), (3, -2, 0, -1, -1, -1)]
# piece 1 STRICTLY worse for every L >= 1: gap_open + gap_extend < gap_open2 + gap_extend2 and gap_extend <= gap_extend2
STRICTLY_WORSE = [(2, -4, -6, -3, -4, -2), (1, -1, -3, -5, -3, -1), (3, -2, -1, -1, 0, -1), (2, -4, -5, -2, -4, -2), (1, -1, -1, 0, 0, 0)]


@MODES
@pytest.mark.parametrize("w", [0, 1, 2, 3])
def test_checker_under_a_dominated_piece_equals_the_one_piece_cigar_checker(mode, w):
    b, cs = cc.small(bd.admits, mode, w, seed=1921, top=9)
    assert b.n_pairs >= 10
    for s in DOMINATED:
        _same(dcr.expected(b, mode, w, cs, s), one_ref.expected(b, mode, w, cs, dc.piece1(s)), "piece 2 dominated %s" % (s,))
    for s in STRICTLY_WORSE:
        _same(dcr.expected(b, mode, w, cs, s), one_ref.expected(b, mode, w, cs, dc.piece2(s)), "piece 1 strictly worse %s" % (s,))


def test_on_a_tie_between_the_pieces_no_equality_is_claimed():
    """S_SMALL, the scoring of the device's small shapes: piece 1 = (-2, -2) is the better one at L = 1, ties piece 2 = (-4, -1) at
    L = 2 and is worse beyond, so neither equivalence applies.  What holds: the checker's CIGARs pass path_checks, and its scores
    are at least both one-piece scores, strictly above each somewhere."""
    b, cs = cc.small(bd.admits, bd.GLOBAL, 3, seed=1922)
    h, off, ops = dcr.expected(b, bd.GLOBAL, 3, cs, cc.S_SMALL)
    assert dcr.path_checks(b, 3, cs, h, off, ops, cc.S_SMALL) == -1
    s1 = bd.align(b, bd.GLOBAL, 3, cs, bd.SPANS, dc.piece1(cc.S_SMALL))["score"]
    s2 = bd.align(b, bd.GLOBAL, 3, cs, bd.SPANS, dc.piece2(cc.S_SMALL))["score"]
    assert np.all(h["score"] >= np.maximum(s1, s2)) and np.any(h["score"] > s1) and np.any(h["score"] > s2)


@MODES
@pytest.mark.parametrize("s", [dc.S_MM2, dc.S_SWAP, (2, -4, -4, -2, -8, -1), (3, -5, -1, -3, -6, 0), dc.S_ZERO, (1, -1, 0, -2, -3, -1), cc.S_SMALL], ids=str)
def test_checker_equals_the_literal_full_matrix_dp(mode, s):
    """Pairs up to 12 x 12 in a band that holds the whole matrix: the checker's score is that of a DP that tries every gap length
    in every cell under the literal cost, and the checker's CIGAR consumes the span and rescores to it under the literal cost of
    every maximal run (path_checks, and the library's host check agx_sw_cigar_rescore_dual on the same list)."""
    rng = np.random.default_rng(1923 + mode)
    seqs = []
    for k in range(120):
        la, lb = (int(v) for v in rng.integers(0 if k % 10 == 0 else 1, 13, size=2))
        a = _rand(rng, la)
        if k % 3 == 0:
            t = _rand(rng, lb)
        else:  # a with a stretch cut out or put in
            cut = int(rng.integers(0, la + 1))
            L = int(rng.integers(1, 7))
            t = (a[:cut] + a[cut + L:]) if k % 3 == 1 else (a[:cut] + _rand(rng, L) + a[cut:])[:12]
        seqs += [a, t]
    b = synth.sw_from_seqs(seqs)
    h, off, ops = dcr.expected(b, mode, 13, 0, s)
    assert dcr.path_checks(b, 13, 0, h, off, ops, s) == -1
    sc = agx.SwScoringDual(*s)
    for p in range(b.n_pairs):
        a, t = seqs[2 * p], seqs[2 * p + 1]
        if a and t:
            want = _literal(a, t, s, mode)
            if mode in (bd.LOCAL, bd.EXTEND) and want[0] == 0:
                want = (0, -1, -1)
            assert (int(h["score"][p]), int(h["a_end"][p]), int(h["b_end"][p])) == want, (p, a, t, tuple(h[p]), want)
        ca, cb = (int(v[p]) for v in dcr.spans(h))
        x = np.frombuffer(a, np.uint8)[max(int(h["a_begin"][p]), 0):][:ca].copy()
        y = np.frombuffer(t, np.uint8)[max(int(h["b_begin"][p]), 0):][:cb].copy()
        o = ops[int(off[p]):int(off[p + 1])].copy()
        args = (agx._ptr(o) if o.size else None, o.size, agx._ptr(x) if ca else None, ca, agx._ptr(y) if cb else None, cb)
        assert agx.lib().agx_sw_cigar_rescore_dual(C.byref(sc), *args, int(h["score"][p])) == 1, (p, dcr.strings(off[p:p + 2] - off[p], o))
        if o.size:
            assert agx.lib().agx_sw_cigar_rescore_dual(C.byref(sc), *args, int(h["score"][p]) + 1) == 0


def test_small_shapes_meet_all_five_sources_and_all_four_extensions():
    """What tests/test_sw_band_dual_cigar_gpu.py relies on: over its small shapes under S_SMALL the walks of the checker take H from
    the diagonal move, E1, F1, E2 and F2, and stay in each of the four gap states."""
    met = 0
    for mode in bd.MODES:
        for w in range(4):
            b, cs = cc.small(bd.admits, mode, w)
            seen = []
            dcr.expected(b, mode, w, cs, cc.S_SMALL, seen=seen)
            met |= seen[0]
    assert met == dcr.SEEN_DIAGONAL | dcr.SEEN_SOURCES | dcr.SEEN_EXTENDED, hex(met)


# ---- 3. merged runs


def test_a_run_joined_from_both_pieces_costs_at_most_the_literal_run():
    """include/agx.h's argument, by enumeration: with opens <= 0, p1(L1) + p2(L2) <= max(p1(L1 + L2), p2(L1 + L2)) -- in either
    order -- for every setting of a coarse grid and all L1, L2 in 1..40; and for three stretches."""
    grid = (0, -1, -2, -4, -24, -1000)
    L = np.arange(1, 41)
    L1, L2 = np.meshgrid(L, L)
    for o1 in grid:
        for e1 in grid:
            for o2 in grid:
                for e2 in grid:
                    p1 = lambda n: o1 + n * e1  # noqa: E731
                    p2 = lambda n: o2 + n * e2  # noqa: E731
                    lit = np.maximum(p1(L1 + L2), p2(L1 + L2))
                    assert np.all(p1(L1) + p2(L2) <= lit), (o1, e1, o2, e2)
                    assert np.all(p1(L1) + p1(L2) <= lit) and np.all(p2(L1) + p2(L2) <= lit)
                    assert np.all(p1(L1) + p2(L2) + p1(3) <= np.maximum(p1(L1 + L2 + 3), p2(L1 + L2 + 3)))


@pytest.mark.parametrize("mode", [bd.GLOBAL, bd.FIT], ids=["global", "fit"])
def test_adjacent_planted_gaps_come_out_as_one_run_at_its_literal_cost(mode):
    """Two planted gaps with nothing between them (1..3 and 25..40 symbols) under S_MM2: the checker's CIGAR holds ONE run of their
    joint length on the right side, whichever pieces the walk passed through, and rescores under the literal cost."""
    b, L, in_a = cc.adjacent_gaps()
    h, off, ops = dcr.expected(b, mode, 64, 0, dc.S_MM2)
    assert dcr.path_checks(b, 64, 0, h, off, ops, dc.S_MM2) == -1
    hit = 0
    for p in range(b.n_pairs):
        o = ops[int(off[p]):int(off[p + 1])]
        gaps = [(int(v) & 15, int(v) >> 4) for v in o if (int(v) & 15) in (dcr.OP_I, dcr.OP_D)]
        hit += gaps == [(dcr.OP_I if in_a[p] else dcr.OP_D, int(L[p]))]
    assert hit == b.n_pairs, hit  # (a gap may slide along equal symbols of its flanks; its length and its side do not change)


# ---- 4. the chunk bound


def test_bytes_bound_has_eight_bits_a_cell():
    """Per class K a pair's directions are (cb + G) G K / 4 dwords, rounded up to four: for K >= 8 twice the four-bit figure
    (ceil(K / 8) dwords a lane and step), for K = 4 the same (the four-bit build fills half of its dword there).  The bound takes
    the worst class for the width, as agx_sw_band_cigar_bytes_bound does, so its direction part lies between the four-bit bound's
    and twice that, and is twice that -- but for the rounding to four dwords -- wherever K = 4 cannot tile the width (beyond 256
    diagonals)."""
    lib = agx.lib()
    rng = np.random.default_rng(1931)

    def formula(width, ca, cb, words):
        worst = 0
        for K in (4, 8, 16, 32):
            G = (width + K - 1) // K
            if G <= 64:
                worst = max(worst, ((cb + G) * G * words(K) + 3) & ~3)
        return 4 * worst, 4 * (ca + cb)

    widths = [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048] + [int(v) for v in rng.integers(1, 2049, size=200)]
    for width in widths:
        for ca, cb in ((1, 1), (150, 150), (10000, 9999), (65535, 65535), (int(rng.integers(1, 65536)), int(rng.integers(1, 65536)))):
            d8, slot = formula(width, ca, cb, lambda K: K // 4)
            d4, _ = formula(width, ca, cb, lambda K: (K + 7) // 8)
            assert lib.agx_sw_band_dual_cigar_bytes_bound(width, ca, cb) == d8 + slot
            assert lib.agx_sw_band_cigar_bytes_bound(width, ca, cb) == d4 + slot  # unchanged
            assert d4 <= d8 <= 2 * d4
            if width > 256:  # no K = 4 tiling: every class doubles
                assert 2 * d4 - 16 <= d8
    for width in (0, -1, 2049):
        assert lib.agx_sw_band_dual_cigar_bytes_bound(width, 10, 10) == 0
    assert lib.agx_sw_band_dual_cigar_bytes_bound(2048, 65535, 65535) == 4 * ((65535 + 64) * 64 * 8 + 2 * 65535)  # about 134 MB


# ---- 5. the kernels

TRACED_DUAL_VGPRS = {4: 94, 8: 109, 16: 142, 32: 224}


def test_kernel_resources():
    """Exactly the four traced two-piece builds and the one walk exist: no scratch, no spills, no LDS, no AGPRs, within the 256
    VGPRs of a 256-thread workgroup, the counts of DESIGN.md 4.1o's table.  sw_walk_band and sw_walk_band_at keep their 32 VGPRs,
    and no new kernel's name starts with a prefix the existing resource tests count."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.kernel_resources(agx.LIB_PATH)
    new = {k: v for k, v in table.items() if k.startswith("sw_fill_band_trace_dual")}
    assert sorted(new) == sorted("sw_fill_band_trace_dual<%d>" % K for K in (4, 8, 16, 32)), sorted(new)
    for k, r in list(new.items()) + [("sw_walk_band_dual", table["sw_walk_band_dual"])]:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0 and r["agpr"] == 0 and r["vgpr"] <= 256, (k, r)
    for K, vgpr in TRACED_DUAL_VGPRS.items():
        assert table["sw_fill_band_trace_dual<%d>" % K]["vgpr"] == vgpr, (K, table["sw_fill_band_trace_dual<%d>" % K])
    assert table["sw_walk_band_dual"]["vgpr"] == 34
    for k in ("sw_walk_band", "sw_walk_band_at"):
        r = table[k]
        assert r["vgpr"] == 32 and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (k, r)
    assert len([k for k in table if k.startswith("sw_walk_band")]) == 3
    counts = {"sw_fill_band_dual": 20, "sw_fill_band_trace<": 4, "sw_fill_band_trace_at<": 4, "sw_fill_band_trace_mat<": 4, "sw_fill_band<": 8,
              "sw_fill_band_at<": 12, "sw_fill_band_mat<": 20, "sw_fill_band_zd<": 4, "sw_fill_band_stats<": 8, "sw_fill_band_at_stats<": 8}
    for prefix, n in counts.items():
        assert len([k for k in table if k.startswith(prefix)]) == n, prefix
