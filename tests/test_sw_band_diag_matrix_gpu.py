"""Banded alignment around a diagonal under a substitution matrix on the device (agx_sw_batch_create_align_band_diag_matrix /
agx_sw_align_band_diag_matrix): every comparison is exact, all five hit fields, against the by-definition checker of
tests/sw_band_diag_matrix_ref.py or against the entries the header names as equivalent.  Shapes are chosen for where the banded
fill can go wrong -- every K and G of the lane tiling, every fpad, trimmed rows, groups of mixed row counts -- not for a workload."""
import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_diag_matrix_cases as cases
from tests import sw_band_diag_matrix_ref as mr

pytestmark = pytest.mark.gpu

FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
MODES = pytest.mark.parametrize("mode", mr.MODES, ids=[mr.MODE_NAMES[m] for m in mr.MODES])
NOTHING = (0, -1, -1, -1, -1)


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


def _same(got, want, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---- 1. the tiling sweep


@pytest.mark.parametrize("w", cases.WIDTHS)
def test_tiling_sweep(ctx, w):
    """Half-widths across all four K and G = 1 .. 64; la in 1 .. 300 and lb up to about 700 mixed within one batch; every residue
    of c mod 4 (every fpad); c + w < 0 (the first filled row is > 0) in FIT and LOCAL; positive centres with la < c + w; a LOCAL
    band that misses the matrix; empty sides.  Random and related proteins under BLOSUM62, all five modes, ENDS and SPANS."""
    m = cases.blosum62()
    for mode in mr.MODES:
        b, cs, rel = cases.sweep(mode, w)
        la = b.len[0::2].astype(np.int64)
        assert {int(c) % 4 for c in cs} == ({0, 1, 2, 3} if w >= 2 or mode in (mr.LOCAL, mr.FIT) else {int(c) % 4 for c in range(-w, w + 1)})
        if mode in (mr.LOCAL, mr.FIT):
            assert (cs + w < 0).any()
        if w > 0 and mode != mr.FIT:
            assert ((cs > 0) & (la < cs + w) & (la > 0)).any()
        assert ((b.len[0::2] == 0) | (b.len[1::2] == 0)).sum() >= 3
        for what in (mr.ENDS, mr.SPANS):
            want = mr.align(b, m, mode, w, cs, what)
            if mode in (mr.LOCAL, mr.FIT):  # a condition on the inputs: the comparison is not between zeros
                assert np.all(want["score"][rel] > 0)
            if mode == mr.LOCAL:
                assert tuple(int(v) for v in want[b.n_pairs - 6]) == NOTHING  # the band misses the matrix
            _same(ctx.sw_align_band_diag(b, mode, w, cs, what, matrix=m), want, "%s w=%d what=%d" % (mr.MODE_NAMES[mode], w, what))


# ---- 2. the equivalences the header names


@MODES
@pytest.mark.parametrize("what", [mr.ENDS, mr.SPANS], ids=["ends", "spans"])
def test_a_band_that_holds_the_whole_matrix_equals_the_unbanded_matrix_batch(ctx, mode, what):
    b = synth.protein_pairs(300, 0, 200, 801, 0.6)
    m = cases.blosum62()
    want = ctx.sw_align(b, what, mode=mode, matrix=m)
    for c, w in ((0, 200), (-37, 237)):
        _same(ctx.sw_align_band_diag(b, mode, w, c, what, matrix=m), want, "c=%d w=%d" % (c, w))


def _dna(mode, w, seed, n=200):
    """DNA reads in their windows, in either case, with the centres of the planted diagonals (pinned modes: around 0)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGTacgt", np.uint8)
    seqs, cs = [], []
    for _ in range(n):
        la = int(rng.integers(1, 200))
        a = acgt[rng.integers(0, 8, size=la)].tobytes()
        copy = bytearray(a.swapcase() if rng.random() < 0.5 else a)
        for k in rng.integers(0, la, size=la // 12):
            copy[k] = acgt[rng.integers(0, 8)]
        pinned = mode in cases.PINNED
        s = int(rng.integers(0, min(w, 8) + 1)) if pinned else int(rng.integers(0, 300))
        tail = int(rng.integers(0, max(0, w - s) + 1)) if mode == mr.GLOBAL else int(rng.integers(0, 200))
        t = acgt[rng.integers(0, 8, size=s)].tobytes() + bytes(copy) + acgt[rng.integers(0, 8, size=tail)].tobytes()
        c = -s + (int(rng.integers(-1, 2)) if w >= 2 and not pinned else 0)
        if mode == mr.GLOBAL:
            c = -((s + tail) // 2)
        if mr.admits(mode, la, len(t), c, w):
            seqs += [a, t]
            cs.append(c)
    assert len(cs) > n // 2
    return synth.sw_from_seqs(seqs), np.array(cs, np.int32)


@MODES
@pytest.mark.parametrize("scoring", [(1, -1, -3, -1), (5, -4, -10, -2)], ids=str)
def test_the_restated_scoring_equals_the_match_mismatch_batch(ctx, mode, scoring):
    """The ACGT matrix that restates a supported scoring, on sequences in upper and lower case (one code per letter): hit for hit
    what agx_sw_align_band_diag reports under the scoring on the same sequences in one case."""
    m = mr.restated(*scoring)
    for w in (0, 3, 24):
        b, cs = _dna(mode, w, 810 + w)
        assert np.any(b.bases >= ord("a")) and np.any(b.bases < ord("a"))
        upper = synth.SWBatch(np.frombuffer(bytes(b.bases).upper(), np.uint8).copy(), b.off, b.len)
        for what in (mr.ENDS, mr.SPANS):
            want = ctx.sw_align_band_diag(upper, mode, w, cs, what, scoring)
            assert np.any(want["score"] > 20 * scoring[0])
            _same(ctx.sw_align_band_diag(b, mode, w, cs, what, matrix=m), want, "w=%d what=%d" % (w, what))


# ---- 3. the value range


def test_the_longest_pair_at_the_highest_entry(ctx):
    """65 535 x 65 535 at w = 8 over a one-symbol matrix of +127: GLOBAL and EXTEND score 127 x 65 535 along the main diagonal."""
    m = agx.SwMatrix.build(b"A", [[127]], -1000, -1000)
    b = synth.sw_from_seqs([b"A" * 65535, b"A" * 65535])
    for mode in (mr.GLOBAL, mr.EXTEND):
        want = mr.align(b, m, mode, 8, 0)
        assert int(want["score"][0]) == 127 * 65535
        _same(ctx.sw_align_band_diag(b, mode, 8, 0, matrix=m), want, mr.MODE_NAMES[mode])


def test_the_longest_pair_at_the_lowest_entry_and_the_dearest_gaps(ctx):
    """65 535 x 65 535 at w = 8 over a two-symbol matrix whose entries are all -128, gaps -1000 / -1000: GLOBAL and EXTEND_QUERY."""
    m = agx.SwMatrix.build(b"AC", [[-128, -128], [-128, -128]], -1000, -1000)
    rng = np.random.default_rng(820)
    ac = np.frombuffer(b"AC", np.uint8)
    b = synth.sw_from_seqs([ac[rng.integers(0, 2, size=65535)].tobytes(), ac[rng.integers(0, 2, size=65535)].tobytes()])
    for mode in (mr.GLOBAL, mr.EXTEND_QUERY):
        want = mr.align(b, m, mode, 8, 0)
        assert int(want["score"][0]) <= -128 * 65535 + 2000 and int(want["score"][0]) >= -128 * 65535 - 36000
        _same(ctx.sw_align_band_diag(b, mode, 8, 0, matrix=m), want, mr.MODE_NAMES[mode])


def test_local_under_a_matrix_without_a_positive_entry_consumes_nothing(ctx):
    m = agx.SwMatrix.build(b"ACGT", -np.ones((4, 4), np.int8) + np.eye(4, dtype=np.int8), -3, -1)  # 0 on the diagonal, -1 elsewhere
    b, cs = _dna(mr.LOCAL, 8, 821)
    for what in (mr.ENDS, mr.SPANS):
        got = ctx.sw_align_band_diag(b, mr.LOCAL, 8, cs, what, matrix=m)
        assert all(tuple(int(v) for v in h) == NOTHING for h in got)
    got = ctx.sw_align_band_diag(b, mr.EXTEND, 400, 0, matrix=m)
    assert all(tuple(int(v) for v in h) == NOTHING for h in got)


# ---- 4. the batch's life


@MODES
def test_relaunch_scores_and_the_calls_the_batch_refuses(ctx, mode):
    w = 16
    b, cs, _ = cases.sweep(mode, w, seed=5)
    m = cases.blosum62()
    want = mr.align(b, m, mode, w, cs)
    dev = ctx.sw_batch(b, matrix=m, mode=mode, band=w, diag=cs)
    try:
        assert dev.info().cells == b.cells() and dev.info().n_waves > 0
        bound = agx.host_array(b.n_pairs, np.int32)
        bound[:] = -77
        dev.bind_scores(bound)
        dev.launch()
        got = dev.hits()
        _same(got, want, "batch")
        assert np.array_equal(dev.scores(), got["score"])
        assert np.all(bound == -77)  # accepted and ignored
        dev.bind_scores(None)
        dev.launch()
        _same(dev.hits(), want, "relaunch")
        for call in (dev.stats, dev.zdrop_stops, dev.cigars):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_ARG
    finally:
        dev.close()
    empty = ctx.sw_align_band_diag(synth.sw_from_seqs([]), mode, w, None, matrix=m)
    assert empty.size == 0


def test_a_byte_outside_the_alphabet_names_the_lowest_pair(ctx):
    """... also a byte in a row of b that the band never touches, and in the cigar batch; byte 0x00 is such a byte under BLOSUM62."""
    m = cases.blosum62()
    rng = np.random.default_rng(830)
    read = cases.prot(rng, 40)
    window = cases.prot(rng, 300) + read + cases.prot(rng, 300)
    far = bytearray(window)
    far[5] = ord("B")  # row 5: the band around -300 at w = 8 starts at row 292
    good = [read, window]
    for bad_pair, seqs in ((2, good + good + [read, bytes(far)] + good), (1, good + [read[:10] + b"\x00" + read[11:], window] + [read, bytes(far)]),
                           (0, [read[:10] + b"J" + read[11:], window] + good)):
        b = synth.sw_from_seqs(seqs)
        for cigar in (False, True):
            with pytest.raises(agx.AgxError) as e:
                if cigar:
                    ctx.sw_align_band_diag_cigar(b, mr.FIT, 8, -300, matrix=m)
                else:
                    ctx.sw_align_band_diag(b, mr.FIT, 8, -300, matrix=m)
            assert e.value.code == agx.E_SYMBOL and "pair %d " % bad_pair in str(e.value), (bad_pair, cigar, str(e.value))
