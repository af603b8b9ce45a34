"""CIGARs of batches banded around a diagonal under two-piece gap costs on the device
(agx_sw_batch_create_align_band_diag_dual_cigar / agx_sw_align_band_diag_dual_cigar): every comparison is exact -- hits, op_off
and ops -- against the by-definition checker of tests/sw_band_dual_cigar_ref.py, or against the entry the header names as
equivalent.  Independently of the checker every returned CIGAR is walked from its begin cell: it stays in the band of the full
matrix, consumes exactly its span and rescores to its hit's score under the literal two-piece cost of every maximal run."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_diag_ref as bd
from tests import sw_band_dual_cases as dc
from tests import sw_band_dual_cigar_cases as cc
from tests import sw_band_dual_cigar_ref as dcr
from tests import sw_fuzz_cases as fz
from tests.test_sw_band_diag_cigar_gpu import PHASE_WIDTHS, _phase_pairs, _reads, _tiling
from tests.test_sw_band_diag_gpu import _mutate, _rand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
LOCAL, GLOBAL, FIT, EXTEND, EXTEND_QUERY = bd.MODES
MODES = pytest.mark.parametrize("mode", bd.MODES, ids=[bd.MODE_NAMES[m] for m in bd.MODES])
FREE = pytest.mark.parametrize("mode", [LOCAL, FIT], ids=["local", "fit"])
S_MM2, S_SWAP, S_EDGE, S_ZERO, S_SMALL = dc.S_MM2, dc.S_SWAP, dc.S_EDGE, dc.S_ZERO, cc.S_SMALL


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


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


def _batch(ctx, b, mode, w, diag, scoring=S_MM2):
    dev = ctx.sw_batch(b, mode=mode, band=w, diag=diag, dual_cigar=scoring)
    try:
        dev.launch()
        hits, op_off, ops = dev.cigars()
        return hits, op_off, ops.copy(), dev.cigar_info()
    finally:
        dev.close()


def _check(ctx, b, mode, w, diag, scoring=S_MM2, one_shot=False, want=None):
    """The batch (and the one-shot) against the checker, and every returned CIGAR against its band, span and literal score."""
    want = want or dcr.expected(b, mode, w, diag, scoring)
    name = "%s w=%d %s" % (bd.MODE_NAMES[mode], w, scoring)
    hits, op_off, ops, info = _batch(ctx, b, mode, w, diag, scoring)
    assert dcr.path_checks(b, w, diag, hits, op_off, ops, scoring) == -1, name
    _same((hits, op_off, ops), want, name + " batch")
    if one_shot:
        _same(ctx.sw_align_band_diag_dual_cigar(b, mode, w, diag, scoring), want, name + " one-shot")
    return want, (hits, op_off, ops), info


def _gap_runs(op_off, ops, p):
    o = ops[int(op_off[p]):int(op_off[p + 1])]
    return [(int(v) & 15, int(v) >> 4) for v in o if (int(v) & 15) in (dcr.OP_I, dcr.OP_D)]


# ---- 1. every small shape, every admitted centre


@MODES
@pytest.mark.parametrize("w", [0, 1, 2, 3])
def test_every_shape_up_to_10_around_every_admitted_centre(ctx, mode, w):
    """Over a two-letter alphabet under S_SMALL, whose pieces break even at L = 2: shapes this small meet piece 2, ties between the
    pieces and all five sources (tests/test_sw_band_dual_cigar_cpu.py asserts from the checker that over this very set all five
    sources and all four extended bits occur)."""
    b, cs = cc.small(bd.admits, mode, w)
    assert b.n_pairs >= 11  # (GLOBAL at w = 0 admits the square pairs around 0 only)
    _check(ctx, b, mode, w, cs, S_SMALL, one_shot=True)
    _check(ctx, b, mode, w, cs, S_ZERO)


# ---- 2. planted gaps across the break-even and across lanes


def test_the_planted_widths_lay_a_gap_across_lanes():
    """What the planner makes of the two widths on the planted pairs' rows: K = 16 on 9 lanes and K = 32 on 16, so a gap of 48
    crosses lane boundaries in the trace, upwards and to the left.  (The planner gives K = 4 and K = 8 to bands of one lane only,
    so no width lays a gap across lanes of K = 4; the start-phase widths below run those classes.)"""
    assert _tiling(2 * 64 + 1, 150) == (16, 9) and _tiling(2 * 255 + 1, 150) == (32, 16)


@pytest.mark.parametrize("mode", [GLOBAL, FIT], ids=["global", "fit"])
@pytest.mark.parametrize("w", [64, 255])
def test_planted_gaps_across_the_break_even_and_across_lanes(ctx, mode, w):
    """x + ins(L) + y against x + y under S_MM2, L = 1 .. 48 on either side of the break-even length 20, on either side of the
    pair: every CIGAR holds one gap run, of exactly L, on the right side."""
    b, L, in_a = dc.planted_gaps()
    want, (hits, op_off, ops), info = _check(ctx, b, mode, w, 0)
    assert info.n_traced == b.n_pairs
    for p in range(b.n_pairs):
        assert _gap_runs(op_off, ops, p) == [(dcr.OP_I if in_a[p] else dcr.OP_D, int(L[p]))], (p, dcr.strings(op_off[p:p + 2] - op_off[p], ops[int(op_off[p]):int(op_off[p + 1])]))
    _same(_batch(ctx, b, mode, w, 0, S_SWAP)[:3], want, "swapped pieces")  # (the hits; the operations too: no gap here is a tie of pieces)


@MODES
def test_both_pieces_within_one_alignment(ctx, mode):
    """One gap of 1 .. 3 and one of 30 .. 60 in every pair, w = 80: in every mode each CIGAR has one run of <= 3 and one of
    >= 30 and no other gap run."""
    b = dc.both_pieces()
    want, (hits, op_off, ops), _ = _check(ctx, b, mode, 80, 0)
    both = 0
    for p in range(b.n_pairs):
        runs = sorted(n for _, n in _gap_runs(op_off, ops, p))
        both += len(runs) == 2 and runs[0] <= 3 and runs[1] >= 30
    assert both == b.n_pairs, (mode, both)


# ---- 3. start phases and widths


def test_the_phase_widths_reach_every_class_and_its_lane_counts():
    seen = {_tiling(2 * w + 1, rows) for w in PHASE_WIDTHS for rows in (40, 120)}
    assert {(4, 1), (8, 1), (16, 1), (16, 3), (32, 1), (32, 3), (32, 16), (32, 32), (32, 64)} <= seen, sorted(seen)


@FREE
@pytest.mark.parametrize("w", PHASE_WIDTHS)
def test_spans_that_begin_at_every_phase(ctx, mode, w):
    """The pairs of tests/test_sw_band_diag_cigar_gpu.py (40 x 120, spans that begin at all sixteen (s mod 4, a_begin mod 4) in
    LOCAL, at every phase the band holds in FIT) at its fifteen widths: every class and lane count the planner makes, K = 32 from
    1 to 64 lanes."""
    b, cs = _phase_pairs(mode, w)
    want, (hits, _, _), info = _check(ctx, b, mode, w, cs)
    assert info.n_traced == b.n_pairs
    row0 = np.maximum(0, -(cs.astype(np.int64) + w))
    combos = {(int(s) & 3, int(a) & 3) for s, a in zip(hits["b_begin"] - row0, hits["a_begin"])}
    assert len(combos) == (16 if mode == LOCAL else min(4, 2 * w + 1)), sorted(combos)


# ---- 4. the two equivalences


@MODES
def test_the_two_equivalences_with_the_one_piece_cigar_batch(ctx, mode):
    """Piece 2 never the better one: hits and operations of agx_sw_align_band_diag_cigar under piece 1.  Piece 1 strictly worse
    for every L: those under piece 2."""
    b, cs = cc.small(bd.admits, mode, 3, seed=1941)
    rng = np.random.default_rng(1942)
    seqs, ds = [], []
    for _ in range(64):
        a = _rand(rng, int(rng.integers(40, 300)))
        t = _mutate(rng, a, indel=0.02, longest=30)
        a, t = fz._fit_to_band(mode, a, t, 40)  # the centre 0 at w = 40 must be admitted
        seqs += [a, t]
        ds.append(0)
    for batch, w, diag in ((b, 3, cs), (synth.sw_from_seqs(seqs), 40, np.array(ds, np.int32))):
        for s in ((2, -4, -4, -2, -4, -2), (2, -4, -4, -2, -6, -3), (1, -1, -3, -1, -3, -5), (3, -2, 0, -1, -1, -1)):
            _same(_batch(ctx, batch, mode, w, diag, s)[:3], ctx.sw_align_band_diag_cigar(batch, mode, w, diag, dc.piece1(s)), "dominated %s" % (s,))
        for s in ((2, -4, -6, -3, -4, -2), (1, -1, -3, -5, -3, -1), (3, -2, -1, -1, 0, -1), (2, -4, -5, -2, -4, -2)):
            _same(_batch(ctx, batch, mode, w, diag, s)[:3], ctx.sw_align_band_diag_cigar(batch, mode, w, diag, dc.piece2(s)), "strictly worse %s" % (s,))


# ---- 5. ties


@MODES
def test_ties_in_homopolymers_and_repeats(ctx, mode):
    """Homopolymers and two-letter repeats under S_ZERO, S_EDGE and S_SWAP: the maximum is reached by many alignments, through
    either piece; the tie rule picks one."""
    for w in (0, 3, 50):
        seqs, diag = [], []
        for n in (1, 2, 5, 13, 40):
            for m in (1, 2, 5, 13, 40):
                for a, t in ((b"A" * n, b"A" * m), (b"AC" * n, b"AC" * m), (b"AC" * n, b"CA" * m), (b"AC" * n, b"A" * m)):
                    for c in sorted({0, 1, -1, 2, -2, len(a) - len(t), (len(a) - len(t)) // 2, -len(t) + 1}):
                        if bd.admits(mode, len(a), len(t), c, w):
                            seqs += [a, t]
                            diag.append(c)
        assert len(diag) >= 16
        b = synth.sw_from_seqs(seqs)
        for scoring in (S_ZERO, S_EDGE, S_SWAP):
            _check(ctx, b, mode, w, np.array(diag, np.int32), scoring)


# ---- 6. lone runs, "*" and empty sides


def test_lone_runs_and_no_operations(ctx):
    sc = (1, -100, -1, -1, -3, 0)
    one = lambda seqs, mode, w, c, s=S_MM2: ctx.sw_align_band_diag_dual_cigar(synth.sw_from_seqs(seqs), mode, w, c, s)  # noqa: E731
    # FIT, all of a in one gap along one row: b_begin = b_end + 1 (tests/test_sw_band_diag_cigar_gpu.py has the one-piece twin):
    # a gap of 4 costs max(-1 - 4, -3 - 0) = -3 under piece 2
    hits, off, ops = one([b"TTTT", b"AAAAAAAAAA"], FIT, 2, -5, sc)
    assert tuple(int(v) for v in hits[0]) == (-3, 0, 3, 7, 6) and dcr.strings(off, ops) == ["4I"]
    seqs = [b"AAAA", b"CCCC", b"ACGT", b"ACGT", b"", b"ACGT", b"ACGT", b"", b"", b""]
    hits, off, ops = one(seqs, LOCAL, 1, [0, 9, 0, 0, 0])
    assert hits["score"][0] == 0 and hits["score"][1] == 0 and ops.size == 0 and dcr.strings(off, ops) == ["*"] * 5
    assert dcr.strings(*one([b"", b"ACGT", b"ACGT", b"", b"", b"", b"ACGT", b"ACGT"], GLOBAL, 4, 0)[1:]) == ["4D", "4I", "*", "4="]


@MODES
def test_empty_sides(ctx, mode):
    """One side empty, the other of 1 .. 40 symbols, among pairs that are filled: answered without a fill, a lone run (or none)
    at the two-piece cost of its length."""
    rng = np.random.default_rng(1943)
    seqs = []
    for n in range(1, 41):
        seqs += [b"", _rand(rng, n), _rand(rng, n), b"", _rand(rng, n), _rand(rng, n)]
    b = synth.sw_from_seqs(seqs)
    want, (hits, op_off, ops), info = _check(ctx, b, mode, 40, 0, one_shot=True)
    assert info.n_traced <= 40
    if mode == GLOBAL:
        n = np.arange(1, 41)
        assert np.array_equal(hits["score"][0::3], np.maximum(-4 - 2 * n, -24 - n))
        assert dcr.strings(op_off, ops)[:2] == ["1D", "1I"]


# ---- 7. one long pair


def test_twenty_thousand_at_the_widest_band_with_a_planted_deletion(ctx):
    """One 20 000 x 20 000 GLOBAL pair at c = 0, w = 1023: 64 lanes of K = 32, 41 MB of directions; 300 bases of a are missing in b
    at 9 000 (b is filled up at its end).  The CIGAR is checked by path_checks and holds a run of 300 I; the score is the
    checker's (its five band matrices of this pair would take the test beyond a few seconds)."""
    rng = np.random.default_rng(1944)
    a = _rand(rng, 20000)
    t = _mutate(rng, a[:9000] + a[9300:], indel=0.001) + _rand(rng, 600)
    b = synth.sw_from_seqs([a, t[:20000]])
    hits, op_off, ops, info = _batch(ctx, b, GLOBAL, 1023, 0)
    assert dcr.path_checks(b, 1023, 0, hits, op_off, ops) == -1
    want = dcr.dual_ref.align(b, GLOBAL, 1023, 0)
    assert tuple(int(v) for v in hits[0]) == tuple(int(v) for v in want[0]) and int(want["score"][0]) > 30000
    assert (dcr.OP_I, 300) in _gap_runs(op_off, ops, 0)
    assert info.trace_bytes_peak >= (20000 + 64) * 64 * 8 * 4 and info.n_chunks == 1


# ---- 8. chunking


@FREE
def test_chunking(mode):
    """A budget cut from agx_sw_band_dual_cigar_bytes_bound so that the batch needs at least three chunks and its largest pair
    exceeds the budget alone: the same answer as under the default, and cig_info.n_chunks says so."""
    b, cs = _reads(mode)
    w = 24
    want = dcr.expected(b, mode, w, cs)
    ca, cb = dcr.spans(want[0])
    need = [int(agx.lib().agx_sw_band_dual_cigar_bytes_bound(2 * w + 1, int(x), int(y))) for x, y in zip(ca, cb) if x and y]
    budget = max(need) - 1
    assert sum(need) > 3 * budget
    infos = {}
    for opt in (budget, None):
        with agx.Context(0) as c:
            if opt is not None:
                c.set_option(agx.OPT_SW_TRACE_BYTES, opt)
            hits, op_off, ops, infos[opt] = _batch(c, b, mode, w, cs)
        _same((hits, op_off, ops), want, "budget %s" % opt)
    cut, default = infos[budget], infos[None]
    assert default.n_chunks == 1 and 3 <= cut.n_chunks <= len(need)
    assert cut.n_traced == default.n_traced == len(need) and cut.trace_cells == default.trace_cells > 0
    assert cut.trace_bytes_peak <= max(need) and default.trace_bytes_peak <= sum(need)


# ---- 9. the batch's life and the other entry points


def test_lifecycle_mixed_order_and_a_batch_split_in_two(ctx):
    """Sizing call then the real call; a short ops_cap; the answer is kept until the next launch; a relaunch reproduces it; the
    pairs in another order and in two halves give the same records; stats() and zdrop_stops() on the new batch and cigars() on the
    plain two-piece batch are AGX_E_ARG."""
    mode, w = FIT, 24
    b, cs = _reads(mode)
    want = dcr.expected(b, mode, w, cs)
    n, lib = b.n_pairs, agx.lib()
    dev = ctx.sw_batch(b, mode=mode, band=w, diag=cs, dual_cigar=S_MM2)
    plain = ctx.sw_batch(b, mode=mode, band=w, diag=cs, dual=S_MM2)
    try:
        dev.launch()
        op_off = np.zeros(n + 1, np.uint64)
        assert lib.agx_sw_batch_cigars(dev._h, None, agx._ptr(op_off), None, 0) == agx.OK  # the sizing call
        assert np.array_equal(op_off, want[1])
        total = int(op_off[n])
        ops, hits = np.full(total, 0xdeadbeef, np.uint32), np.empty(n, agx.SwHit)
        op_off[:] = 0
        assert lib.agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), agx._ptr(ops), total - 1) == agx.E_ARG
        assert str(total).encode() in lib.agx_last_error()
        assert np.array_equal(op_off, want[1]) and np.all(ops == 0xdeadbeef)  # op_off filled, ops untouched
        assert lib.agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), agx._ptr(ops), total) == agx.OK
        _same((hits, op_off, ops), want, "real call")
        assert dev.cigar_info().n_chunks == 1  # all three calls were answered from one computation
        _same((dev.hits(), op_off, ops), want, "hits() beside cigars()")
        assert np.array_equal(dev.scores(), want[0]["score"])
        dev.launch()
        _same(dev.cigars(), want, "relaunch")
        plain.launch()
        assert lib.agx_sw_batch_cigars(plain._h, None, agx._ptr(op_off), None, 0) == agx.E_ARG
        info = agx.SwCigarInfo()
        assert lib.agx_sw_batch_cigar_info(plain._h, C.byref(info)) == agx.E_ARG
        assert lib.agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(np.empty(n, agx.SwStat))) == agx.E_ARG
        assert lib.agx_sw_batch_zdrop_stops(dev._h, agx._ptr(np.empty(n, np.int32))) == agx.E_ARG
        for f in FIELDS:
            assert np.array_equal(plain.hits()[f], want[0][f]), f
    finally:
        dev.close()
        plain.close()
    texts = dcr.strings(want[1], want[2])
    perm = np.random.default_rng(1945).permutation(n)
    shuffled = synth.sw_from_seqs([s for p in perm for s in (b.seq(2 * int(p)), b.seq(2 * int(p) + 1))])
    hits, op_off, ops = ctx.sw_align_band_diag_dual_cigar(shuffled, mode, w, cs[perm], S_MM2)
    assert dcr.strings(op_off, ops) == [texts[int(p)] for p in perm]
    for f in FIELDS:
        assert np.array_equal(hits[f], want[0][f][perm]), f
    got = []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        half = synth.sw_from_seqs([b.seq(k) for k in range(2 * lo, 2 * hi)])
        hits, op_off, ops = ctx.sw_align_band_diag_dual_cigar(half, mode, w, cs[lo:hi], S_MM2)
        got += dcr.strings(op_off, ops)
        for f in FIELDS:
            assert np.array_equal(hits[f], want[0][f][lo:hi]), f
    assert got == texts
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_align_band_diag_dual_cigar(synth.sw_from_seqs([b"ACGT", b"ACGT", b"AC\x00T", b"ACGT"]), FIT, 2, 0, S_MM2)
    assert e.value.code == agx.E_SYMBOL and "pair 1" in str(e.value)
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_align_band_diag_dual_cigar(b, mode, w, cs, None)
    assert e.value.code == agx.E_ARG


def test_two_threads_with_a_context_each(ctx):
    """The threading contract: callers on contexts of their own run at once and each gets its own answer (the begin pass creates,
    launches and destroys an internal two-piece batch, and every chunk takes and returns blocks of its context's pool)."""
    b, cs = _reads(FIT)
    want = {m: dcr.expected(b, m, 24, cs) for m in (LOCAL, FIT)}
    got, errors = {}, []

    def body(mode):
        try:
            with agx.Context(0) as c:
                for _ in range(3):
                    got[mode] = c.sw_align_band_diag_dual_cigar(b, mode, 24, cs, S_MM2)
        except Exception as e:  # noqa: BLE001 -- reported below, in the main thread
            errors.append((mode, e))

    threads = [threading.Thread(target=body, args=(m,)) for m in (LOCAL, FIT)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for m in (LOCAL, FIT):
        _same(got[m], want[m], bd.MODE_NAMES[m])


@pytest.mark.parametrize("word,mode,w,c", [("fit", FIT, 24, -40), ("local", LOCAL, 30, -35)])
def test_swalign_prints_what_the_api_returns(ctx, tmp_path, word, mode, w, c):
    exe = os.path.join(ROOT, "accelerating-genomics_amd", "bin", "swAlign")
    rng = np.random.default_rng(1946)
    path = tmp_path / "reads.in"
    lines = []
    for _ in range(6):
        read = _rand(rng, int(rng.integers(100, 300)))
        cut = int(rng.integers(30, 70))
        lines += [read, _rand(rng, 40) + _mutate(rng, read[:cut] + read[cut + 12:]) + _rand(rng, 1500)]
    path.write_bytes(b"%d\n" % len(lines) + b"".join(s + b"\n" for s in lines))
    six = [str(v) for v in S_MM2]
    out = subprocess.run([exe, str(path), "%s+dualbandcigar=%d@%d" % (word, w, c)] + six, capture_output=True, timeout=300, check=True).stdout
    _, b, _ = agx.read_sw_text(str(path), 65536)
    assert b.n_pairs == 6
    hits, op_off, ops = ctx.sw_align_band_diag_dual_cigar(b, mode, w, c, S_MM2)
    text = [agx.cigar_string(ops[int(op_off[p]):int(op_off[p + 1])]) for p in range(b.n_pairs)]
    assert out == b"".join(b"%d %d %d %d %d %s\n" % (tuple(int(v) for v in h) + (t.encode(),)) for h, t in zip(hits, text))
    assert dcr.path_checks(b, w, c, hits, op_off, ops) == -1 and np.all(hits["score"] > 50)
    # the lines of "+dualband=W@D" with the CIGAR appended
    plain = subprocess.run([exe, str(path), "%s+dualband=%d@%d" % (word, w, c)] + six, capture_output=True, timeout=300, check=True).stdout
    assert [ln.rsplit(b" ", 1)[0] for ln in out.splitlines()] == plain.splitlines()
    good = "%s+dualbandcigar=8@0" % word
    for argv in ([good], [good] + six[:5], [good] + six + ["1"], [good, "2", "-4", "-4", "-2", "-24", "x"], [good + "+cigar"] + six,
                 [good + "+stats"] + six, ["extend+dualbandcigar=8@0+zdrop=100"] + six, ["%s+dualbandcigar=8" % word] + six,
                 ["%s+dualbandcigar=x@0" % word] + six, ["%s+cigar+dualband=8@0" % word] + six, ["%s+bandcigar=8@0" % word] + six):
        bad = subprocess.run([exe, str(path)] + argv, capture_output=True, timeout=60)
        assert bad.returncode != 0 and b"Usage" in bad.stderr and not bad.stdout, argv


# ---- 10. a seeded sweep

SWEEP_SEED, SWEEP_CASES = 1951, 40


def _sweep_case(k):
    """Case k: mode, six scores, band, alphabet and centre per pair drawn with the generators of tests/sw_fuzz_cases.py, lengths up
    to 300 -> (batch, mode, w, diag, six)"""
    rng = np.random.default_rng([SWEEP_SEED, k])
    mode = bd.MODES[k % 5]
    sym = list(fz.ALPHABETS.values())[(k // 5) % len(fz.ALPHABETS)]
    s = fz._scoring(rng, fz.SCORING_KINDS[k % len(fz.SCORING_KINDS)])
    six, _ = fz._second_piece(rng, s, *fz.DUAL_KINDS[k % len(fz.DUAL_KINDS)])
    w = int(fz.WIDTHS[(7 * k) % len(fz.WIDTHS)])
    tags = {"lengths": set(), "related": set()}
    seqs, diag = [], []
    for _ in range(24):
        a = fz._letters(rng, sym, int(rng.integers(0 if rng.random() < 0.05 else 1, 240)))
        if rng.random() < 0.7 and len(a) > 2:
            t, shift = fz._related(rng, sym, a, tags, [])
        else:
            t, shift = fz._letters(rng, sym, int(rng.integers(0 if rng.random() < 0.05 else 1, 300))), 0
        if rng.random() < 0.5:
            a, t, shift = t, a, -shift
        a, t = fz._fit_to_band(mode, a[:300], t[:300], 2 * w)
        lo, hi = fz.centres(mode, len(a), len(t), w)
        c = min(max(-shift + int(rng.integers(-min(w, 3), min(w, 3) + 1)), lo), hi) if rng.random() < 0.6 else int(rng.integers(lo, hi + 1))
        seqs += [a, t]
        diag.append(c)
    return synth.sw_from_seqs(seqs), mode, w, np.array(diag, np.int32), six


@pytest.mark.parametrize("k", range(SWEEP_CASES))
def test_seeded_sweep(ctx, k):
    b, mode, w, diag, six = _sweep_case(k)
    _check(ctx, b, mode, w, diag, six, one_shot=k % 4 == 0)
