"""CIGARs on the device (agx_sw_batch_create_align_cigar / agx_sw_batch_cigars / agx_sw_align_cigar): every comparison is
exact -- all five hit fields, op_off and every operation of every pair -- against the existing by-definition checkers for
score and span and tests/sw_cigar_ref.py for the alignment."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_cigar_cases as cases
from tests import sw_cigar_ref as ref
from tests import sw_stats_ref as stats_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT_FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
MODES = pytest.mark.parametrize("mode", ref.MODES, ids=[ref.MODE_NAMES[m] for m in ref.MODES])
T = cases.T


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


def _same_hits(got, want, what=""):
    for f in HIT_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _same_ops(got_off, got_ops, want_off, want_ops, what=""):
    assert got_off.dtype == np.uint64 and got_ops.dtype == np.uint32
    bad = np.nonzero(got_off != want_off)[0]
    if bad.size == 0 and np.array_equal(got_ops, want_ops):
        return
    g, w = ref.strings(got_off, got_ops), ref.strings(want_off, want_ops)
    p = next(k for k in range(len(w)) if g[k] != w[k])
    raise AssertionError("%s: pair %d: got %s, want %s" % (what, p, g[p], w[p]))


def _batch(ctx, b, mode, scoring=None, matrix=None):
    dev = ctx.sw_batch(b, scoring=scoring, matrix=matrix, mode=mode, cigar=True)
    try:
        dev.launch()
        hits, op_off, ops = dev.cigars()
        assert np.array_equal(dev.scores(), hits["score"])  # agx_sw_batch_scores returns the mode's score
        _same_hits(dev.hits(), hits, "agx_sw_batch_hits of a cigar batch")
        return hits, op_off, ops.copy(), dev.cigar_info()
    finally:
        dev.close()


def _check(ctx, name, b, mode, scoring=None, matrix=None, oneshot=False, plain=False):
    want_hits, want_off, want_ops = cases.expected(name, b, mode, scoring, matrix)
    what = "%s %s %s" % (name, ref.MODE_NAMES[mode], scoring)
    hits, op_off, ops, info = _batch(ctx, b, mode, scoring, matrix)
    _same_hits(hits, want_hits, what + " batch")
    _same_ops(op_off, ops, want_off, want_ops, what + " batch")
    ca, cb = ref.spans(want_hits)
    assert info.n_traced == int(np.count_nonzero((ca > 0) & (cb > 0))) and info.trace_cells == int((ca * cb).sum())
    if oneshot:
        hits, op_off, ops = ctx.sw_align_cigar(b, scoring, mode, matrix)
        _same_hits(hits, want_hits, what + " one-shot")
        _same_ops(op_off, ops, want_off, want_ops, what + " one-shot")
    if plain:  # ... and the hits are a plain SPANS batch's, field for field
        if matrix is not None:
            _same_hits(hits, ctx.sw_align(b, agx.SW_ALIGN_SPANS, mode=mode, matrix=matrix), what + " against a plain SPANS batch")
        else:
            _same_hits(hits, ctx.sw_align(b, agx.SW_ALIGN_SPANS, scoring, mode=mode), what + " against a plain SPANS batch")
    return want_hits, want_off, want_ops, info


@MODES
def test_every_length_pair_up_to_40(ctx, mode):
    """len(a) x len(b) over 0..40 x 0..40 (the batch of tests/test_sw_modes_gpu.py): empty sides, fewer rows than the skew,
    every narrow class.  Batch and one-shot; the hits also against a plain SPANS batch."""
    _check(ctx, "up_to_40", cases.shared("up_to_40", cases.up_to_40), mode, oneshot=True, plain=True)


@pytest.mark.parametrize("mode", [ref.LOCAL, ref.GLOBAL, ref.FIT, ref.EXTEND_QUERY], ids=["local", "global", "fit", "extend-query"])
def test_lane_edges(ctx, mode):
    """Queries either side of one, two and 64 lanes of a class (38 .. 64 T, T the widest traced class) against targets of
    1..60 rows: a column's nibble at the end of a dword, of a lane, in the group's only lane and in its last one."""
    _check(ctx, "lane_edges", cases.shared("lane_edges", cases.lane_edges), mode)


@MODES
@pytest.mark.parametrize("scoring", cases.TIE_SCORINGS, ids=str)
def test_tie_heavy_inputs(ctx, mode, scoring):
    """600 pairs of lengths 1..199 (homopolymers, tandem repeats, an indel inside a repeat, random) under four scorings: where
    "diagonal, then D, then I; open before extend" and gap_open = 0 can go wrong."""
    _check(ctx, "tie_heavy", cases.shared("tie_heavy", cases.tie_heavy), mode, scoring)


@MODES
@pytest.mark.parametrize("which", ["blosum62", "four_symbols"])
def test_matrix(ctx, mode, which):
    """Under BLOSUM62 with gaps -11 / -1 (protein letters) and under a 4-symbol matrix with zero and positive off-diagonal
    entries: the 0..40 x 0..40 batch and 200 pairs of lengths 1..300."""
    m = cases.shared(which, getattr(cases, which))
    if which == "blosum62":
        small = cases.shared("up_to_40_protein", lambda: cases.up_to_40(np.frombuffer(cases.AMINO, np.uint8), 38))
        big = cases.shared("protein_300", lambda: cases.protein_pairs(200, 1, 300, 41))
    else:
        small = cases.shared("up_to_40", cases.up_to_40)
        big = cases.shared("dna_300", lambda: synth.sw_pairs(200, 1, 300, seed=42, related_frac=0.5, newline=False))
    _check(ctx, "small_" + which, small, mode, matrix=m, oneshot=True, plain=True)
    _check(ctx, "big_" + which, big, mode, matrix=m)


def test_matrix_symbol_outside_the_alphabet(ctx):
    b = synth.sw_from_seqs([b"ACGT", b"ACGT", b"ACNT", b"ACGT"])
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_batch(b, matrix=cases.four_symbols(), mode=agx.SW_MODE_GLOBAL, cigar=True)
    assert e.value.code == agx.E_SYMBOL
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_align_cigar(b, mode=agx.SW_MODE_LOCAL, matrix=cases.four_symbols())
    assert e.value.code == agx.E_SYMBOL


@pytest.mark.parametrize("mode", [ref.GLOBAL, ref.FIT, ref.LOCAL], ids=["global", "fit", "local"])
def test_long_targets(ctx, mode):
    """150 against 20 000 with a diverged copy implanted, and 64 T against 3 000: row addressing, 64-lane groups, the walk's
    tails."""
    b = cases.shared("long_targets", cases.long_targets)
    assert list(b.len) == [150, 20000, 64 * T, 3000]
    _check(ctx, "long_targets", b, mode)


def test_chunking():
    """Budgets of 1 byte, 256 KiB and the default give identical output; one chunk per traced pair under 1 byte, several
    under 256 KiB, one under the default; the block held never passes max(budget, the largest single pair)."""
    b = cases.shared("tie_heavy", cases.tie_heavy)
    mode, scoring = ref.FIT, (1, -2, 0, -1)
    want_hits, want_off, want_ops = cases.expected("tie_heavy", b, mode, scoring)
    infos = {}
    for budget in (1, 256 << 10, None):
        with agx.Context(0) as c:
            if budget is not None:
                c.set_option(agx.OPT_SW_TRACE_BYTES, budget)
            hits, op_off, ops, info = _batch(c, b, mode, scoring)
        _same_hits(hits, want_hits, "budget %s" % budget)
        _same_ops(op_off, ops, want_off, want_ops, "budget %s" % budget)
        infos[budget] = info
    one, some, default = infos[1], infos[256 << 10], infos[None]
    assert one.n_traced == some.n_traced == default.n_traced > 0
    assert one.n_chunks == one.n_traced and 1 < some.n_chunks < one.n_chunks and default.n_chunks == 1
    largest = one.trace_bytes_peak  # a chunk of one pair holds exactly that pair
    assert 0 < largest <= (256 << 10)
    assert some.trace_bytes_peak <= max(256 << 10, largest) and default.trace_bytes_peak <= max(1 << 30, largest)
    with agx.Context(0) as c:
        for bad in (0, -5):
            with pytest.raises(agx.AgxError) as e:
                c.set_option(agx.OPT_SW_TRACE_BYTES, bad)
            assert e.value.code == agx.E_ARG


def test_lifecycle(ctx):
    """Sizing call then the real call; a short ops_cap; relaunch; the wrong kinds of batch."""
    b = cases.shared("tie_heavy", cases.tie_heavy)
    mode, scoring = ref.LOCAL, (1, -1, -3, -1)
    want_hits, want_off, want_ops = cases.expected("tie_heavy", b, mode, scoring)
    n, lib = b.n_pairs, agx.lib()
    dev = ctx.sw_batch(b, scoring=scoring, mode=mode, cigar=True)
    spans = ctx.sw_batch(b, scoring=scoring, align=agx.SW_ALIGN_SPANS, mode=mode)
    stats = ctx.sw_batch(b, scoring=scoring, mode=mode, stats=True)
    try:
        dev.launch()
        op_off = np.zeros(n + 1, np.uint64)
        assert lib.agx_sw_batch_cigars(dev._h, None, agx._ptr(op_off), None, 0) == agx.OK  # the sizing call
        assert np.array_equal(op_off, want_off)
        total = int(op_off[n])
        ops, hits = np.full(total, 0xdeadbeef, np.uint32), np.empty(n, agx.SwHit)
        op_off[:] = 0
        assert lib.agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), agx._ptr(ops), total - 1) == agx.E_ARG
        assert str(total).encode() in lib.agx_last_error()
        assert np.array_equal(op_off, want_off) and np.all(ops == 0xdeadbeef)  # op_off filled, ops untouched
        assert lib.agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), agx._ptr(ops), total) == agx.OK
        _same_hits(hits, want_hits, "real call")
        _same_ops(op_off, ops, want_off, want_ops, "real call")
        dev.launch()
        h2, o2, p2 = dev.cigars()
        _same_hits(h2, want_hits, "relaunch")
        _same_ops(o2, p2, want_off, want_ops, "relaunch")
        spans.launch()
        stats.launch()
        for other in (spans, stats):
            assert lib.agx_sw_batch_cigars(other._h, None, agx._ptr(op_off), None, 0) == agx.E_ARG
        assert lib.agx_sw_batch_stats(dev._h, None, agx._ptr(np.empty(n, agx.SwStat))) == agx.E_ARG
        _same_hits(spans.hits(), want_hits, "a SPANS batch beside it")
    finally:
        dev.close()
        spans.close()
        stats.close()


@MODES
@pytest.mark.parametrize("scoring", [(1, -1, -3, -1), (1, -2, 0, -1)], ids=str)
def test_against_the_stats(ctx, mode, scoring):
    """The CIGAR is one optimal alignment of the span, the stats describe the one with the most matches: sum('=') <= matches,
    and where they are equal sum('=' + 'X') <= pairs."""
    b = cases.shared("tie_heavy", cases.tie_heavy)
    hits, op_off, ops, _ = _batch(ctx, b, mode, scoring)
    shits, stats = ctx.sw_align_stats(b, scoring, mode)
    _same_hits(hits, shits, "cigar batch against stats batch")
    pair = np.repeat(np.arange(b.n_pairs), np.diff(op_off).astype(np.int64))
    ln, op = (ops >> 4).astype(np.int64), ops & 15
    eq = np.bincount(pair, weights=ln * (op == agx.CIGAR_EQ), minlength=b.n_pairs).astype(np.int64)
    diag = np.bincount(pair, weights=ln * ((op == agx.CIGAR_EQ) | (op == agx.CIGAR_DIFF)), minlength=b.n_pairs).astype(np.int64)
    assert np.all(eq <= stats["matches"])
    same = eq == stats["matches"]
    assert np.all(diag[same] <= stats["pairs"][same])


def _write_pairs(path, b):
    with open(path, "wb") as f:
        f.write(b"%d\n" % (2 * b.n_pairs))
        for k in range(2 * b.n_pairs):
            f.write(b.bases[int(b.off[k]):int(b.off[k]) + int(b.len[k])].tobytes() + b"\n")


@pytest.mark.parametrize("word,mode,with_matrix", [("local", ref.LOCAL, False), ("global", ref.GLOBAL, False), ("fit", ref.FIT, True),
                                                   ("extend", ref.EXTEND, True)])
def test_swalign_cigar_suffix(tmp_path, word, mode, with_matrix):
    """swAlign <file> <mode>+cigar on the 0..40 x 0..40 batch, with and without the matrix file: the first five columns are byte
    for byte what swAlign <file> <mode> prints, the last is the checker's string; <mode>+stats prints what it printed."""
    exe = os.path.join(ROOT, "accelerating-genomics_amd", "bin", "swAlign")
    path = str(tmp_path / "pairs.in")
    if with_matrix:
        b = cases.shared("up_to_40_protein", lambda: cases.up_to_40(np.frombuffer(cases.AMINO, np.uint8), 38))
        extra = [os.path.join(ROOT, "tests", "golden", "blosum62.mat")]
    else:
        b = cases.shared("up_to_40", cases.up_to_40)
        extra = []
    _write_pairs(path, b)
    run = lambda w: subprocess.run([exe, path, w] + extra, capture_output=True, timeout=300, check=True).stdout.splitlines()
    plain, got, with_stats = run(word), run(word + "+cigar"), run(word + "+stats")
    assert len(plain) == len(got) == len(with_stats) == b.n_pairs
    if with_matrix:  # the command line strips the line ends under a matrix
        _, want_off, want_ops = cases.expected("small_blosum62", b, mode, None, cases.shared("blosum62", cases.blosum62))
        _, smax, _ = stats_ref.expected(b, mode, matrix=cases.shared("blosum62", cases.blosum62))
    else:  # ... and keeps them as symbols otherwise: the batch as the file says it
        _, fb, _ = agx.read_sw_text(path)
        _, want_off, want_ops = ref.expected(fb, mode)
        _, smax, _ = stats_ref.expected(fb, mode)
    want = ref.strings(want_off, want_ops)
    for p in range(b.n_pairs):
        assert got[p] == plain[p] + b" " + want[p].encode(), p
        assert with_stats[p] == plain[p] + b" %d %d" % (smax[p]["matches"], smax[p]["pairs"]), p
    for bad in (word + "+stats+cigar", word + "+cigar+stats"):
        r = subprocess.run([exe, path, bad] + extra, capture_output=True, timeout=60)
        assert r.returncode == 1 and b"Usage" in r.stderr


# ---- every byte


def test_every_byte_but_zero_is_a_symbol(ctx):
    """The twin of tests/test_sw_gpu.py::test_all_byte_values_are_symbols for the CIGARs: cases of the seeded sweep
    (tests/sw_fuzz_cases.py, family "align_cigar") drawn over 0x01 .. 0xff, one per mode -- 0x01, 0x7f / 0x80 and 0xff among them, bytes that
    no other test of this file feeds in -- held to everything tests/test_fuzz_align_gpu.py holds a case to, exactly."""
    from tests import sw_fuzz_cases as fc

    cases = fc.byte_cases("align_cigar")
    assert {c.kw["mode"] for c in cases} == set(fc.MODES_OF.get("align_cigar", fc.MODES))
    for case in cases:
        seen = set(case.batch.bases.tolist())
        assert 0 not in seen and {0x01, 0x7f, 0x80, 0xff} <= seen
        assert fc.check_case(ctx, case) >= 4
