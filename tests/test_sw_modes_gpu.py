"""Alignment modes on the device (agx_sw_batch_create_align_mode / agx_sw_align_mode: global, fit, extension): every
comparison is exact, all five fields of every pair, against the by-definition checker of tests/sw_modes_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_modes_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
MODES = pytest.mark.parametrize("mode", ref.MODES, ids=[ref.MODE_NAMES[m] for m in ref.MODES])


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


def _same(got, want, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _ends_of(spans):
    e = spans.copy()
    e["a_begin"] = -1
    e["b_begin"] = -1
    return e


def _batch(ctx, b, mode, what, scoring=None, relaunch=False):
    dev = ctx.sw_batch(b, scoring=scoring, align=what, mode=mode)
    try:
        dev.launch()
        got = dev.hits()
        assert np.array_equal(dev.scores(), got["score"])  # agx_sw_batch_scores returns the mode's score
        if relaunch:
            dev.launch()
            _same(dev.hits(), got, "relaunch")
        return got
    finally:
        dev.close()


def _check(ctx, b, mode, scoring=None, everything=False):
    """SPANS through a batch and ENDS through the one-shot against the checker; everything: the other two ways as well."""
    want = ref.align(b, mode, ref.SPANS, scoring)
    name = ref.MODE_NAMES[mode]
    _same(_batch(ctx, b, mode, agx.SW_ALIGN_SPANS, scoring), want, name + " SPANS batch")
    _same(ctx.sw_align(b, agx.SW_ALIGN_ENDS, scoring, mode=mode), _ends_of(want), name + " ENDS one-shot")
    if everything:
        _same(_batch(ctx, b, mode, agx.SW_ALIGN_ENDS, scoring), _ends_of(want), name + " ENDS batch")
        _same(ctx.sw_align(b, agx.SW_ALIGN_SPANS, scoring, mode=mode), want, name + " SPANS one-shot")
    return want


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


_cache = {}


def _shared(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _up_to_40():
    rng = np.random.default_rng(31)
    seqs = []
    for la in range(41):
        for lb in range(41):
            a = _rand(rng, la)
            if (la + lb) % 2:
                t = _rand(rng, lb)
            else:  # b from copies of a: the maximum is reached many times
                t = (a * (lb // max(la, 1) + 1))[:lb]
            seqs += [a, t]
    return synth.sw_from_seqs(seqs)


@MODES
def test_every_length_pair_up_to_40(ctx, mode):
    """len(a) x len(b) over 0..40 x 0..40: empty sides, targets shorter than the lanes of a group (fewer rows than the
    skew), every small class; half of the pairs related.  SPANS and ENDS, batch and one-shot."""
    _check(ctx, _shared("up_to_40", _up_to_40), mode, everything=True)


def _last_column():
    rng = np.random.default_rng(33)
    seqs = []
    for la in (38, 39, 40, 41, 76, 77, 150, 151, 152, 300, 512):
        a = _rand(rng, la)
        for lb in range(1, 61):
            kind = lb % 3
            if kind == 0:
                t = _rand(rng, lb)
            elif kind == 1:  # the end of a: the last column carries the maximum in the last rows
                t = a[-lb:]
            else:  # the end of a, then a tail
                t = (a[-(lb - lb // 3):] + _rand(rng, lb))[:lb]
            seqs += [a, t]
    return synth.sw_from_seqs(seqs)


@MODES
def test_last_column_in_every_lane_position(ctx, mode):
    """The query's last column at the end of a lane, at its start, in the group's only lane and in its last one, against
    targets of 1..60 rows (fewer and more rows than lanes)."""
    _check(ctx, _shared("last_column", _last_column), mode)


def _tie_heavy():
    rng = np.random.default_rng(32)
    seqs = []
    for k in range(600):
        la, lb = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        kind = k % 5
        if kind == 0:  # homopolymers: every tie at once
            a, t = b"A" * la, b"A" * lb
        elif kind == 1:  # short tandem repeats
            unit = _rand(rng, int(rng.integers(2, 5)))
            a, t = (unit * la)[:la], (unit * lb)[:lb]
        elif kind == 2:  # the same motif twice in b
            m = _rand(rng, min(la, 30))
            a, t = m, _rand(rng, 5) + m + _rand(rng, int(rng.integers(0, 40))) + m + _rand(rng, 3)
        elif kind == 3:  # ... twice in a
            m = _rand(rng, min(lb, 30))
            a, t = _rand(rng, 5) + m + _rand(rng, int(rng.integers(0, 40))) + m + _rand(rng, 3), m
        else:  # a homopolymer against a repeat that holds its letter
            a, t = b"C" * la, (b"ACC" * lb)[:lb]
        seqs += [a, t]
    return synth.sw_from_seqs(seqs)


@MODES
def test_tie_heavy_inputs(ctx, mode):
    _check(ctx, _shared("tie_heavy", _tie_heavy), mode)


@MODES
@pytest.mark.parametrize("scoring", [(2, -3, -5, -2), (5, -4, -10, -1), (1, 0, 0, 0), (3, -2, 0, -1), (12, -116, -1000, -1000)], ids=str)
def test_runtime_scoring(ctx, mode, scoring):
    """(1, 0, 0, 0): free mismatches and gaps -- padding cells hold as much as the real ones they derive from.
    (12, -116, -1000, -1000): the extremes the header allows -- minus infinity and the rising offset do not wrap."""
    b = _shared("scoring", lambda: synth.sw_pairs(1000, 1, 200, seed=34, related_frac=0.5))
    _check(ctx, b, mode, scoring)


def _limits():
    rng = np.random.default_rng(38)
    a = _rand(rng, agx.SW_ALIGN_MAX_QUERY_LEN)
    return synth.sw_from_seqs([a, a[1000:1100], a, _rand(rng, 100) + a[:2000] + _rand(rng, 30) + a[2000:] + _rand(rng, 3310)])


@MODES
def test_longest_query(ctx, mode):
    """len(a) = 2560 (64 lanes x 40 columns) against a target of 100 and one of 6 000."""
    b = _shared("limits", _limits)
    assert list(b.len) == [2560, 100, 2560, 6000]
    _check(ctx, b, mode)


@MODES
def test_longest_target_at_the_largest_gap_costs(ctx, mode):
    """lb = 65535, la = 64 under (1, -1, -1000, -1000): the boundary column reaches -65 536 000."""
    def make():
        rng = np.random.default_rng(39)
        a = _rand(rng, 64)
        return synth.sw_from_seqs([a, _rand(rng, 30000) + a + _rand(rng, 65535 - 30064)])

    b = _shared("longest_target", make)
    assert list(b.len) == [64, 65535]
    _check(ctx, b, mode, (1, -1, -1000, -1000))


def _mixed_reads_and_contigs():
    """8 192 pairs, every length in 32..512: queries are reads of 32..150 with one in ten a contig of 300..512, targets
    32..512, a third of the targets cut from copies of their query."""
    rng = np.random.default_rng(4)
    seqs = []
    for k in range(8192):
        la = int(rng.integers(300, 513)) if rng.random() < 0.1 else int(rng.integers(32, 151))
        lb = int(rng.integers(32, 513))
        a = _rand(rng, la)
        t = (a * 17)[int(rng.integers(0, la)):][:lb] if k % 3 == 0 else _rand(rng, lb)
        seqs += [a, t]
    return synth.sw_from_seqs(seqs)


@MODES
def test_mixed_lengths_several_launches(ctx, mode):
    """Mixed lengths 32..512, 8 192 pairs, more than one launch (the fan-out over streams), all modes against the checker.
    The planner keeps about one column class per 4 096 wavefronts: 8 192 pairs drawn evenly from 32..512 plan to ONE launch
    (about 2 600 wavefronts), whatever the mode.  A mix of reads and contigs within the same range keeps several classes --
    the narrow class of the reads cannot span the contigs -- so that batch carries the assertion; the even mix is checked too."""
    b = _shared("mixed", _mixed_reads_and_contigs)
    assert b.n_pairs == 8192 and int(b.len.min()) >= 32 and int(b.len.max()) <= 512
    dev = ctx.sw_batch(b, align=agx.SW_ALIGN_ENDS, mode=mode)
    try:
        assert dev.info().n_launches > 1
    finally:
        dev.close()
    _check(ctx, b, mode)
    _check(ctx, _shared("mixed_even", lambda: synth.sw_pairs(8192, 32, 512, seed=4, related_frac=0.3, newline=False)), mode)


def test_local_through_the_new_entry_point_and_relaunch(ctx):
    b = synth.sw_pairs(3000, 1, 300, seed=37, related_frac=0.5)
    for what in (agx.SW_ALIGN_ENDS, agx.SW_ALIGN_SPANS):
        want = ctx.sw_align(b, what)  # agx_sw_align
        got = np.empty(b.n_pairs, agx.SwHit)
        rc = agx.lib().agx_sw_align_mode(ctx._h, None, agx.SW_MODE_LOCAL, what, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, agx._ptr(got))
        assert rc == agx.OK
        _same(got, want, "LOCAL")
        h = C.c_void_p()
        assert agx.lib().agx_sw_batch_create_align_mode(ctx._h, None, agx.SW_MODE_LOCAL, what, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h)) == agx.OK
        try:
            for _ in range(2):
                assert agx.lib().agx_sw_batch_launch(h) == agx.OK
                assert agx.lib().agx_sw_batch_hits(h, agx._ptr(got)) == agx.OK
                _same(got, want, "LOCAL batch")
        finally:
            agx.lib().agx_sw_batch_destroy(h)
    for mode in ref.MODES:  # a resident batch relaunches to the same hits
        _batch(ctx, b, mode, agx.SW_ALIGN_SPANS, relaunch=True)


@pytest.mark.parametrize("word,mode", [("global", ref.GLOBAL), ("fit", ref.FIT)])
def test_swalign_prints_what_the_api_returns(ctx, word, mode):
    path = os.path.join(ROOT, "tests", "golden", "sw_mixed.in")
    exe = os.path.join(ROOT, "accelerating-genomics_amd", "bin", "swAlign")
    out = subprocess.run([exe, path, word], capture_output=True, timeout=300, check=True).stdout
    _, b, _ = agx.read_sw_text(path)
    hits = ctx.sw_align(b, agx.SW_ALIGN_SPANS, mode=mode)
    want = b"".join(b"%d %d %d %d %d\n" % tuple(int(v) for v in h) for h in hits)
    assert out == want and b.n_pairs > 0
    _same(hits, ref.align(b, mode, ref.SPANS), word)
    bad = subprocess.run([exe, path, "sideways"], capture_output=True, timeout=60)
    assert bad.returncode != 0 and b"Usage" in bad.stderr and not bad.stdout


# ---- every byte


def test_every_byte_but_zero_is_a_symbol(ctx):
    """The twin of tests/test_sw_gpu.py::test_all_byte_values_are_symbols for the alignment modes: cases of the seeded sweep
    (tests/sw_fuzz_cases.py, family "align_mode") drawn over 0x01 .. 0xff, one per mode -- 0x01, 0x7f / 0x80 and 0xff among them, bytes that
    no other test of this file feeds in -- held to everything tests/test_fuzz_align_gpu.py holds a case to, exactly."""
    from tests import sw_fuzz_cases as fc

    cases = fc.byte_cases("align_mode")
    assert {c.kw["mode"] for c in cases} == set(fc.MODES_OF.get("align_mode", fc.MODES))
    for case in cases:
        seen = set(case.batch.bases.tolist())
        assert 0 not in seen and {0x01, 0x7f, 0x80, 0xff} <= seen
        assert fc.check_case(ctx, case) >= 4
