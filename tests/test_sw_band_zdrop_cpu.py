"""Z-drop termination of banded extension (include/agx.h, "Z-drop for banded extension") without a GPU: the checker itself
(tests/sw_band_zdrop_ref.py) against the band-diag checker and on properties of the rule; the conditions the GPU tests' inputs
must meet; the new C-ABI on plan-only batches and its argument errors; the kernels' resources as the code objects state them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_diag_ref as bd
from tests import sw_band_zdrop_ref as zd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
HAND = [b"AAAATTTTTTTT", b"AAAACCCCCCCC"]
DNA = (2, -4, -4, -2)


def _same(got, want, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _differ(x, y):
    return np.any([x[f] != y[f] for f in FIELDS], axis=0)


# ---- 1. the checker


@pytest.mark.parametrize("what", [zd.ENDS, zd.SPANS], ids=["ends", "spans"])
@pytest.mark.parametrize("scoring", [None, DNA, (1, 0, 0, 0)], ids=str)
def test_checker_at_zdrop_max_equals_the_band_diag_checker(what, scoring):
    """Random batches, empty sides and per-pair centres included: a z-drop that never fires is EXTEND inside the band."""
    rng = np.random.default_rng(301)
    seqs = zd.three_kinds(rng, 90) + zd.long_gaps(rng, 40) + [b"", b"ACGT", b"ACGT", b"", b"", b""]
    for _ in range(60):
        seqs += [zd.rand(rng, int(rng.integers(0, 50))), zd.rand(rng, int(rng.integers(0, 50)))]
    b = synth.sw_from_seqs(seqs)
    for w in (0, 3, 8, 40):
        diag = rng.integers(-w, w + 1, size=b.n_pairs).astype(np.int32)
        hits, stops = zd.align(b, w, zd.ZDROP_MAX, diag, what, scoring)
        _same(hits, bd.align(b, bd.EXTEND, w, diag, what, scoring), "w=%d" % w)
        assert np.all(stops == -1)


def test_the_case_worked_by_hand():
    """(1, -1, -3, -1), w = 4, c = 0: four matches, then mismatches only; row 4 + k has R = 4 - k on the main diagonal."""
    for z in range(0, 12):
        assert zd.align_seqs(HAND, 4, z) == [((4, 0, 3, 0, 3), 4 + z if z <= 7 else -1)], z
    assert zd.align_seqs(HAND, 4, zd.ZDROP_MAX) == [((4, 0, 3, 0, 3), -1)]
    assert zd.align_seqs(HAND, 4, 3, what=zd.ENDS) == [((4, -1, 3, -1, 3), 7)]
    # empty sides and a pair of score 0 that never drops below zdrop
    assert zd.align_seqs([b"", b"ACGT", b"ACGT", b""], 4, 0) == [((0, -1, -1, -1, -1), -1)] * 2
    assert zd.align_seqs([b"A", b"C"], 4, 1) == [((0, -1, -1, -1, -1), -1)]
    assert zd.align_seqs([b"A", b"C"], 4, 0) == [((0, -1, -1, -1, -1), 0)]  # row 1: R = -1, 0 - (-1) > 0
    # the diagonal term under (2, -4, -4, -2): B = 16 at (8, 8), then three inserted rows.  Row 10 has R = 8 first in column 8 (the
    # gap of two, 16 - 4 - 4): the drop 8 exceeds zdrop = 5 but not 5 + 2 * |2 - 0|; row 11 has R = 6 in column 8, 10 <= 5 + 6; the
    # second stretch then climbs to 16 - 10 + 24.  Without the term row 10 terminates.
    a, t = b"ACGTACGT" + b"GGCCTTAAGGCC", b"ACGTACGT" + b"TTT" + b"GGCCTTAAGGCC"
    assert zd.align_seqs([a, t], 6, 5, scoring=DNA) == [((30, 0, 19, 0, 22), -1)]
    assert zd.align_seqs([a, t], 6, 5, scoring=DNA, term=False) == [((16, 0, 7, 0, 7), 9)]


def test_score_never_rises_and_stop_never_moves_later_as_zdrop_falls():
    rng = np.random.default_rng(302)
    b = synth.sw_from_seqs(zd.three_kinds(rng, 120) + zd.long_gaps(rng, 60))
    for scoring in (None, DNA):
        prev_h, prev_s = zd.align(b, 16, zd.ZDROP_MAX, scoring=scoring)
        fired = 0
        for z in (200, 100, 50, 30, 20, 10, 5, 3, 2, 1, 0):
            h, s = zd.align(b, 16, z, scoring=scoring)
            assert np.all(h["score"] <= prev_h["score"]), z
            later = np.where(s < 0, np.iinfo(np.int32).max, s) > np.where(prev_s < 0, np.iinfo(np.int32).max, prev_s)
            assert not np.any(later), z
            fired += int(np.count_nonzero(s >= 0))
            prev_h, prev_s = h, s
        assert fired > 0 and np.all(prev_s >= 0)  # zdrop = 0 terminates every pair of these (none is a perfect match to its end)


# ---- 2. the conditions on the GPU tests' inputs, from the checker alone


@pytest.mark.parametrize("scoring,zdrop", [(DNA, 20), (zd.REFERENCE_SCORING, 5)], ids=str)
@pytest.mark.parametrize("w", [8, 32])
def test_three_kind_generator_exercises_the_rule(scoring, zdrop, w):
    rng = np.random.default_rng(303)
    b = synth.sw_from_seqs(zd.three_kinds(rng, 300))
    hits, stops = zd.align(b, w, zdrop, scoring=scoring)
    plain = bd.align(b, bd.EXTEND, w, None, bd.SPANS, scoring)
    n = b.n_pairs
    terminated, differ = np.count_nonzero(stops >= 0) / n, np.count_nonzero(_differ(hits, plain)) / n
    print("terminated %.2f, ran through %.2f, another hit %.2f" % (terminated, 1 - terminated, differ))
    assert terminated >= 0.25 and 1 - terminated >= 0.25 and differ >= 0.2


def test_long_gap_generator_exercises_the_diagonal_term():
    rng = np.random.default_rng(304)
    b = synth.sw_from_seqs(zd.long_gaps(rng, 300))
    on, s_on = zd.align(b, 40, 20, scoring=DNA)
    off, s_off = zd.align(b, 40, 20, scoring=DNA, term=False)
    frac = np.count_nonzero(_differ(on, off) | (s_on != s_off)) / b.n_pairs
    print("the term changes %.2f of the pairs" % frac)
    assert frac >= 0.2


# ---- 3. the C-ABI on plan-only batches


def _create(b, mode, w, zdrop, diag=None, what=agx.SW_ALIGN_SPANS, cigar=False):
    h = C.c_void_p()
    d = agx._diag(diag, b.n_pairs)
    if cigar:
        rc = agx.lib().agx_sw_batch_create_align_band_zdrop_cigar(None, None, mode, w, agx._ptr(d), zdrop, agx._ptr(b.bases), agx._ptr(b.off),
                                                                  agx._ptr(b.len), b.n_pairs, C.byref(h))
    else:
        rc = agx.lib().agx_sw_batch_create_align_band_zdrop(None, None, mode, what, w, agx._ptr(d), zdrop, agx._ptr(b.bases), agx._ptr(b.off),
                                                            agx._ptr(b.len), b.n_pairs, C.byref(h))
    return rc, h


def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(agx.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    for s in ("agx_sw_batch_create_align_band_zdrop", "agx_sw_align_band_zdrop", "agx_sw_batch_zdrop_stops",
              "agx_sw_batch_create_align_band_zdrop_cigar", "agx_sw_align_band_zdrop_cigar"):
        assert s in agx.SYMBOLS and hasattr(lib, s) and ("int %s(" % s) in hdr, s
    assert "Z-drop for banded extension" in hdr and "#define AGX_SW_ZDROP_MAX 1000000000" in hdr
    assert agx.SW_ZDROP_MAX == zd.ZDROP_MAX == 1000000000


@pytest.mark.parametrize("cigar", [False, True], ids=["hits", "cigar"])
def test_plan_only_batch(cigar):
    rng = np.random.default_rng(305)
    seqs = [b"ACGT" * 20, b"ACGT" * 30, b"", b"ACG", b"ACG", b"", b"", b""]
    for n in (1, 5, 150, 2000, 10000, 65535):
        seqs += [zd.rand(rng, n), zd.rand(rng, max(1, n - 7))]
    b = synth.sw_from_seqs(seqs)
    dev = agx.SwBatch(None, b, mode=agx.SW_MODE_EXTEND, band=64, zdrop=100, cigar=cigar)
    plain = agx.SwBatch(None, b, mode=agx.SW_MODE_EXTEND, band=64, diag=0, cigar=cigar)
    try:
        i, j = dev.info(), plain.info()
        assert i.n_pairs == b.n_pairs and i.cells == b.cells()
        assert (i.n_waves, i.n_launches, i.padded_cells, i.input_bytes) == (j.n_waves, j.n_launches, j.padded_cells, j.input_bytes)
        for call in (dev.launch, dev.hits, dev.scores, dev.zdrop_stops):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_NODEVICE
        hits, stats = np.empty(b.n_pairs, agx.SwHit), np.empty(b.n_pairs, agx.SwStat)
        assert agx.lib().agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(stats)) == agx.E_ARG
        op_off = np.zeros(b.n_pairs + 1, np.uint64)
        assert agx.lib().agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), None, 0) == (agx.E_NODEVICE if cigar else agx.E_ARG)
    finally:
        dev.close()
        plain.close()
    dev = agx.SwBatch(None, synth.sw_from_seqs([b"", b"ACG", b"ACG", b"", b"", b""]), mode=agx.SW_MODE_EXTEND, band=3, diag=[0, 1, -2], zdrop=0,
                      cigar=cigar)
    try:
        assert dev.info().n_pairs == 3 and dev.info().n_waves == 0 and dev.info().cells == 0
    finally:
        dev.close()


@pytest.mark.parametrize("cigar", [False, True], ids=["hits", "cigar"])
def test_every_argument_error(cigar):
    rng = np.random.default_rng(306)
    short = [zd.rand(rng, 10), zd.rand(rng, 12)]
    b = synth.sw_from_seqs(short + short)
    err = agx.lib().agx_last_error

    def refused(rc, h, word):
        return rc == agx.E_ARG and not h.value and word in err()

    for z in (-1, -(1 << 31), agx.SW_ZDROP_MAX + 1, (1 << 31) - 1):
        assert refused(*_create(b, agx.SW_MODE_EXTEND, 4, z, cigar=cigar), b"zdrop"), z
    for z in (0, 1, agx.SW_ZDROP_MAX):
        rc, h = _create(b, agx.SW_MODE_EXTEND, 4, z, cigar=cigar)
        assert rc == agx.OK and h.value, z
        agx.lib().agx_sw_batch_destroy(h)
    for mode in (agx.SW_MODE_LOCAL, agx.SW_MODE_GLOBAL, agx.SW_MODE_FIT, agx.SW_MODE_EXTEND_QUERY, -1, 5):
        assert refused(*_create(b, mode, 4, 10, cigar=cigar), b"mode"), mode
    # a band that misses the origin, on either side, names the pair
    for c in (5, -5):
        rc, h = _create(b, agx.SW_MODE_EXTEND, 4, 10, [0, c], cigar=cigar)
        assert refused(rc, h, b"pair 1:") and b"origin" in err(), c
    for c in (4, -4):
        rc, h = _create(b, agx.SW_MODE_EXTEND, 4, 10, [0, c], cigar=cigar)
        assert rc == agx.OK and h.value
        agx.lib().agx_sw_batch_destroy(h)
    assert refused(*_create(b, agx.SW_MODE_EXTEND, -1, 10, cigar=cigar), b"band")
    rc, h = _create(b, agx.SW_MODE_EXTEND, 1024, 10, cigar=cigar)
    assert rc == agx.E_LIMIT and not h.value
    if not cigar:
        for what in (0, 3):
            assert refused(*_create(b, agx.SW_MODE_EXTEND, 4, 10, what=what), b"what")
    # the message names the entry point that was called
    _create(b, agx.SW_MODE_EXTEND, 4, -1, cigar=cigar)
    assert (b"agx_sw_batch_create_align_band_zdrop_cigar:" if cigar else b"agx_sw_batch_create_align_band_zdrop:") in err()


def test_stops_on_the_other_kinds_of_batch_and_stats_on_this_one():
    rng = np.random.default_rng(307)
    b = synth.sw_from_seqs([zd.rand(rng, 30), zd.rand(rng, 40)] * 3)
    stops = np.empty(b.n_pairs, np.int32)
    others = [dict(), dict(align=agx.SW_ALIGN_SPANS), dict(align=agx.SW_ALIGN_SPANS, mode=agx.SW_MODE_EXTEND), dict(stats=True), dict(cigar=True),
              dict(mode=agx.SW_MODE_EXTEND, band=8), dict(mode=agx.SW_MODE_EXTEND, band=8, cigar=True), dict(mode=agx.SW_MODE_EXTEND, band=8, diag=0),
              dict(mode=agx.SW_MODE_EXTEND, band=8, diag=0, cigar=True)]
    for kw in others:
        dev = agx.SwBatch(None, b, **kw)
        try:
            assert agx.lib().agx_sw_batch_zdrop_stops(dev._h, agx._ptr(stops)) == agx.E_ARG, kw
            assert b"not a z-drop batch" in agx.lib().agx_last_error()
        finally:
            dev.close()
    assert agx.lib().agx_sw_batch_zdrop_stops(None, agx._ptr(stops)) == agx.E_ARG
    for cigar in (False, True):
        dev = agx.SwBatch(None, b, mode=agx.SW_MODE_EXTEND, band=8, zdrop=20, cigar=cigar)
        try:
            hits, stats = np.empty(b.n_pairs, agx.SwHit), np.empty(b.n_pairs, agx.SwStat)
            assert agx.lib().agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(stats)) == agx.E_ARG
            assert agx.lib().agx_sw_batch_zdrop_stops(dev._h, None) == agx.E_ARG
        finally:
            dev.close()
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, b, mode=agx.SW_MODE_EXTEND, zdrop=20)  # no band
    assert e.value.code == agx.E_ARG


# ---- the kernels


ZD_VGPRS = {4: 59, 8: 72, 16: 99, 32: 151}


def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernel_resources(agx.LIB_PATH)


def test_kernel_resources():
    """The four new builds (K = 4, 8, 16, 32 diagonals per lane): no scratch, no AGPRs, no LDS, the VGPR counts of DESIGN.md 4.1k.
    The plain builds keep the counts of 4.1g's table, the traced ones those of 4.1h's and the builds around a diagonal their number:
    what the z-drop adds to the shared body stands inside `if constexpr`."""
    table = _resources()
    new = {k: v for k, v in table.items() if k.startswith("sw_fill_band_zd<")}
    assert sorted(new) == sorted("sw_fill_band_zd<%d>" % K for K in ZD_VGPRS), sorted(new)
    for K, vgpr in ZD_VGPRS.items():
        r = new["sw_fill_band_zd<%d>" % K]
        assert r["vgpr"] == vgpr and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (K, r)
    plain = {(4, "false"): 55, (4, "true"): 55, (8, "false"): 67, (8, "true"): 65, (16, "false"): 104, (16, "true"): 83, (32, "false"): 162,
             (32, "true"): 119}
    for (K, ext), vgpr in plain.items():
        r = table["sw_fill_band<%d, %s>" % (K, ext)]
        assert r["vgpr"] == vgpr and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (K, ext, r)
    for K, vgpr in {4: 71, 8: 96, 16: 130, 32: 186}.items():
        r = table["sw_fill_band_trace<%d>" % K]
        assert r["vgpr"] == vgpr and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (K, r)
    assert len([k for k in table if k.startswith("sw_fill_band_at<")]) == 12
    assert len([k for k in table if k.startswith("sw_fill_band<")]) == 8
