"""Banded alignment around a diagonal (include/agx.h, "Banded alignment around a diagonal") without a GPU: the checker itself
(tests/sw_band_diag_ref.py) against the unbanded checkers and on properties of the definition; the new C-ABI on plan-only
batches -- the band conditions of every mode on both sides of their edges, the limits, the trimmed rows; the kernels' resources
as the code objects state them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_align_ref as loc
from tests import sw_band_diag_ref as bd
from tests import sw_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
MODES = pytest.mark.parametrize("mode", bd.MODES, ids=[bd.MODE_NAMES[m] for m in bd.MODES])
WHATS = pytest.mark.parametrize("what", [bd.ENDS, bd.SPANS], ids=["ends", "spans"])


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def _same(got, want, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _up_to_30():
    """The related / unrelated mix of tests/test_sw_modes_gpu.py::test_every_length_pair_up_to_40, empty sides included."""
    rng = np.random.default_rng(131)
    seqs = []
    for la in range(31):
        for lb in range(31):
            a = _rand(rng, la)
            t = _rand(rng, lb) if (la + lb) % 2 else (a * (lb // max(la, 1) + 1))[:lb]
            seqs += [a, t]
    return synth.sw_from_seqs(seqs)


def _unbanded(b, mode, what, scoring=None):
    return loc.align(b, what, scoring) if mode == bd.LOCAL else ref.align(b, mode, what, scoring)


# ---- 1. the checker against the unbanded checkers


@MODES
@WHATS
@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2), (1, 0, 0, 0)], ids=str)
@pytest.mark.parametrize("c,w", [(0, 30), (7, 37), (-11, 41)], ids=str)
def test_checker_with_the_whole_matrix_in_the_band_equals_the_unbanded_checkers(mode, what, scoring, c, w):
    """All (la, lb) in 0..30 x 0..30 with c - w <= -lb and c + w >= la: such a band is no band, around any centre."""
    b = _up_to_30()
    _same(bd.align(b, mode, w, c, what, scoring), _unbanded(b, mode, what, scoring), "%s c=%d w=%d" % (bd.MODE_NAMES[mode], c, w))


# ---- 2. properties of the definition


@pytest.mark.parametrize("mode", [bd.FIT, bd.LOCAL], ids=["fit", "local"])
def test_score_does_not_fall_as_the_band_grows(mode):
    """A wider band around the same centre only adds paths: over w = 0..30 the score never decreases and ends at the unbanded one."""
    rng = np.random.default_rng(132)
    seqs, cs = [], []
    for _ in range(150):
        read = _rand(rng, int(rng.integers(20, 60)))
        s = int(rng.integers(0, 40))
        seqs += [read, _rand(rng, s) + _mutate(rng, read) + _rand(rng, int(rng.integers(20, 40)))]
        cs.append(-s)
    b = synth.sw_from_seqs(seqs)
    cs = np.array(cs, np.int32)
    assert all(bd.admits(mode, int(b.len[2 * p]), int(b.len[2 * p + 1]), int(cs[p]), 0) for p in range(b.n_pairs))
    prev = bd.align(b, mode, 0, cs)["score"]
    rose = 0
    for w in range(1, 31):
        cur = bd.align(b, mode, w, cs)["score"]
        assert np.all(cur >= prev), w
        rose += int(np.count_nonzero(cur > prev))
        prev = cur
    assert rose > 0
    assert np.all(prev <= _unbanded(b, mode, bd.SPANS)["score"])
    _same(bd.align(b, mode, 200, cs), _unbanded(b, mode, bd.SPANS), "w = 200")


def _mutate(rng, a, sub=0.05, indel=0.03):
    out = bytearray()
    for x in a:
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out += _rand(rng, 1)
        out.append(x if rng.random() >= sub else ACGT[rng.integers(0, 4)])
    return bytes(out)


def test_a_planted_read_is_found_on_its_own_diagonal():
    """A read planted at offset s in random flanks: FIT at c = -s, w = 0 follows the one diagonal that holds it and scores la x match."""
    rng = np.random.default_rng(133)
    for sc in ((1, -1, -3, -1), (12, -116, -1000, -1000), (3, -2, 0, -1)):
        for la in (1, 5, 37, 200):
            for s in (0, 1, 17, 300):
                read = _rand(rng, la)
                window = _rand(rng, s) + read + _rand(rng, int(rng.integers(0, 50)))
                assert bd.align_seqs([read, window], bd.FIT, 0, -s, bd.SPANS, sc) == [(la * sc[0], 0, la - 1, s, s + la - 1)], (sc, la, s)
                assert bd.align_seqs([read, window], bd.FIT, 0, -s, bd.ENDS, sc) == [(la * sc[0], -1, la - 1, -1, s + la - 1)]


def test_cases_worked_by_hand():
    sc = (1, -1, -3, -1)
    # LOCAL, w = 0: the best run of one diagonal.  c = 2 pairs a[j] with b[j - 2]
    assert bd.align_seqs([b"TTACGTAC", b"ACGTAC"], bd.LOCAL, 0, 2, bd.SPANS, sc) == [(6, 2, 7, 0, 5)]
    assert bd.align_seqs([b"TTACGTAC", b"ACGTAC"], bd.LOCAL, 0, 0, bd.SPANS, sc)[0][0] < 6
    # a band that misses the matrix scores 0; so does an empty side
    assert bd.align_seqs([b"ACGT", b"ACGT", b"", b"ACGT"], bd.LOCAL, 1, 9, bd.SPANS, sc) == [(0, -1, -1, -1, -1)] * 2
    # FIT with the band's row 0 cut off (dhi < 0): the read cannot start before row -dhi
    assert bd.align_seqs([b"ACG", b"ACGTTACG"], bd.FIT, 0, -5, bd.SPANS, sc) == [(3, 0, 2, 5, 7)]
    assert bd.align_seqs([b"ACG", b"ACGTTACG"], bd.FIT, 0, 0, bd.SPANS, sc) == [(3, 0, 2, 0, 2)]
    # FIT, w = 1 around c = -1 with la = 1: column 1 holds rows 0..3 only; row 0 costs a gap, row 1 a mismatch, row 2 the match
    assert bd.align_seqs([b"A", b"CAT"], bd.FIT, 1, -1, bd.SPANS, sc) == [(1, 0, 0, 1, 1)]
    # EXTEND_QUERY: all of a, pinned start, the best row of column la inside the band
    assert bd.align_seqs([b"ACGT", b"ACGTACGT"], bd.EXTEND_QUERY, 2, 0, bd.SPANS, sc) == [(4, 0, 3, 0, 3)]
    # GLOBAL never widens: la - lb = 3 must be inside c +- w
    assert bd.align_seqs([b"ACGTTTTACGT", b"ACGTACGT"], bd.GLOBAL, 2, 1, bd.SPANS, sc) == [(8 - 6, 0, 10, 0, 7)]
    # empty sides: the formulas of "Alignment modes", whatever the band
    assert bd.align_seqs([b"AAA", b""], bd.GLOBAL, 3, 0, bd.SPANS, sc) == [(-6, 0, 2, 0, -1)]
    assert bd.align_seqs([b"AAA", b""], bd.FIT, 3, 0, bd.ENDS, sc) == [(-6, -1, 2, -1, -1)]
    assert bd.align_seqs([b"", b"AAA"], bd.FIT, 3, 0, bd.SPANS, sc) == [(0, 0, -1, 0, -1)]


# ---- 3. the C-ABI on plan-only batches


def _create(b, mode, w, diag=None, what=agx.SW_ALIGN_SPANS, scoring=None):
    h = C.c_void_p()
    sc = C.byref(agx.SwScoring(*scoring)) if scoring is not None else None
    d = agx._diag(diag, b.n_pairs)
    rc = agx.lib().agx_sw_batch_create_align_band_diag(None, sc, mode, what, w, agx._ptr(d), agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len),
                                                       b.n_pairs, C.byref(h))
    return rc, h


def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(agx.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    for s in ("agx_sw_batch_create_align_band_diag", "agx_sw_align_band_diag"):
        assert s in agx.SYMBOLS and hasattr(lib, s) and ("int %s(" % s) in hdr, s
    assert "Banded alignment around a diagonal" in hdr


@MODES
@WHATS
def test_plan_only_batch(mode, what):
    rng = np.random.default_rng(134)
    seqs = [b"ACGT" * 20, b"ACGT" * 30, b"", b"ACG", b"ACG", b"", b"", b""]
    for n in (1, 5, 150, 2000, 10000, 65535):
        seqs += [_rand(rng, n), _rand(rng, max(1, n - 7))]
    b = synth.sw_from_seqs(seqs)
    dev = agx.SwBatch(None, b, mode=mode, align=what, band=64, diag=0)
    try:
        i = dev.info()
        assert i.n_pairs == b.n_pairs and i.cells == b.cells() == int((b.len[0::2].astype(np.int64) * b.len[1::2]).sum())
        assert i.n_waves > 0 and i.n_launches >= 1 and i.padded_cells > 0 and i.input_bytes >= int(b.len.sum())
        for call in (dev.launch, dev.hits, dev.scores):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_NODEVICE
        hits, stats = np.empty(b.n_pairs, agx.SwHit), np.empty(b.n_pairs, agx.SwStat)
        assert agx.lib().agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(stats)) == agx.E_ARG
        op_off = np.zeros(b.n_pairs + 1, np.uint64)
        assert agx.lib().agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), None, 0) == agx.E_ARG
    finally:
        dev.close()
    dev = agx.SwBatch(None, synth.sw_from_seqs([]), mode=mode, align=what, band=3, diag=0)
    try:
        assert dev.info().n_pairs == 0 and dev.info().n_waves == 0
        hits, stats = np.empty(1, agx.SwHit), np.empty(1, agx.SwStat)
        assert agx.lib().agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(stats)) == agx.E_ARG
        assert agx.lib().agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(np.zeros(1, np.uint64)), None, 0) == agx.E_ARG
    finally:
        dev.close()
    # a batch of empty sides only plans no fill
    dev = agx.SwBatch(None, synth.sw_from_seqs([b"", b"ACG", b"ACG", b"", b"", b""]), mode=mode, align=what, band=3, diag=0)
    try:
        assert dev.info().n_pairs == 3 and dev.info().n_waves == 0 and dev.info().cells == 0
    finally:
        dev.close()


@MODES
def test_every_band_condition_on_both_sides_of_its_edge(mode):
    """Every (la, lb) in 0..7, w in 0..2 and c in -10..10: the create succeeds exactly where the header's table admits the pair,
    empty sides included, and a refusal is AGX_E_ARG naming the pair.  Each condition's edge lies inside this range (dlo = 0 and 1,
    dhi = 0 and -1, dlo = la - lb and one more, dhi = la - lb and one less)."""
    rng = np.random.default_rng(135)
    first = [_rand(rng, 9), _rand(rng, 9)]  # pair 0 is admitted around 0 in every mode: a refusal names pair 1
    edges = {"dlo<=0": [0, 0], "0<=dhi": [0, 0], "dlo<=la-lb": [0, 0], "dhi>=la-lb": [0, 0]}
    for la in range(8):
        for lb in range(8):
            b = synth.sw_from_seqs(first + [_rand(rng, la), _rand(rng, lb)])
            for w in range(3):
                for c in range(-10, 11):
                    rc, h = _create(b, mode, w, [0, c])
                    ok = bd.admits(mode, la, lb, c, w)
                    msg = agx.lib().agx_last_error()
                    if ok:
                        assert rc == agx.OK and h.value, (la, lb, w, c, msg)
                        agx.lib().agx_sw_batch_destroy(h)
                    else:
                        assert rc == agx.E_ARG and not h.value and b"pair 1:" in msg, (la, lb, w, c, rc, msg)
                    dlo, dhi = c - w, c + w
                    for name, holds in (("dlo<=0", dlo <= 0), ("0<=dhi", 0 <= dhi), ("dlo<=la-lb", dlo <= la - lb), ("dhi>=la-lb", dhi >= la - lb)):
                        edges[name][int(holds)] += 1
    assert all(v[0] > 0 and v[1] > 0 for v in edges.values())


def test_the_table_by_hand():
    """One refusal and one acceptance per condition of the table, at the edge, on a 10 x 20 pair (la - lb = -10)."""
    rng = np.random.default_rng(136)
    b = synth.sw_from_seqs([_rand(rng, 10), _rand(rng, 20)])

    def verdict(mode, w, c):
        rc, h = _create(b, mode, w, c)
        if h.value:
            agx.lib().agx_sw_batch_destroy(h)
        else:
            assert b"pair 0:" in agx.lib().agx_last_error()
        return rc

    G, X, Q, F, L = bd.GLOBAL, bd.EXTEND, bd.EXTEND_QUERY, bd.FIT, bd.LOCAL
    # GLOBAL: 0 and -10 inside c +- w
    assert verdict(G, 5, -5) == agx.OK and verdict(G, 5, -4) == agx.E_ARG and verdict(G, 5, -6) == agx.E_ARG and verdict(G, 4, -5) == agx.E_ARG
    # EXTEND: 0 inside
    assert verdict(X, 3, 3) == agx.OK and verdict(X, 3, 4) == agx.E_ARG and verdict(X, 3, -3) == agx.OK and verdict(X, 3, -4) == agx.E_ARG
    # EXTEND_QUERY: 0 inside and dhi >= -10 (which 0 <= dhi implies here); on a 20 x 10 pair it does not
    assert verdict(Q, 3, 3) == agx.OK and verdict(Q, 3, 4) == agx.E_ARG and verdict(Q, 3, -4) == agx.E_ARG
    b2 = synth.sw_from_seqs([_rand(rng, 20), _rand(rng, 10)])
    for w, c, want in ((5, 5, agx.OK), (5, 4, agx.E_ARG), (10, 0, agx.OK), (9, 0, agx.E_ARG)):
        rc, h = _create(b2, Q, w, c)
        assert rc == want, (w, c)
        if h.value:
            agx.lib().agx_sw_batch_destroy(h)
    # FIT: dlo <= 0 and dhi >= -10
    assert verdict(F, 2, 2) == agx.OK and verdict(F, 2, 3) == agx.E_ARG and verdict(F, 2, -12) == agx.OK and verdict(F, 2, -13) == agx.E_ARG
    # LOCAL: nothing
    for c in (-65535 - 2, -30, 0, 30, 65535 + 2):
        assert verdict(L, 2, c) == agx.OK


def test_limits():
    rng = np.random.default_rng(137)
    short = [_rand(rng, 10), _rand(rng, 12)]
    b = synth.sw_from_seqs(short + short)
    for mode in bd.MODES:
        rc, h = _create(b, mode, -1, 0)
        assert rc == agx.E_ARG and not h.value and b"band" in agx.lib().agx_last_error()
        rc, h = _create(b, mode, 1024, 0)  # 2w + 1 = 2049
        assert rc == agx.E_LIMIT and not h.value
        rc, h = _create(b, mode, 1023, 0)
        assert rc == agx.OK and h.value
        agx.lib().agx_sw_batch_destroy(h)
        for c in (65535 + 7 + 1, -(65535 + 7 + 1)):  # |c| > AGX_SW_BAND_MAX_LEN + w
            rc, h = _create(b, mode, 7, [0, c])
            assert rc == agx.E_ARG and not h.value and b"pair 1:" in agx.lib().agx_last_error(), (mode, c)
        for what in (0, 3):
            rc, h = _create(b, mode, 7, 0, what)
            assert rc == agx.E_ARG and not h.value and b"what" in agx.lib().agx_last_error()
        rc, h = _create(b, mode, 8, 0, scoring=(13, -1, -3, -1))
        assert rc == agx.E_LIMIT and not h.value
    for c in (65535 + 7, -(65535 + 7)):  # the farthest centre: LOCAL admits it, the band misses the matrix
        rc, h = _create(b, bd.LOCAL, 7, [0, c])
        assert rc == agx.OK and h.value
        agx.lib().agx_sw_batch_destroy(h)
    for mode in (-1, 5, 99):
        rc, h = _create(b, mode, 8, 0)
        assert rc == agx.E_ARG and not h.value and b"mode" in agx.lib().agx_last_error()
    long = _rand(rng, 65536)
    for mode in bd.MODES:
        rc, h = _create(synth.sw_from_seqs(short + [long, long[:65000]]), mode, 600, 0)
        assert rc == agx.E_LIMIT and not h.value and b"pair 1" in agx.lib().agx_last_error()
        rc, h = _create(synth.sw_from_seqs(short + short + [long[:65000], long]), mode, 600, 0)
        assert rc == agx.E_LIMIT and not h.value and b"pair 2" in agx.lib().agx_last_error()
        rc, h = _create(synth.sw_from_seqs(short + [long[:65535], long[1:]]), mode, 4, 0)  # 65535 on both sides
        assert rc == agx.OK and h.value
        agx.lib().agx_sw_batch_destroy(h)
    # the old entry still refuses the modes with a free start or a column capture
    for mode in (bd.LOCAL, bd.FIT, bd.EXTEND_QUERY):
        h = C.c_void_p()
        rc = agx.lib().agx_sw_batch_create_align_band(None, None, mode, 8, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h))
        assert rc == agx.E_ARG and not h.value
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, b, mode=bd.FIT, band=4, diag=0, stats=True)
    assert e.value.code == agx.E_ARG


def test_only_the_rows_the_band_touches_are_issued():
    """One pair with la = 100, lb = 60 000, c = -30 000, w = 8 in FIT: the band touches the rows -dhi .. la - dlo only, 100 + 2w + 1
    of them, and a group steps over those plus its lanes (at most 64) -- a wave issues 64 lanes x at most 32 diagonals a step."""
    rng = np.random.default_rng(138)
    la, lb, c, w = 100, 60000, -30000, 8
    dev = agx.SwBatch(None, synth.sw_from_seqs([_rand(rng, la), _rand(rng, lb)]), mode=bd.FIT, band=w, diag=c)
    try:
        i = dev.info()
        assert i.cells == la * lb and i.n_waves == 1
        assert 0 < i.padded_cells <= 64 * 32 * (la + 2 * w + 1 + 64), i.padded_cells
    finally:
        dev.close()
    # untrimmed the same pair would step over all of b
    assert 64 * 4 * lb > 64 * 32 * (la + 2 * w + 1 + 64)


# ---- the kernels


TRACED_VGPRS = {4: 71, 8: 96, 16: 130, 32: 186}


def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernel_resources(agx.LIB_PATH)


def test_kernel_resources():
    """The twelve new builds (K = 4, 8, 16, 32 diagonals per lane; LOCAL, FIT, EXTEND_QUERY): no scratch, no AGPRs, no LDS.  The
    eight plain builds keep the VGPR counts of DESIGN.md 4.1g's table and the traced four those of 4.1h's: what the new builds add
    to the shared body stands inside `if constexpr`."""
    table = _resources()
    new = {k: v for k, v in table.items() if k.startswith("sw_fill_band_at<")}
    assert len(new) == 12, sorted(new)
    for k, r in new.items():
        assert r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0 and r["vgpr"] <= 256, (k, r)
    plain = {(4, "false"): 55, (4, "true"): 55, (8, "false"): 67, (8, "true"): 65, (16, "false"): 104, (16, "true"): 83, (32, "false"): 162,
             (32, "true"): 119}
    for (K, ext), vgpr in plain.items():
        r = table["sw_fill_band<%d, %s>" % (K, ext)]
        assert r["vgpr"] == vgpr and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (K, ext, r)
    for K, vgpr in TRACED_VGPRS.items():
        r = table["sw_fill_band_trace<%d>" % K]
        assert r["vgpr"] == vgpr and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (K, r)
