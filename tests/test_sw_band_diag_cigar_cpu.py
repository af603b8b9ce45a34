"""CIGARs for batches banded around a diagonal (include/agx.h, "CIGARs for batches banded around a diagonal") without a GPU: the
new C-ABI on plan-only batches -- the band conditions of every mode on both sides of their edges, the limits; the Python argument
rules; the checker itself (tests/sw_band_diag_cigar_ref.py) against the checkers of the sections it must agree with; the span
record that starts a traced fill inside the resident image; the new kernels' resources as the code objects state them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_cigar_ref as bc
from tests import sw_band_diag_cigar_ref as dc
from tests import sw_band_diag_ref as bd
from tests import sw_cigar_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AC = np.frombuffer(b"AC", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
MODES = pytest.mark.parametrize("mode", bd.MODES, ids=[bd.MODE_NAMES[m] for m in bd.MODES])


def _rand(rng, n, alphabet=ACGT):
    return alphabet[rng.integers(0, len(alphabet), size=n)].tobytes()


def _same(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        if k == 0:
            for f in FIELDS:
                bad = np.nonzero(g[f] != w[f])[0]
                assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], g[bad[0]], w[bad[0]])
        else:
            assert np.array_equal(np.asarray(g), np.asarray(w)), "%s: %s differ" % (what, ("hits", "op_off", "ops")[k])


def _up_to(n, seed, alphabet=AC):
    """every (la, lb) in 0..n x 0..n, a related / unrelated mix over a two-letter alphabet: ties are dense"""
    rng = np.random.default_rng(seed)
    seqs = []
    for la in range(n + 1):
        for lb in range(n + 1):
            a = _rand(rng, la, alphabet)
            t = _rand(rng, lb, alphabet) if (la + lb) % 2 or not la else (a * (lb // la + 1))[:lb]
            seqs += [a, t]
    return synth.sw_from_seqs(seqs)


def _create(b, mode, w, diag=None, scoring=None):
    h = C.c_void_p()
    sc = C.byref(agx.SwScoring(*scoring)) if scoring is not None else None
    d = agx._diag(diag, b.n_pairs)
    rc = agx.lib().agx_sw_batch_create_align_band_diag_cigar(None, sc, mode, w, agx._ptr(d), agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len),
                                                             b.n_pairs, C.byref(h))
    return rc, h


# ---- 1. the C-ABI on plan-only batches


def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(agx.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    for s in ("agx_sw_batch_create_align_band_diag_cigar", "agx_sw_align_band_diag_cigar", "agx_sw_band_span_record"):
        assert s in agx.SYMBOLS and hasattr(lib, s) and ("int %s(" % s) in hdr, s
    assert "CIGARs for batches banded around a diagonal" in hdr


@MODES
def test_plan_only_batch(mode):
    rng = np.random.default_rng(141)
    seqs = [b"ACGT" * 20, b"ACGT" * 30, b"", b"ACG", b"ACG", b"", b"", b""]
    for n in (1, 5, 150, 2000, 10000, 65535):
        seqs += [_rand(rng, n), _rand(rng, max(1, n - 7))]
    b = synth.sw_from_seqs(seqs)
    dev = agx.SwBatch(None, b, mode=mode, cigar=True, band=64, diag=0)
    plain = agx.SwBatch(None, b, mode=mode, band=64, diag=0)
    try:
        i, j = dev.info(), plain.info()
        assert i.n_pairs == b.n_pairs and i.cells == b.cells()
        # the same plan as the band-diag SPANS batch
        assert (i.n_waves, i.n_launches, i.padded_cells, i.input_bytes) == (j.n_waves, j.n_launches, j.padded_cells, j.input_bytes)
        for call in (dev.launch, dev.hits, dev.scores, dev.cigars):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_NODEVICE
        assert dev.cigar_info().n_chunks == 0
        with pytest.raises(agx.AgxError) as e:
            dev.stats()
        assert e.value.code == agx.E_ARG
        with pytest.raises(agx.AgxError) as e:  # a plain band-diag batch is no cigar batch
            plain.cigars()
        assert e.value.code == agx.E_ARG
    finally:
        dev.close()
        plain.close()
    dev = agx.SwBatch(None, synth.sw_from_seqs([]), mode=mode, cigar=True, band=3, diag=0)
    try:
        assert dev.info().n_pairs == 0 and dev.info().n_waves == 0
    finally:
        dev.close()


@MODES
def test_every_band_condition_on_both_sides_of_its_edge(mode):
    """Every (la, lb) in 0..7, w in 0..2 and c in -10..10: the create succeeds exactly where the table of "Banded alignment around
    a diagonal" admits the pair, empty sides included, and a refusal is AGX_E_ARG naming the pair."""
    rng = np.random.default_rng(142)
    first = [_rand(rng, 9), _rand(rng, 9)]  # pair 0 is admitted around 0 in every mode: a refusal names pair 1
    edges = {"dlo<=0": [0, 0], "0<=dhi": [0, 0], "dlo<=la-lb": [0, 0], "dhi>=la-lb": [0, 0]}
    for la in range(8):
        for lb in range(8):
            b = synth.sw_from_seqs(first + [_rand(rng, la), _rand(rng, lb)])
            for w in range(3):
                for c in range(-10, 11):
                    rc, h = _create(b, mode, w, [0, c])
                    msg = agx.lib().agx_last_error()
                    if bd.admits(mode, la, lb, c, w):
                        assert rc == agx.OK and h.value, (la, lb, w, c, msg)
                        agx.lib().agx_sw_batch_destroy(h)
                    else:
                        assert rc == agx.E_ARG and not h.value and b"pair 1:" in msg, (la, lb, w, c, rc, msg)
                    dlo, dhi = c - w, c + w
                    for name, holds in (("dlo<=0", dlo <= 0), ("0<=dhi", 0 <= dhi), ("dlo<=la-lb", dlo <= la - lb), ("dhi>=la-lb", dhi >= la - lb)):
                        edges[name][int(holds)] += 1
    assert all(v[0] > 0 and v[1] > 0 for v in edges.values())


def test_limits():
    rng = np.random.default_rng(143)
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
        for c, want in ((65535 + 7 + 1, agx.E_ARG), (-(65535 + 7 + 1), agx.E_ARG)):  # |c| > AGX_SW_BAND_MAX_LEN + w
            rc, h = _create(b, mode, 7, [0, c])
            assert rc == want and not h.value and b"pair 1:" in agx.lib().agx_last_error(), (mode, c)
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
    h = C.c_void_p(1)
    assert agx.lib().agx_sw_batch_create_align_band_diag_cigar(None, None, bd.FIT, 4, None, None, None, None, 5, C.byref(h)) == agx.E_ARG and not h.value


def test_python_argument_rules():
    b = synth.sw_from_seqs([b"ACGTACGT", b"ACGTTACGT"])
    for kw in (dict(stats=True), dict(matrix=agx.SwMatrix()), dict(cigar=True, stats=True), dict(cigar=True, matrix=agx.SwMatrix()),
               dict(cigar=True, align=agx.SW_ALIGN_ENDS)):
        with pytest.raises(agx.AgxError) as e:
            agx.SwBatch(None, b, mode=bd.FIT, band=4, diag=0, **kw)
        assert e.value.code == agx.E_ARG, kw
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, b, mode=bd.FIT, diag=0, cigar=True)  # no band
    assert e.value.code == agx.E_ARG
    for kw in (dict(cigar=True), dict(cigar=True, align=agx.SW_ALIGN_SPANS), dict(cigar=True, diag=[-1])):
        dev = agx.SwBatch(None, b, mode=bd.FIT, band=4, **dict(dict(diag=0), **kw))
        assert dev.cigar_info().n_traced == 0
        dev.close()
    # without diag= nothing changes: a band around the main diagonal serves GLOBAL and EXTEND only
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, b, mode=bd.FIT, band=4, cigar=True)
    assert e.value.code == agx.E_ARG
    assert hasattr(agx.Context, "sw_align_band_diag_cigar")


# ---- 2. the checker against the checkers of the sections it must agree with


@MODES
@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2), (1, 0, 0, 0)], ids=str)
@pytest.mark.parametrize("c,w", [(0, 12), (5, 17), (-4, 16)], ids=str)
def test_checker_with_the_whole_matrix_in_the_band_equals_the_cigar_checker(mode, scoring, c, w):
    """All (la, lb) in 0..12 x 0..12 with c - w <= -lb and c + w >= la: such a band is no band, around any centre."""
    b = _up_to(12, 144)
    _same(dc.expected(b, mode, w, c, scoring), cr.expected(b, mode, scoring), "%s c=%d w=%d" % (bd.MODE_NAMES[mode], c, w))


@pytest.mark.parametrize("w", [0, 1, 2, 3, 7], ids=str)
@pytest.mark.parametrize("scoring", [None, (1, 0, 0, 0), (3, -2, -4, -1)], ids=str)
def test_checker_extend_without_diag_equals_the_band_cigar_checker(w, scoring):
    b = _up_to(12, 145)
    _same(dc.expected(b, bd.EXTEND, w, None, scoring), bc.expected(b, bc.EXTEND, w, scoring), "extend w=%d" % w)


@pytest.mark.parametrize("w", [0, 1, 2, 3, 7], ids=str)
@pytest.mark.parametrize("scoring", [None, (1, 0, 0, 0), (3, -2, -4, -1)], ids=str)
def test_checker_global_at_zero_on_square_pairs_equals_the_band_cigar_checker(w, scoring):
    rng = np.random.default_rng(146)
    seqs = []
    for n in list(range(0, 25)) * 4:
        a = _rand(rng, n, AC)
        seqs += [a, bytes(x if rng.random() > 0.2 else AC[rng.integers(0, 2)] for x in a)]
    b = synth.sw_from_seqs(seqs)
    _same(dc.expected(b, bd.GLOBAL, w, 0, scoring), bc.expected(b, bc.GLOBAL, w, scoring), "global w=%d" % w)


def test_checker_cases_worked_by_hand():
    def one(a, t, mode, w, c, sc=None):
        h, off, ops = dc.expected(synth.sw_from_seqs([a, t]), mode, w, c, sc)
        return tuple(int(v) for v in h[0]), dc.strings(off, ops)[0]

    # FIT, all of a in one gap along one row of the window: b_begin = b_end + 1, a lone run.  A row holds the five cells of
    # columns 0 .. 4 only in a band of five diagonals: at w = 2 around -5 that is row 7.  At w = 1 no row does, and the best
    # path zigzags between the band's edges: from (6, 0) two I, two D, two I to (8, 4), three gaps of two = -9.
    assert one(b"TTTT", b"AAAAAAAAAA", bd.FIT, 2, -5, (1, -100, -1, -1)) == ((-5, 0, 3, 7, 6), "4I")
    assert one(b"TTTT", b"AAAAAAAAAA", bd.FIT, 1, -5, (1, -100, -1, -1)) == ((-9, 0, 3, 6, 7), "2I2D2I")
    # LOCAL with nothing to align, and a band that misses the matrix
    assert one(b"AAAA", b"CCCC", bd.LOCAL, 2, 0) == ((0, -1, -1, -1, -1), "*")
    assert one(b"ACGT", b"ACGT", bd.LOCAL, 1, 9) == ((0, -1, -1, -1, -1), "*")
    # a read on its own diagonal, far from the main one
    assert one(b"ACGTA", b"TTTTTTTACGTATT", bd.FIT, 0, -7) == ((5, 0, 4, 7, 11), "5=")
    # LOCAL on diagonal 2
    assert one(b"TTACGTAC", b"ACGTAC", bd.LOCAL, 0, 2) == ((6, 2, 7, 0, 5), "6=")
    # empty sides
    assert one(b"AAA", b"", bd.GLOBAL, 3, 0) == ((-6, 0, 2, 0, -1), "3I")
    assert one(b"", b"AAA", bd.GLOBAL, 3, 0) == ((-6, 0, -1, 0, 2), "3D")
    assert one(b"", b"AAA", bd.FIT, 3, 0) == ((0, 0, -1, 0, -1), "*")


# ---- 3. the span record


def _span(la, rows, row0, fpad, dlo, dhi, lanes, hit):
    h = np.array([hit], agx.SwHit)
    sp = agx.SwBandSpan()
    rc = agx.lib().agx_sw_band_span_record(la, rows, row0, fpad, dlo, dhi, lanes, agx._ptr(h), C.byref(sp))
    return rc, sp


@pytest.mark.parametrize("row0", [0, 21], ids=["untrimmed", "trimmed"])
def test_span_record_for_every_phase_and_begin_column(row0):
    """An image of a 40-symbol query and the rows row0 .. row0 + 120 of its target in the band -70 .. -10 counted from row0, on 7
    lanes: for every s mod 4 x a_begin mod 4 the record gives the offsets, the shifted band and the steps of the definition."""
    la, rows, fpad, dlo, dhi, lanes = 40, 120, 3, -70, -10, 7
    seen = set()
    for s in range(20, 40):
        for a_begin in range(0, 9):
            for ca, cb in ((1, 1), (5, 9), (30, 33)):
                hit = (7, a_begin, a_begin + ca - 1, row0 + s, row0 + s + cb - 1)
                lo, hi = dlo + s - a_begin, dhi + s - a_begin
                rc, sp = _span(la, rows, row0, fpad, dlo, dhi, lanes, hit)
                if not (lo <= 0 <= hi and lo <= ca - cb <= hi):
                    assert rc == agx.E_ARG, (s, a_begin, ca, cb)
                    continue
                assert rc == agx.OK, (s, a_begin, ca, cb, agx.lib().agx_last_error())
                assert (sp.ca, sp.cb, sp.x_bytes, sp.y_dwords, sp.phase) == (ca, cb, fpad + a_begin, s // 4, s % 4)
                assert (sp.dlo, sp.dhi, sp.steps) == (lo, hi, cb + lanes + s % 4)
                # what the kernel relies on: byte 1 + phase behind the moved offset is b[b_begin], the width is unchanged
                assert 4 * sp.y_dwords + sp.phase == s and sp.dhi - sp.dlo == dhi - dlo
                seen.add((s % 4, a_begin % 4))
    assert len(seen) == 16
    # a span from the image's first row and column is the image's own record
    rc, sp = _span(la, rows, row0, fpad, -5, 5, lanes, (0, 0, 9, row0, row0 + 9))
    assert rc == agx.OK and (sp.x_bytes, sp.y_dwords, sp.phase, sp.dlo, sp.dhi, sp.steps) == (fpad, 0, 0, -5, 5, 10 + lanes)


def test_span_record_refusals():
    ok = (5, 1, 4, 2, 6)
    assert _span(10, 10, 0, 0, -3, 3, 2, ok)[0] == agx.OK
    for args in ((10, 10, 0, 0, -3, 3, 0, ok), (10, 10, 0, 0, -3, 3, 65, ok), (10, 10, 3, 0, -3, 3, 2, ok), (10, 6, 0, 0, -3, 3, 2, ok),
                 (4, 10, 0, 0, -3, 3, 2, ok), (10, 10, 0, 0, -3, 3, 2, (5, -1, 4, 2, 6)), (10, 10, 0, 0, -3, 3, 2, (5, 1, 4, 7, 6)),
                 (10, 10, 0, 0, 0, 3, 2, ok), (10, 10, 0, 0, -3, -2, 2, ok), (10, 10, 0, 0, -3, 3, 2, (5, 1, 9, 2, 3))):
        assert _span(*args)[0] == agx.E_ARG, args
    assert agx.lib().agx_sw_band_span_record(10, 10, 0, 0, -3, 3, 2, None, C.byref(agx.SwBandSpan())) == agx.E_ARG


# ---- 4. the kernels


TRACED_AT_VGPRS = {4: 71, 8: 99, 16: 116, 32: 184}


def test_kernel_resources():
    """The four traced builds that start inside the image and their walk: no scratch, no AGPRs, no LDS, the VGPR counts of
    DESIGN.md 4.1j's table."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.kernel_resources(agx.LIB_PATH)
    new = {k: v for k, v in table.items() if k.startswith("sw_fill_band_trace_at<")}
    assert len(new) == 4, sorted(new)
    for K, vgpr in TRACED_AT_VGPRS.items():
        r = table["sw_fill_band_trace_at<%d>" % K]
        assert r["vgpr"] == vgpr and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, (K, r)
    r = table["sw_walk_band_at"]
    assert r["vgpr"] == 32 and r["scratch"] == 0 and r["agpr"] == 0 and r["lds"] == 0, r
