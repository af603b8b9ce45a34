"""Banded alignment (include/agx.h, "Banded alignment") without a GPU: the checker itself (tests/sw_band_ref.py) against the
unbanded checker, on cases worked by hand and on a property of the definition; the new C-ABI on plan-only batches; the banded
kernels' resources as the code objects state them."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_ref as band
from tests import sw_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
GLOBAL, EXTEND = agx.SW_MODE_GLOBAL, agx.SW_MODE_EXTEND


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def _same(got, want, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _up_to_40():
    """The related / unrelated mix of tests/test_sw_modes_gpu.py::test_every_length_pair_up_to_40."""
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


# ---- 1. the checker against the existing checker


@pytest.mark.parametrize("mode,w", [(GLOBAL, 40), (EXTEND, 41)], ids=["global", "extend"])
@pytest.mark.parametrize("scoring", [None, (2, -3, -5, -2), (1, 0, 0, 0)], ids=str)
def test_wide_band_checker_equals_the_unbanded_checker(mode, w, scoring):
    """All (la, lb) in 0..40 x 0..40: a band that holds the whole matrix is no band (w >= min(la, lb) in GLOBAL, >= max in EXTEND)."""
    b = _up_to_40()
    _same(band.align(b, mode, w, scoring), ref.align(b, mode, ref.SPANS, scoring), band.MODE_NAMES[mode])


# ---- 2. the checker on cases worked by hand


def test_band_zero_is_the_pure_diagonal():
    rng = np.random.default_rng(51)
    for sc in ((1, -1, -3, -1), (2, -3, -5, -2), (12, -116, -1000, -1000)):
        for n in (1, 2, 7, 64, 301):
            a = _rand(rng, n)
            t = bytearray(a)
            for k in rng.integers(0, n, size=n // 3):
                t[k] = ord("N")  # a sure mismatch
            t = bytes(t)
            matches = sum(x == y for x, y in zip(a, t))
            want = matches * sc[0] + (n - matches) * sc[1]
            assert band.align_seqs([a, t], GLOBAL, 0, sc) == [(want, 0, n - 1, 0, n - 1)]
            # EXTEND on the same diagonal: the best prefix
            run, best, at = 0, 0, -1
            for k, (x, y) in enumerate(zip(a, t)):
                run += sc[0] if x == y else sc[1]
                if run > best:
                    best, at = run, k
            assert band.align_seqs([a, t], EXTEND, 0, sc) == [(best, 0, at, 0, at) if best > 0 else (0, -1, -1, -1, -1)]


def test_global_band_zero_with_three_more_query_symbols():
    """GLOBAL, w = 0, la = lb + 3: the band is the diagonals 0..3, so exactly three query symbols fall into gaps."""
    sc = (1, -1, -3, -1)
    # one gap of three anywhere costs -3 + 3 * -1 = -6; eight matches
    assert band.align_seqs([b"ACGTTTTACGT", b"ACGTACGT"], GLOBAL, 0, sc) == [(8 - 6, 0, 10, 0, 7)]
    assert band.align_seqs([b"AAAACGTACGT", b"CGTACGT"], GLOBAL, 0, sc)[0][0] == 7 - 7  # a_end - b_end = 4: gap of four in front
    assert band.align_seqs([b"AAA", b""], GLOBAL, 0, sc) == [(-6, 0, 2, 0, -1)]
    assert band.align_seqs([b"", b"AAA"], GLOBAL, 0, sc) == [(-6, 0, -1, 0, 2)]
    assert band.align_seqs([b"", b""], GLOBAL, 0, sc) == [(0, 0, -1, 0, -1)]
    assert band.align_seqs([b"", b"AAA"], EXTEND, 5, sc) == [(0, -1, -1, -1, -1)]
    # the mirrored pair has the same score (the band is widened downwards instead)
    assert band.align_seqs([b"ACGTACGT", b"ACGTTTTACGT"], GLOBAL, 0, sc) == [(2, 0, 7, 0, 10)]
    # three single gaps would cost 3 * -4: with w = 0 they are still allowed anywhere on diagonals 0..3
    assert band.align_seqs([b"ACGTTTTACGT", b"ACGTACGT"], GLOBAL, 0, (1, -1, 0, -1))[0][0] == 8 - 3


def indel_pair(rng, g, n=300, first=100, apart=100):
    """A pair of n symbols each that differs by a deletion of g symbols at `first` and an insertion of g symbols `apart` further on:
    between the two the alignment runs g diagonals off the main one."""
    a = _rand(rng, n)
    t = a[:first] + a[first + g:first + g + apart] + _rand(rng, g) + a[first + g + apart:]
    return a, t


@pytest.mark.parametrize("w", [1, 6, 33])
def test_an_indel_longer_than_the_band_must_be_routed_inside_it(w):
    """Indels of g = w - 1, w, w + 1: the banded global score equals the unbanded one while the shifted stretch fits the band
    (g <= w) and falls below it when it does not (g = w + 1)."""
    rng = np.random.default_rng(52)
    for g in (w - 1, w, w + 1):
        if g == 0:
            continue
        for _ in range(8):
            a, t = indel_pair(rng, g)
            assert len(a) == len(t) == 300
            free = ref.align_seqs([a, t], ref.GLOBAL)[0]
            got = band.align_seqs([a, t], GLOBAL, w)[0]
            if g <= w:
                assert got == free, (g, w)
            else:
                assert got[0] < free[0] and got[1:] == free[1:], (g, w)


# ---- 3. plan-only batches


def _create(b, mode, w, scoring=None):
    h = C.c_void_p()
    sc = C.byref(agx.SwScoring(*scoring)) if scoring is not None else None
    rc = agx.lib().agx_sw_batch_create_align_band(None, sc, mode, w, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h))
    return rc, h


def test_new_symbols_are_exported():
    lib = C.CDLL(agx.LIB_PATH)
    for s in ("agx_sw_batch_create_align_band", "agx_sw_align_band"):
        assert s in agx.SYMBOLS and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "agx.h")).read()
    assert "#define AGX_SW_BAND_MAX_LEN 65535\n" in hdr and "#define AGX_SW_BAND_MAX_WIDTH 2048\n" in hdr
    assert (agx.SW_BAND_MAX_LEN, agx.SW_BAND_MAX_WIDTH) == (65535, 2048)


@pytest.mark.parametrize("mode", [GLOBAL, EXTEND])
def test_plan_only_batch(mode):
    rng = np.random.default_rng(53)
    seqs = [b"ACGT" * 20, b"ACGT" * 30, b"", b"ACG", b"ACG", b"", b"", b""]
    for n in (1, 5, 150, 2000, 10000, 65535):
        seqs += [_rand(rng, n), _rand(rng, max(1, n - 7))]
    b = synth.sw_from_seqs(seqs)
    dev = agx.SwBatch(None, b, mode=mode, band=64)
    try:
        i = dev.info()
        assert i.n_pairs == b.n_pairs and i.cells == b.cells() == int((b.len[0::2].astype(np.int64) * b.len[1::2]).sum())
        assert i.n_waves > 0 and i.n_launches >= 1 and i.padded_cells > 0 and i.input_bytes >= int(b.len.sum())
        for call in (dev.launch, dev.hits, dev.scores):
            with pytest.raises(agx.AgxError) as e:
                call()
            assert e.value.code == agx.E_NODEVICE
        # no statistics and no CIGARs on a banded batch
        hits, stats = np.empty(b.n_pairs, agx.SwHit), np.empty(b.n_pairs, agx.SwStat)
        assert agx.lib().agx_sw_batch_stats(dev._h, agx._ptr(hits), agx._ptr(stats)) == agx.E_ARG
        op_off = np.zeros(b.n_pairs + 1, np.uint64)
        assert agx.lib().agx_sw_batch_cigars(dev._h, agx._ptr(hits), agx._ptr(op_off), None, 0) == agx.E_ARG
    finally:
        dev.close()
    dev = agx.SwBatch(None, synth.sw_from_seqs([]), mode=mode, band=3)
    try:
        assert dev.info().n_pairs == 0 and dev.info().n_waves == 0
    finally:
        dev.close()


def test_argument_errors():
    b = synth.sw_pairs(4, 5, 20, seed=4)
    rc, h = _create(b, GLOBAL, -1)
    assert rc == agx.E_ARG and not h.value and b"band" in agx.lib().agx_last_error()
    for mode in (agx.SW_MODE_LOCAL, agx.SW_MODE_FIT, agx.SW_MODE_EXTEND_QUERY, -1, 5, 99):
        rc, h = _create(b, mode, 8)
        assert rc == agx.E_ARG and not h.value and b"mode" in agx.lib().agx_last_error(), mode
        out = np.empty(b.n_pairs, agx.SwHit)
        rc = agx.lib().agx_sw_align_band(None, None, mode, 8, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, agx._ptr(out))
        assert rc == agx.E_ARG
    with pytest.raises(agx.AgxError) as e:
        agx.SwBatch(None, b, mode=GLOBAL, band=4, stats=True)
    assert e.value.code == agx.E_ARG
    rc, h = _create(b, GLOBAL, 8, (13, -1, -3, -1))  # the scoring limits are those of every batch
    assert rc == agx.E_LIMIT and not h.value


def test_limits_name_the_pair():
    rng = np.random.default_rng(54)
    short = [_rand(rng, 10), _rand(rng, 12)]

    def refused(seqs, mode, w, pair):
        rc, h = _create(synth.sw_from_seqs(seqs), mode, w)
        msg = agx.lib().agx_last_error()
        assert rc == agx.E_LIMIT and not h.value and (b"pair %d" % pair) in msg, (rc, msg)

    def accepted(seqs, mode, w):
        rc, h = _create(synth.sw_from_seqs(seqs), mode, w)
        assert rc == agx.OK and h.value, agx.lib().agx_last_error()
        agx.lib().agx_sw_batch_destroy(h)

    long = _rand(rng, 65536)
    for mode in (GLOBAL, EXTEND):
        refused(short + [long, long[:65000]], mode, 4, 1)
        refused(short + short + [long[:65000], long], mode, 4, 2)
        accepted(short + [long[:65535], long[1:]], mode, 4)  # 65535 on both sides: the point of the feature
    # width = |la - lb| + 2 w + 1 in GLOBAL
    refused(short + [long[:2348], long[:300]], GLOBAL, 0, 1)  # 2049
    refused(short + [long[:300], long[:2348]], GLOBAL, 0, 1)
    accepted(short + [long[:2347], long[:300]], GLOBAL, 0)  # 2048
    accepted(short + [long[:300], long[:2347]], GLOBAL, 0)
    refused([long[:100], long[:99]], GLOBAL, 1024, 0)  # 1 + 2048 + 1
    accepted([long[:100], long[:99]], GLOBAL, 1023)  # 1 + 2046 + 1 = 2048
    # width = 2 w + 1 in EXTEND, whatever the lengths
    refused(short, EXTEND, 1024, 0)  # 2049
    accepted(short + [long[:2348], long[:300]], EXTEND, 1023)  # 2047: the widest an EXTEND band (always odd) can be
    # an empty side still has a width
    refused([b"", long[:3000]], GLOBAL, 0, 0)
    accepted([b"", long[:2047]], GLOBAL, 0)


# ---- 4. a property of the definition


def test_global_score_does_not_fall_as_the_band_grows():
    """A wider band only adds paths: over w = 0..30 the checker's GLOBAL score never decreases, and it ends at the unbanded one."""
    b = synth.sw_pairs(200, 20, 120, seed=55, related_frac=1.0, newline=False)
    prev = band.align(b, GLOBAL, 0)["score"]
    rose = 0
    for w in range(1, 31):
        cur = band.align(b, GLOBAL, w)["score"]
        assert np.all(cur >= prev), w
        rose += int(np.count_nonzero(cur > prev))
        prev = cur
    assert rose > 0
    free = ref.align(b, ref.GLOBAL, ref.SPANS)["score"]
    assert np.all(prev <= free)
    wide = band.align(b, GLOBAL, 120)
    _same(wide, ref.align(b, ref.GLOBAL, ref.SPANS), "w = 120")


# ---- the kernels


def test_banded_kernels_resources():
    """Every banded kernel (K = 4, 8, 16, 32 diagonals per lane, two captures): no scratch, no AGPRs, no LDS."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = mod.kernel_resources(agx.LIB_PATH)
    fills = {k: v for k, v in table.items() if k.startswith("sw_fill_band<")}
    assert len(fills) == 8, sorted(fills)
    for k, r in fills.items():
        assert r["scratch"] == 0 and r["agpr"] == 0 and r["vgpr"] <= 256 and r["lds"] == 0, (k, r)
