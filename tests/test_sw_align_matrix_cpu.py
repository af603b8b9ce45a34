"""Align batches under a substitution matrix, the parts that need no device: the by-definition checker of
tests/sw_matrix_align_ref.py pinned to the checkers that already exist and to the oracle, and the ABI of
agx_sw_batch_create_align_matrix / agx_sw_align_matrix on plan-only batches."""
import ctypes as C

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_align_ref, sw_modes_ref
from tests import sw_matrix_align_ref as ref

FIELDS = ("score", "a_begin", "a_end", "b_begin", "b_end")
DNA = b"ACGTN\n"
BLOSUM = lambda: agx.SwMatrix.build(synth.AMINO, synth.BLOSUM62, -11, -1)


def _same(got, want, what=""):
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s %s: %d pairs differ, first %d: got %s, want %s" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _dna_pairs():
    """400 seeded pairs of lengths 0..120 over ACGTN and the newline: a third unrelated, a third mutated copies, a third
    repeats (ties)."""
    rng = np.random.default_rng(71)
    sym = np.frombuffer(b"ACGTACGTACGTN", np.uint8)
    seqs = []
    for k in range(400):
        la, lb = int(rng.integers(0, 121)), int(rng.integers(0, 121))
        a = sym[rng.integers(0, sym.size, size=la)]
        if k % 3 == 0:
            t = sym[rng.integers(0, sym.size, size=lb)]
        elif k % 3 == 1:
            t = np.resize(a, lb).copy() if la else sym[rng.integers(0, sym.size, size=lb)]
            hit = rng.random(lb) < 0.1
            t[hit] = sym[rng.integers(0, sym.size, size=int(hit.sum()))]
        else:
            unit = sym[rng.integers(0, 4, size=int(rng.integers(1, 4)))]
            a, t = np.resize(unit, la), np.resize(unit, lb)
        a, t = a.tobytes(), t.tobytes()
        if k % 4 == 0:  # the reference CLI's trailing newline, a symbol like any other
            a, t = a + b"\n", t + b"\n"
        seqs += [a, t]
    return synth.sw_from_seqs(seqs)


@pytest.fixture(scope="module")
def dna():
    return _dna_pairs()


@pytest.mark.parametrize("scoring", [sw_modes_ref.REFERENCE_SCORING, (1, 0, 0, 0)], ids=str)
@pytest.mark.parametrize("what", [ref.ENDS, ref.SPANS], ids=["ends", "spans"])
def test_checker_equals_the_match_mismatch_checkers(dna, scoring, what):
    """A matrix of match on the diagonal and mismatch elsewhere over ACGTN\\n: record for record what sw_align_ref (LOCAL)
    and sw_modes_ref (the four other modes) give.  (1, 0, 0, 0): free gaps and mismatches, ties everywhere."""
    assert dna.n_pairs == 400 and int(dna.len.min()) == 0
    m = ref.match_matrix(DNA, *scoring)
    _same(ref.align(dna, m, ref.LOCAL, what), sw_align_ref.align(dna, what, scoring), "local")
    for mode in sw_modes_ref.MODES:
        _same(ref.align(dna, m, mode, what), sw_modes_ref.align(dna, mode, what, scoring), sw_modes_ref.MODE_NAMES[mode])


def test_checker_local_scores_equal_the_oracle_under_blosum62(oracle):
    b = synth.protein_pairs(300, 1, 150, seed=72)
    m = BLOSUM()
    assert np.array_equal(ref.align(b, m, ref.LOCAL, ref.ENDS)["score"], oracle.sw_batch_matrix(b, m))


def test_checker_on_hand_made_cases():
    m = BLOSUM()
    # the hand-checked pairs of tests/test_oracle_sw.py: WW+F/W+W = 11+11+1+11; HEA/HEA = 8+5+4 beats AWGHE/AW-HE = 16
    assert ref.align_seqs([b"WWWW", b"WWFW", b"HEAGAWGHEE", b"PAWHEAE"], m, ref.LOCAL) == [(34, 0, 3, 0, 3), (17, 0, 2, 3, 5)]
    # global: A-W against W pays the gap in front or behind: W/W 11 + (-11 - 1); all of a, all of b
    assert ref.align_seqs([b"AW", b"W"], m, ref.GLOBAL) == [(-1, 0, 1, 0, 0)]
    # a diagonal that is not positive: nothing is consumed in LOCAL and EXTEND, GLOBAL is negative
    z = agx.SwMatrix.build(b"AC", [[-1, -2], [-2, 0]], -3, -1)
    assert ref.align_seqs([b"ACCA", b"ACCA"], z, ref.LOCAL) == [(0, -1, -1, -1, -1)]
    assert ref.align_seqs([b"ACCA", b"ACCA"], z, ref.EXTEND) == [(0, -1, -1, -1, -1)]
    assert ref.align_seqs([b"ACCA", b"ACCA"], z, ref.GLOBAL) == [(-2, 0, 3, 0, 3)]


# ---- ABI (plan-only batches: ctx = NULL)

def _create(matrix, b, mode=agx.SW_MODE_LOCAL, what=agx.SW_ALIGN_SPANS):
    h = C.c_void_p()
    rc = agx.lib().agx_sw_batch_create_align_matrix(None, C.byref(matrix) if matrix is not None else None, mode, what, agx._ptr(b.bases),
                                                    agx._ptr(b.off), agx._ptr(b.len), b.n_pairs, C.byref(h))
    return rc, h


def test_both_symbols_are_exported_and_declared():
    for name in ("agx_sw_batch_create_align_matrix", "agx_sw_align_matrix"):
        assert name in agx.SYMBOLS
        assert getattr(agx.lib(), name)


@pytest.mark.parametrize("mode", ref.MODES, ids=[ref.MODE_NAMES[m] for m in ref.MODES])
def test_plan_only_batch_answers_info(mode):
    b = synth.protein_pairs(200, 1, 300, seed=73)
    for what in (agx.SW_ALIGN_ENDS, agx.SW_ALIGN_SPANS):
        p = agx.SwBatch(None, b, matrix=BLOSUM(), align=what, mode=mode)
        i = p.info()
        assert i.n_pairs == 200 and i.cells == b.cells() and i.padded_cells >= i.cells and i.n_launches >= 1
        with pytest.raises(agx.AgxError) as e:
            p.launch()
        assert e.value.code == agx.E_NODEVICE
        p.close()


def test_bad_arguments_are_e_arg():
    b = synth.sw_from_seqs([b"ARND", b"ARNE"])
    rc, h = _create(None, b)
    assert rc == agx.E_ARG and not h.value and b"NULL" in agx.lib().agx_last_error()
    skew = BLOSUM()
    skew.score[2][5] += 1
    rc, h = _create(skew, b)
    assert rc == agx.E_ARG and not h.value and b"symmetric" in agx.lib().agx_last_error()
    rc, h = _create(BLOSUM(), b, mode=5)
    assert rc == agx.E_ARG and not h.value and b"mode = 5" in agx.lib().agx_last_error()
    rc, h = _create(BLOSUM(), b, mode=-1)
    assert rc == agx.E_ARG and not h.value
    rc, h = _create(BLOSUM(), b, what=0)
    assert rc == agx.E_ARG and not h.value and b"what = 0" in agx.lib().agx_last_error()
    out = np.empty(1, agx.SwHit)
    assert agx.lib().agx_sw_align_matrix(None, None, 0, agx.SW_ALIGN_ENDS, agx._ptr(b.bases), agx._ptr(b.off), agx._ptr(b.len), 1, agx._ptr(out)) == agx.E_ARG
    with pytest.raises(agx.AgxError) as e:  # the Python view: a matrix together with scoring= is an error
        agx.SwBatch(None, b, scoring=(1, -1, -3, -1), matrix=BLOSUM(), align=agx.SW_ALIGN_ENDS)
    assert e.value.code == agx.E_ARG


def test_matrix_validation_is_the_score_only_batchs():
    b = synth.sw_from_seqs([b"ARND", b"ARNE"])
    for change, code in ((lambda m: setattr(m, "n_symbols", 0), agx.E_ARG), (lambda m: setattr(m, "n_symbols", 33), agx.E_ARG),
                         (lambda m: m.code.__setitem__(ord("A"), 20), agx.E_ARG), (lambda m: setattr(m, "gap_open", 1), agx.E_LIMIT),
                         (lambda m: setattr(m, "gap_extend", -1001), agx.E_LIMIT)):
        m = BLOSUM()
        change(m)
        rc, h = _create(m, b)
        with pytest.raises(agx.AgxError) as e:
            agx.SwBatch(None, b, matrix=m)
        assert rc == code == e.value.code and not h.value


def test_a_byte_outside_the_alphabet_names_the_pair():
    b = synth.sw_from_seqs([b"ARND", b"ARNE", b"ARND", b"ARNB", b"ARND\n", b"ARND"])
    for mode in ref.MODES:
        rc, h = _create(BLOSUM(), b, mode=mode)
        assert rc == agx.E_SYMBOL and not h.value
        assert agx.lib().agx_last_error().startswith(b"pair 1 ")


def test_limits_are_the_align_batchs():
    m = BLOSUM()
    rc, h = _create(m, synth.sw_from_seqs([b"A" * 2561, b"R" * 10]))
    assert rc == agx.E_LIMIT and not h.value and b"pair 0" in agx.lib().agx_last_error()
    rc, h = _create(m, synth.sw_from_seqs([b"A" * 10, b"R" * 65536]))
    assert rc == agx.E_LIMIT and not h.value
    # the roles carry the limits: a query of 2560 against a target of 3000 plans
    rc, h = _create(m, synth.sw_from_seqs([b"A" * 2560, b"R" * 3000]), mode=agx.SW_MODE_GLOBAL)
    assert rc == agx.OK and h.value
    agx.lib().agx_sw_batch_destroy(h)
    rc, h = _create(m, synth.sw_from_seqs([b"A" * 2561, b""]), mode=agx.SW_MODE_GLOBAL)  # an empty side does not lift them
    assert rc == agx.E_LIMIT and not h.value
