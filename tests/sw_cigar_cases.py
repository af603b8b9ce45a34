"""Batches of the CIGAR tests (tests/test_sw_cigar_cpu.py, tests/test_sw_cigar_gpu.py): the generators of the modes and stats
tests, made once per process and shared; expectations by tests/sw_cigar_ref.py are cached beside them and never changed."""
import os

import numpy as np

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_cigar_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
AMINO = b"ARNDCQEGHILKMFPSTWYV"
TIE_SCORINGS = [(1, -1, -3, -1), (1, 0, 0, 0), (1, -2, 0, -1), (2, -3, -5, -2)]
QMAX = agx.SW_CIGAR_MAX_QUERY_LEN
T = QMAX // 64  # the widest lane class of the traced builds

_cache = {}


def shared(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def expected(name, b, mode, scoring=None, matrix=None):
    """(hits, op_off, ops) by definition, computed once per (batch, mode, scoring)."""
    return shared(("want", name, mode, scoring), lambda: ref.expected(b, mode, scoring, matrix))


def rand(rng, n, alphabet=ACGT):
    return alphabet[rng.integers(0, alphabet.size, size=n)].tobytes()


def up_to_40(alphabet=ACGT, seed=31):
    """len(a) x len(b) over 0..40 x 0..40: half random, half b built from copies of a."""
    rng = np.random.default_rng(seed)
    seqs = []
    for la in range(41):
        for lb in range(41):
            a = rand(rng, la, alphabet)
            if (la + lb) % 2:
                t = rand(rng, lb, alphabet)
            else:  # b from copies of a: the maximum is reached many times
                t = (a * (lb // max(la, 1) + 1))[:lb]
            seqs += [a, t]
    return synth.sw_from_seqs(seqs)


def lane_edges():
    """Queries either side of one, two and all 64 lanes of the narrow and the widest class against targets of 1..60 rows:
    random, the end of a, and the end of a plus a tail."""
    rng = np.random.default_rng(33)
    seqs = []
    for la in (38, 39, 40, 41, 79, 80, 81, 150, 151, 152, 300, 512, T - 1, T, T + 1, 2 * T, 2 * T + 1, 64 * T - 1, 64 * T):
        a = rand(rng, la)
        for lb in range(1, 61):
            kind = lb % 3
            if kind == 0:
                t = rand(rng, lb)
            elif kind == 1:
                t = a[-lb:]
            else:
                t = (a[-(lb - lb // 3):] + rand(rng, lb))[:lb]
            seqs += [a, t]
    return synth.sw_from_seqs(seqs)


def tie_heavy():
    """600 pairs of lengths 1..199: homopolymers, tandem repeats of period 2..4, a read with one insertion or deletion inside
    a repeat, and random pairs."""
    rng = np.random.default_rng(32)
    seqs = []
    for k in range(600):
        la, lb = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        kind = k % 4
        if kind == 0:  # homopolymers: every tie at once
            a, t = b"A" * la, b"A" * lb
        elif kind == 1:  # tandem repeats of period 2..4
            unit = rand(rng, int(rng.integers(2, 5)))
            a, t = (unit * la)[:la], (unit * lb)[:lb]
        elif kind == 2:  # a repeat between two flanks; the read has one unit more or one symbol less inside it
            unit = rand(rng, int(rng.integers(1, 5)))
            f1, f2 = rand(rng, int(rng.integers(3, 30))), rand(rng, int(rng.integers(3, 30)))
            n = int(rng.integers(2, 25))
            rep = unit * n
            a = f1 + rep + f2
            t = f1 + (rep + unit if k % 8 < 4 else rep[:-1]) + f2
            a, t = a[:199], t[:199]
        else:
            a, t = rand(rng, la), rand(rng, lb)
        seqs += [a, t]
    return synth.sw_from_seqs(seqs)


def blosum62():
    path = os.path.join(ROOT, "tests", "golden", "blosum62.mat")
    rows = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    alphabet = "".join(rows[0]).encode()
    scores = [[int(v) for v in r[1:]] for r in rows[1:]]
    assert [r[0] for r in rows[1:]] == rows[0]
    return agx.SwMatrix.build(alphabet, scores, -11, -1)


def four_symbols():
    """Zero and positive entries off the diagonal: a mismatch can tie with or beat a match elsewhere."""
    return agx.SwMatrix.build(b"ACGT", [[2, 1, 0, -3], [1, 2, -3, 0], [0, -3, 2, 1], [-3, 0, 1, 2]], -2, -1)


def protein_pairs(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    aa = np.frombuffer(AMINO, np.uint8)
    seqs = []
    for k in range(n):
        la, lb = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        a = aa[rng.integers(0, 20, size=la)]
        if k % 3 == 0:  # a mutated copy: 10 % substitutions, a few indels, cut or padded to its length
            t = a.copy()
            sub = rng.random(t.size) < 0.1
            t[sub] = aa[rng.integers(0, 20, size=int(sub.sum()))]
            for _ in range(int(rng.integers(0, 4))):
                at = int(rng.integers(0, t.size + 1))
                t = np.concatenate([t[:at], aa[rng.integers(0, 20, size=int(rng.integers(1, 6)))], t[at:]]) if rng.random() < 0.5 else np.delete(t, slice(at, at + 3))
            t = np.concatenate([t, aa[rng.integers(0, 20, size=lb)]])[:lb]
        else:
            t = aa[rng.integers(0, 20, size=lb)]
        seqs += [a.tobytes(), t.tobytes()]
    return synth.sw_from_seqs(seqs)


def diverged(rng, a, subs=0.05, indels=2):
    """A copy of a with `subs` substitutions and `indels` indels of 1..5 symbols."""
    t = np.frombuffer(a, np.uint8).copy()
    hit = rng.random(t.size) < subs
    t[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    for k in range(indels):
        at = int(rng.integers(10, t.size - 10))
        t = np.concatenate([t[:at], ACGT[rng.integers(0, 4, size=int(rng.integers(1, 6)))], t[at:]]) if k % 2 == 0 else np.delete(t, slice(at, at + 3))
    return t.tobytes()


def long_targets():
    """150 against 20 000 with a diverged copy implanted, and the longest query against 3 000."""
    rng = np.random.default_rng(34)
    a = rand(rng, 150)
    big = rand(rng, 64 * T)
    # (the indels change the copy's length: the tail is cut so that the targets have exactly 20 000 and 3 000 symbols)
    return synth.sw_from_seqs([a, (rand(rng, 12000) + diverged(rng, a) + rand(rng, 8000))[:20000], big,
                               (rand(rng, 700) + diverged(rng, big, indels=6)[:2000] + rand(rng, 400))[:3000]])


def span_bytes(b, h, p):
    """-> (x, y): the bytes of pair p's span."""
    a0, b0 = int(b.off[2 * p]), int(b.off[2 * p + 1])
    x = b.bases[a0 + h["a_begin"][p]:a0 + h["a_end"][p] + 1].tobytes() if h["a_begin"][p] >= 0 and h["a_end"][p] >= h["a_begin"][p] else b""
    y = b.bases[b0 + h["b_begin"][p]:b0 + h["b_end"][p] + 1].tobytes() if h["b_begin"][p] >= 0 and h["b_end"][p] >= h["b_begin"][p] else b""
    return x, y
