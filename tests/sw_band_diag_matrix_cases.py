"""The inputs of the tiling sweep of banded alignment around a diagonal under a substitution matrix, shared by the CPU test that
confirms the checker's side of them and the GPU tests that run them (tests/test_sw_band_diag_matrix_*).  Protein pairs under
BLOSUM62; shapes chosen for where the banded fill can go wrong, not for a workload."""
import numpy as np

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_band_diag_matrix_ref as mr

# every K (4, 8, 16, 32 diagonals per lane) and G from 1 lane (first = last) to 64
WIDTHS = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 511, 1023)
LAS = (1, 3, 4, 5, 31, 33, 150, 300)
AMINO = np.frombuffer(synth.AMINO, np.uint8)
PINNED = (mr.GLOBAL, mr.EXTEND, mr.EXTEND_QUERY)


def blosum62():
    return agx.SwMatrix.build(synth.AMINO, synth.BLOSUM62, -11, -1)


def prot(rng, n):
    return AMINO[rng.integers(0, 20, size=n)].tobytes()


def substituted(rng, a, rate=0.1):
    """a with about `rate` of its residues replaced, the first one kept (a related pair of one residue stays an identity)"""
    out = bytearray(a)
    for k in range(1, len(out)):
        if rng.random() < rate:
            out[k] = AMINO[rng.integers(0, 20)]
    return bytes(out)


def with_indels(rng, a, n):
    """n single-residue insertions or deletions somewhere behind the first residues"""
    out = bytearray(a)
    for _ in range(n):
        if len(out) < 8:
            break
        k = int(rng.integers(4, len(out) - 2))
        if rng.random() < 0.5:
            del out[k]
        else:
            out.insert(k, AMINO[rng.integers(0, 20)])
    return bytes(out)


def sweep(mode, w, las=LAS, max_lb=700, seed=0):
    """-> (batch, centres int32, related bool): for every la and every residue of c mod 4 one related pair whose true diagonal is
    the centre (the read's copy stands at offset s = -c of the target, or the target's copy at offset c of the read), among tails
    of mixed length so that the groups of a wave have different row counts; unrelated pairs; a LOCAL pair whose band misses the
    matrix; pairs with an empty side.  FIT and LOCAL take centres down to -(max_lb - la), beyond -w (the first filled row is
    > 0), and LOCAL positive ones with la < c + w; the pinned modes hold the origin, |c| <= w, GLOBAL the corner too."""
    rng = np.random.default_rng(9000 + 31 * w + mode + seed)
    seqs, cs, rel = [], [], []

    def add(a, t, c, related):
        assert mr.admits(mode, len(a), len(t), c, w), (mode, w, len(a), len(t), c)
        seqs.extend([a, t])
        cs.append(c)
        rel.append(related)

    for la in las:
        for r in range(4):
            a = prot(rng, la)
            copy = substituted(rng, a)
            if w >= 8 and la >= 31 and mode != mr.GLOBAL:
                copy = with_indels(rng, copy, 2)  # (the path leaves the centre by at most two diagonals)
            if mode in PINNED:
                cands = [c for c in range(-w, w + 1) if c % 4 == r]
                c = int(cands[rng.integers(0, len(cands))]) if cands else 0
                if mode == mr.GLOBAL:  # the corner on the centre diagonal, or as near as the lengths allow
                    d = min(c, la - 1)
                    t = prot(rng, -d) + copy if d <= 0 else copy[d:]
                else:
                    s = max(0, -c)
                    head = prot(rng, c) if c > 0 else b""  # the read's copy of the target starts c residues into the read
                    a = head + a if la > 8 else a
                    t = prot(rng, s) + copy + prot(rng, int(rng.integers(0, max(1, max_lb - la - s) if r else 1)))
                    if mode == mr.EXTEND_QUERY and c + w < len(a) - len(t):
                        t += prot(rng, len(a) - len(t) - c - w)
                add(a, t, c, True)
                continue
            # FIT and LOCAL: the copy at offset s, c = -s in the residue asked for
            s = int(rng.integers(0, max(1, max_lb - la - 8)))
            if r == 1:
                s = w + 1 + (s % 40)  # c + w < 0: the first filled row is > 0
            s += (-s - r) % 4  # (-s) % 4 == r
            t = prot(rng, s) + copy + prot(rng, int(rng.integers(0, 60)))
            add(a, t, -s, True)
            if mode == mr.LOCAL and r >= 2:  # a positive centre: the target's copy stands c residues into the read
                c = int(rng.integers(1, 40))
                c += (r - c) % 4
                add(prot(rng, c) + a, copy + prot(rng, int(rng.integers(0, 30))), c, True)
        for _ in range(2):  # unrelated
            c = 0 if mode in PINNED else int(rng.integers(-60, 1))
            t = prot(rng, int(rng.integers(max(1, la - w), la + w + 1))) if mode == mr.GLOBAL else prot(rng, int(rng.integers(min(la + 60, max_lb - 1), max_lb)))
            add(prot(rng, la), t, c, False)
    if mode == mr.LOCAL:
        add(prot(rng, 5), prot(rng, 5), 5 + w + 3, False)  # the band misses the matrix
        add(prot(rng, 5), prot(rng, 5), -(5 + w + 3), False)
        add(prot(rng, 2), prot(rng, 40), 1 + w, False)  # la < c + w
    k = min(3, w)
    for la, lb in ((0, k), (k, 0), (0, 0)):
        add(prot(rng, la), prot(rng, lb), 0, False)
    return synth.sw_from_seqs(seqs), np.array(cs, np.int32), np.array(rel, bool)
