"""The CHECKER for the CIGARs of batches banded around a diagonal under two-piece gap costs: tests/host/sw_band_dual_cigar_ref.c.
Spans come from the two-piece checker (tests/sw_band_dual_ref.py); the C helper then does a five-state Gotoh of every span's full
matrix with the explicit limits dlo' = c - w - delta, dhi' = c + w - delta (delta = a_begin - b_begin) and walks back exactly as
include/agx.h words it ("CIGARs for batches banded around a diagonal under two-piece gap costs").  Compiled here with the system
compiler into a scratch directory and called through ctypes (which releases the GIL: batches are checked on several cores).  Also
path_checks, which needs no checker: a path stays in its band, consumes its span and rescores to its score under the LITERAL
two-piece cost of every maximal run.  Used by the tests only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import accelerating_genomics_amd.api as agx
from tests import sw_band_dual_ref as dual_ref
from tests.sw_band_dual_ref import EXTEND, EXTEND_QUERY, FIT, GLOBAL, LOCAL, MODE_NAMES, MODES, S_MM2, SPANS, _threads, admits  # noqa: F401
from tests.sw_cigar_ref import OP_CHARS, OP_D, OP_EQ, OP_I, OP_X, spans, strings  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "sw_band_dual_cigar_ref.c")
_lib = None
SEEN_DIAGONAL, SEEN_SOURCES, SEEN_EXTENDED = 1, 0x1e, 0x1e0  # bits of `seen`: the diagonal move; H from E1, F1, E2, F2; a stay in each


def load():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="sw_band_dual_cigar_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libsw_band_dual_cigar_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-shared", "-fPIC", "-Wall", "-Wextra", _SRC, "-o", so], check=True)
        l = C.CDLL(so)
        l.sw_band_dual_cigar_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def _diag(diag, n):
    return np.zeros(n, np.int32) if diag is None else np.ascontiguousarray(np.broadcast_to(np.asarray(diag, np.int32), (n,)))


def cigars(b, h, band, diag=None, scoring=S_MM2, threads=None, seen=None):
    """b: synth.SWBatch, h: its two-piece band-diag SPANS SwHit records -> (op_off, ops) as agx_sw_batch_cigars lays them out.
    seen: a list that receives one int, the OR of what the walks met (SEEN_*)."""
    from concurrent.futures import ThreadPoolExecutor

    sc = np.array(tuple(scoring), np.int32)
    assert sc.size == 6
    n = b.n_pairs
    assert b.off.dtype == np.uint64 and b.len.dtype == np.uint32 and b.bases.dtype == np.uint8 and h.dtype == agx.SwHit
    h = np.ascontiguousarray(h)
    d = _diag(diag, n)
    bases = b.bases if b.bases.size else np.zeros(1, np.uint8)
    ca, cb = spans(h)
    slot = np.zeros(n + 1, np.uint64)
    slot[1:] = np.cumsum(ca + cb)
    wide = np.zeros(max(int(slot[n]), 1), np.uint32)
    count = np.zeros(max(n, 1), np.uint32)
    t = max(1, min(threads or _threads(), n // 4 or 1))
    cuts = np.linspace(0, n, 4 * t + 1).astype(np.int64)
    met = np.zeros(4 * t, np.uint32)
    lib = load()

    def one(k):
        lo, hi = int(cuts[k]), int(cuts[k + 1])
        if hi <= lo:
            return
        rc = lib.sw_band_dual_cigar_ref(bases.ctypes.data, b.off[2 * lo:].ctypes.data, b.len[2 * lo:].ctypes.data, hi - lo, sc.ctypes.data, int(band),
                                        d[lo:].ctypes.data, h[lo:].ctypes.data, slot[lo:].ctypes.data, wide.ctypes.data, count[lo:].ctypes.data,
                                        met[k:].ctypes.data)
        assert rc == 0, "checker failed: %d (-2: the banded fill over the span does not give the hit's score, -4: the path left the band)" % rc

    with ThreadPoolExecutor(t) as ex:
        list(ex.map(one, range(4 * t)))
    if seen is not None:
        seen.append(int(np.bitwise_or.reduce(met)))
    count = count[:n].astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(count, out=off[1:])
    take = np.repeat(slot[:n].astype(np.int64) - off[:n], count) + np.arange(int(off[n]), dtype=np.int64)
    return off.astype(np.uint64), wide[take]


def expected(b, mode, band, diag=None, scoring=S_MM2, seen=None):
    """-> (hits, op_off, ops) of a two-piece cigar batch banded around a diagonal, by definition."""
    h = dual_ref.align(b, mode, band, diag, SPANS, scoring)
    op_off, ops = cigars(b, h, band, diag, scoring, seen=seen)
    return h, op_off, ops


def gap_cost(ln, sc):
    """the literal two-piece cost of runs of length ln (an array)"""
    return np.maximum(sc[2] + ln * sc[3], sc[4] + ln * sc[5])


def path_checks(b, band, diag, hits, op_off, ops, scoring=S_MM2):
    """Independent of any checker, vectorised over the whole batch: every CIGAR is made of I, D, =, X runs of positive length
    with no two equal neighbours; run from its begin cell it stays within diag - band <= j - i <= diag + band of the full matrix
    after every operation, consumes exactly the span of its hit, every '=' / 'X' agrees with the symbols, and the operations
    rescore to the hit's score, every I or D run at the literal two-piece cost of its length.  Returns the first bad pair or -1."""
    sc = tuple(scoring)
    n = b.n_pairs
    op_off = np.asarray(op_off, np.int64)
    ops = np.asarray(ops, np.uint32)
    total = int(op_off[n])
    assert ops.size == total
    ca, cb = spans(hits)
    c = _diag(diag, n).astype(np.int64)
    a0 = np.maximum(hits["a_begin"].astype(np.int64), 0)
    b0 = np.maximum(hits["b_begin"].astype(np.int64), 0)
    cnt = np.diff(op_off)
    bad = np.zeros(n, bool)
    bad |= (cnt > 0) & ((a0 - b0 < c - band) | (a0 - b0 > c + band))  # the begin cell
    pair = np.repeat(np.arange(n), cnt)
    op = (ops & 15).astype(np.int64)
    ln = (ops >> 4).astype(np.int64)
    first = np.zeros(total, bool)
    first[op_off[:n][cnt > 0]] = True
    ok_op = np.isin(op, (OP_I, OP_D, OP_EQ, OP_X)) & (ln > 0)
    same_as_prev = np.zeros(total, bool)
    same_as_prev[1:] = (op[1:] == op[:-1]) & ~first[1:]
    np.logical_or.at(bad, pair, ~ok_op | same_as_prev)
    dj = np.where(op != OP_D, ln, 0)  # query symbols consumed
    di = np.where(op != OP_I, ln, 0)
    cj, ci = np.cumsum(dj), np.cumsum(di)
    base_j = np.concatenate([[0], cj])[op_off[:n]]
    base_i = np.concatenate([[0], ci])[op_off[:n]]
    j_end, i_end = cj - base_j[pair], ci - base_i[pair]  # after every operation, within the span
    d = (a0[pair] + j_end) - (b0[pair] + i_end)
    np.logical_or.at(bad, pair, (d < c[pair] - band) | (d > c[pair] + band))
    sum_j, sum_i = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(sum_j, pair, dj)
    np.add.at(sum_i, pair, di)
    bad |= (sum_j != ca) | (sum_i != cb)
    score = np.zeros(n, np.int64)
    np.add.at(score, pair, np.where((op == OP_I) | (op == OP_D), gap_cost(ln, sc), 0))
    diagonal = (op == OP_EQ) | (op == OP_X)
    if diagonal.any() and not bad.any():
        rl = ln[diagonal]
        rp = pair[diagonal]
        j0, i0 = (a0[pair] + j_end - dj)[diagonal], (b0[pair] + i_end - di)[diagonal]
        within = np.arange(int(rl.sum())) - np.repeat(np.cumsum(rl) - rl, rl)
        xp = np.repeat(b.off[0::2].astype(np.int64)[rp] + j0, rl) + within
        yp = np.repeat(b.off[1::2].astype(np.int64)[rp] + i0, rl) + within
        same = b.bases[xp] == b.bases[yp]
        want = np.repeat(op[diagonal] == OP_EQ, rl)
        pp = np.repeat(rp, rl)
        np.logical_or.at(bad, pp, same != want)
        np.add.at(score, pp, np.where(same, sc[0], sc[1]))
    if not bad.any():
        bad |= score != hits["score"]
    w = np.nonzero(bad)[0]
    return int(w[0]) if w.size else -1
