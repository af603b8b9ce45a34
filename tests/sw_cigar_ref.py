"""The CHECKER for CIGARs: tests/host/sw_cigar_ref.c, the three full matrices of the pinned Gotoh recurrence over the span
the existing checkers report (sw_align_ref, sw_modes_ref, sw_matrix_align_ref) and the walk back from the corner exactly as
include/agx.h words it ("Alignment itself").  Compiled here with the system compiler into a scratch directory and called
through ctypes (which releases the GIL: batches are checked on several cores).  Used by the tests only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import accelerating_genomics_amd.api as agx
from tests.sw_stats_ref import EXTEND, EXTEND_QUERY, FIT, GLOBAL, LOCAL, MODE_NAMES, MODES, REFERENCE_SCORING, _threads, hits  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "sw_cigar_ref.c")
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OP_CHARS = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
_lib = None


def load():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="sw_cigar_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libsw_cigar_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-shared", "-fPIC", "-Wall", "-Wextra", _SRC, "-o", so], check=True)
        l = C.CDLL(so)
        l.sw_cigar_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def spans(h):
    """-> (ca, cb): the consumed lengths of every hit."""
    ca = np.where((h["a_begin"] >= 0) & (h["a_end"] >= h["a_begin"]), h["a_end"].astype(np.int64) - h["a_begin"] + 1, 0)
    cb = np.where((h["b_begin"] >= 0) & (h["b_end"] >= h["b_begin"]), h["b_end"].astype(np.int64) - h["b_begin"] + 1, 0)
    return ca, cb


def scoring_args(scoring=None, matrix=None):
    """-> ((match, mismatch, gap_open, gap_extend), score table or None, code map or None) as the C checkers take them."""
    if matrix is not None:
        score = np.ascontiguousarray(np.ctypeslib.as_array(matrix.score), np.int8).reshape(32, 32).copy()
        code = np.ascontiguousarray(np.ctypeslib.as_array(matrix.code), np.uint8).copy()
        code[code >= matrix.n_symbols] = 0xff
        return (0, 0, matrix.gap_open, matrix.gap_extend), score, code
    return (tuple(scoring) if scoring is not None else REFERENCE_SCORING), None, None


def cigars(b, h, scoring=None, matrix=None, threads=None):
    """b: synth.SWBatch, h: its SwHit records -> (op_off, ops): uint64[n + 1], uint32[op_off[n]] as agx_sw_batch_cigars lays them out."""
    from concurrent.futures import ThreadPoolExecutor

    n = b.n_pairs
    assert b.off.dtype == np.uint64 and b.len.dtype == np.uint32 and b.bases.dtype == np.uint8 and h.dtype == agx.SwHit
    h = np.ascontiguousarray(h)
    bases = b.bases if b.bases.size else np.zeros(1, np.uint8)
    sc, score, code = scoring_args(scoring, matrix)
    sp, cp = (score.ctypes.data, code.ctypes.data) if matrix is not None else (None, None)
    ca, cb = spans(h)
    slot = np.zeros(n + 1, np.uint64)
    slot[1:] = np.cumsum(ca + cb)
    wide = np.zeros(max(int(slot[n]), 1), np.uint32)
    count = np.zeros(max(n, 1), np.uint32)
    t = max(1, min(threads or _threads(), n // 16 or 1))
    cuts = np.linspace(0, n, 4 * t + 1).astype(np.int64)
    lib = load()

    def one(k):
        lo, hi = int(cuts[k]), int(cuts[k + 1])
        if hi <= lo:
            return
        rc = lib.sw_cigar_ref(bases.ctypes.data, b.off[2 * lo:].ctypes.data, b.len[2 * lo:].ctypes.data, hi - lo, *sc, sp, cp,
                              h[lo:].ctypes.data, slot[lo:].ctypes.data, wide.ctypes.data, count[lo:].ctypes.data)
        assert rc == 0, "checker failed: %d (-2: the pinned fill over the span does not give the hit's score)" % rc

    with ThreadPoolExecutor(t) as ex:
        list(ex.map(one, range(4 * t)))
    count = count[:n].astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(count, out=off[1:])
    take = np.repeat(slot[:n].astype(np.int64) - off[:n], count) + np.arange(int(off[n]), dtype=np.int64)
    return off.astype(np.uint64), wide[take]


def expected(b, mode, scoring=None, matrix=None):
    """-> (hits, op_off, ops) of a cigar batch of `mode`, by definition."""
    h = hits(b, mode, scoring, matrix)
    op_off, ops = cigars(b, h, scoring, matrix)
    return h, op_off, ops


def strings(op_off, ops):
    """One CIGAR string per pair, '*' for zero operations."""
    out = []
    for p in range(len(op_off) - 1):
        o = ops[int(op_off[p]):int(op_off[p + 1])]
        out.append("".join("%d%s" % (int(v) >> 4, OP_CHARS[int(v) & 15]) for v in o) or "*")
    return out


def host_checks(x, y, ops, score, scoring=None, matrix=None):
    """The five checks the library applies to one CIGAR before it returns it (x, y: the span's bytes; corner == score is the
    caller's): the operations consume exactly x and y, every '=' / 'X' agrees with the symbols, no two neighbouring runs share
    an op, and rescoring gives `score`."""
    sc, table, code = scoring_args(scoring, matrix)
    i = j = total = 0
    prev = 0
    for v in ops:
        op, ln = int(v) & 15, int(v) >> 4
        if ln == 0 or op == prev:
            return False
        prev = op
        if op in (OP_EQ, OP_X):
            if j + ln > len(x) or i + ln > len(y):
                return False
            for _ in range(ln):
                if matrix is not None:
                    same = code[x[j]] == code[y[i]]
                    total += int(table[code[x[j]], code[y[i]]])
                else:
                    same = x[j] == y[i]
                    total += sc[0] if same else sc[1]
                if same != (op == OP_EQ):
                    return False
                i, j = i + 1, j + 1
        elif op == OP_I:
            j += ln
            total += sc[2] + ln * sc[3]
        elif op == OP_D:
            i += ln
            total += sc[2] + ln * sc[3]
        else:
            return False
    return i == len(y) and j == len(x) and total == score
