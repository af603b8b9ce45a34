"""The CHECKER for align batches under a substitution matrix: tests/host/sw_matrix_align_ref.c, a full-matrix Gotoh that
applies the tables of include/agx.h ("Alignment coordinates", "Alignment modes") by definition with a 32 x 32 matrix and a
256-byte code map, compiled here with the system compiler into a scratch directory and called through ctypes (which
releases the GIL: batches are checked on several cores).  Used by the tests only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import accelerating_genomics_amd.api as agx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "sw_matrix_align_ref.c")
ENDS, SPANS = 1, 2
LOCAL, GLOBAL, FIT, EXTEND, EXTEND_QUERY = 0, 1, 2, 3, 4
MODES = (LOCAL, GLOBAL, FIT, EXTEND, EXTEND_QUERY)
MODE_NAMES = {LOCAL: "local", GLOBAL: "global", FIT: "fit", EXTEND: "extend", EXTEND_QUERY: "extend-query"}
_lib = None


def load():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="sw_matrix_align_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libsw_matrix_align_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-shared", "-fPIC", "-Wall", "-Wextra", _SRC, "-o", so], check=True)
        l = C.CDLL(so)
        l.sw_matrix_align_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = l
    return _lib


def match_matrix(alphabet: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int):
    """The api.SwMatrix that says what (match, mismatch, gap_open, gap_extend) says over `alphabet` (bytes compared as given)."""
    n = len(alphabet)
    return agx.SwMatrix.build(alphabet, [[match if a == c else mismatch for c in range(n)] for a in range(n)], gap_open, gap_extend,
                              case_insensitive=False)


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


def _one(b, lo, hi, score, code, go, ge, mode, what, out):
    if hi <= lo:
        return
    bases = b.bases if b.bases.size else np.zeros(1, np.uint8)
    rc = load().sw_matrix_align_ref(bases.ctypes.data, b.off[2 * lo:].ctypes.data, b.len[2 * lo:].ctypes.data, hi - lo, score.ctypes.data,
                                    code.ctypes.data, go, ge, mode, what, out[lo:].ctypes.data)
    assert rc == 0, ("checker failed: %d (-2: the reversed problem does not give the begin cell of the definition, "
                     "-4: a byte outside the alphabet)" % rc)


def align(b, matrix, mode, what=SPANS, threads=None):
    """b: synth.SWBatch, matrix: api.SwMatrix -> api.SwHit records, by definition."""
    from concurrent.futures import ThreadPoolExecutor

    n = b.n_pairs
    out = np.empty(n, agx.SwHit)
    assert b.off.dtype == np.uint64 and b.len.dtype == np.uint32 and b.bases.dtype == np.uint8
    score = np.ascontiguousarray(np.ctypeslib.as_array(matrix.score), np.int8).reshape(32, 32).copy()
    code = np.ascontiguousarray(np.ctypeslib.as_array(matrix.code), np.uint8).copy()
    code[code >= matrix.n_symbols] = 0xff
    t = max(1, min(threads or _threads(), n // 64 or 1))
    cuts = np.linspace(0, n, 4 * t + 1).astype(np.int64)
    load()
    with ThreadPoolExecutor(t) as ex:
        list(ex.map(lambda k: _one(b, int(cuts[k]), int(cuts[k + 1]), score, code, matrix.gap_open, matrix.gap_extend, mode, what, out), range(4 * t)))
    return out


def align_seqs(seqs, matrix, mode, what=SPANS):
    """[a0, b0, a1, b1, ...] as bytes -> list of (score, a_begin, a_end, b_begin, b_end)."""
    import accelerating_genomics_amd.synth as synth

    return [tuple(int(v) for v in h) for h in align(synth.sw_from_seqs(seqs), matrix, mode, what)]
