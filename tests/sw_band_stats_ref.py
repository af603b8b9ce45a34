"""The CHECKER for the statistics of batches banded around a diagonal: tests/host/sw_band_stats_ref.c, a banded Gotoh with both
ends pinned over the span the band-diag checker reports (tests/sw_band_diag_ref.py), through in-band cells only, maximising the
tuple (score, matches, pairs) by definition -- include/agx.h, "Statistics for batches banded around a diagonal".  Compiled here
with the system compiler into a scratch directory and called through ctypes (which releases the GIL: batches are checked on several
cores).  Used by the tests only."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import accelerating_genomics_amd.api as agx
from tests import sw_band_diag_ref as bd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "sw_band_stats_ref.c")
REFERENCE_SCORING = bd.REFERENCE_SCORING
LOCAL, GLOBAL, FIT, EXTEND, EXTEND_QUERY = bd.MODES
MODES, MODE_NAMES = bd.MODES, bd.MODE_NAMES
_lib = None


def load():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="sw_band_stats_ref_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libsw_band_stats_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-shared", "-fPIC", "-Wall", "-Wextra", _SRC, "-o", so], check=True)
        l = C.CDLL(so)
        l.sw_band_stats_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def _diag(diag, n):
    return None if diag is None else np.ascontiguousarray(np.broadcast_to(np.asarray(diag, np.int32), (n,)))


def stats(b, h, band, diag=None, scoring=None, threads=None):
    """b: synth.SWBatch, h: its SwHit records inside the band -> (smax, smin): api.SwStat records, the answer of the contract and the
    lexicographic minimum over the same optimal in-band alignments."""
    from concurrent.futures import ThreadPoolExecutor

    n = b.n_pairs
    smax, smin = np.zeros(n, agx.SwStat), np.zeros(n, agx.SwStat)
    assert b.off.dtype == np.uint64 and b.len.dtype == np.uint32 and b.bases.dtype == np.uint8 and h.dtype == agx.SwHit
    h = np.ascontiguousarray(h)
    bases = b.bases if b.bases.size else np.zeros(1, np.uint8)
    sc = tuple(scoring) if scoring is not None else REFERENCE_SCORING
    d = _diag(diag, n)
    t = max(1, min(threads or bd._threads(), n // 16 or 1))
    cuts = np.linspace(0, n, 4 * t + 1).astype(np.int64)
    lib = load()

    def one(k):
        lo, hi = int(cuts[k]), int(cuts[k + 1])
        if hi <= lo:
            return
        rc = lib.sw_band_stats_ref(bases.ctypes.data, b.off[2 * lo:].ctypes.data, b.len[2 * lo:].ctypes.data, hi - lo, *sc, int(band),
                                   d[lo:].ctypes.data if d is not None else None, h[lo:].ctypes.data, smax[lo:].ctypes.data, smin[lo:].ctypes.data)
        assert rc == 0, "checker failed: %d (-2: the pinned in-band fill over the span does not give the hit's score; -3: a bad span)" % rc

    with ThreadPoolExecutor(t) as ex:
        list(ex.map(one, range(4 * t)))
    return smax, smin


def expected(b, mode, band, diag=None, scoring=None):
    """-> (hits, smax, smin) of a banded stats batch of `mode`, by definition."""
    h = bd.align(b, mode, band, diag, bd.SPANS, scoring)
    smax, smin = stats(b, h, band, diag, scoring)
    return h, smax, smin


def cigar_counts(op_off, ops):
    """(matches, pairs) per pair counted from CIGAR operations (length << 4 | BAM code; 7 '=', 8 'X')."""
    n = len(op_off) - 1
    out = np.zeros(n, agx.SwStat)
    for p in range(n):
        o = np.asarray(ops[int(op_off[p]):int(op_off[p + 1])], np.uint32)
        ln, code = (o >> 4).astype(np.int64), o & 15
        out[p] = (int(ln[code == 7].sum()), int(ln[(code == 7) | (code == 8)].sum()))
    return out


def lex_le(x, y):
    """x, y: SwStat arrays -> elementwise (x.matches, x.pairs) <= (y.matches, y.pairs) lexicographically."""
    return (x["matches"] < y["matches"]) | ((x["matches"] == y["matches"]) & (x["pairs"] <= y["pairs"]))
