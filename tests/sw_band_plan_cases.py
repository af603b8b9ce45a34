"""The banded batches whose plans and images tests/golden/sw_band_plan_digests.json pins, built the same way in every process.

Each case is small and reaches another branch of agx_sw_host::create_band (csrc/agx_sw_band.cpp, csrc/agx_sw_band_plan.cpp); it is
named for that branch.  A case is created plan-only (no device) under the tuning build's AGX_TRACE_CREATE, whose lines say the kind
of batch, a hash of the plan (constants, launches, every wave and group record, first rows, diagonals, a cigar batch's tables),
what the plan is made of, and a hash of the image the fills read.  The child processes, their groups and the parsing are those of
tests/sw_plan_cases.py:     python tests/sw_band_plan_cases.py GROUP

record() runs every group and returns what the fixture holds; tools/record_sw_band_plan_digests.py writes it to the JSON."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import accelerating_genomics_amd.synth as synth  # noqa: E402
from tests import sw_plan_cases as pc  # noqa: E402

LOCAL, GLOBAL, FIT, EXTEND, EXTEND_QUERY = range(5)
MODE_NAMES = {LOCAL: "local", GLOBAL: "global", FIT: "fit", EXTEND: "extend", EXTEND_QUERY: "extend_query"}
ENDS, SPANS = 1, 2
GROUPS = ("default", "threads_1", "threads_3")  # of pc.GROUPS
# the cases a device creates as well (tests/test_sw_band_gpu.py): what is uploaded is what was hashed here
DEVICE_CASES = ("global_w8", "diag_fit_windows_spans", "cigar_matrix_local")


def _lens(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, size=n), rng.integers(lo, hi + 1, size=n)


def _dna(n, lo, hi, seed):
    la, lb = _lens(n, lo, hi, seed)
    return pc._from_lens(la, lb, seed + 1)


def _protein_from_lens(la, lb, seed):
    """pc._from_lens over the amino acids."""
    b = pc._from_lens(la, lb, seed)
    rng = np.random.default_rng(seed)
    return synth.SWBatch(np.frombuffer(synth.AMINO, np.uint8)[rng.integers(0, 20, size=b.bases.size)], b.off, b.len)


def _pinned(mode, what):
    """GLOBAL, EXTEND, EXTEND_QUERY around per-pair diagonals with |diag| <= band = 16, chosen so that the band holds what the
    mode pins: the origin, and GLOBAL's corner la - lb, or a cell of EXTEND_QUERY's column la (diag + band >= la - lb)."""

    def make():
        rng = np.random.default_rng(60 + mode)
        la = rng.integers(32, 301, size=200)
        lb = la + rng.integers(-10, 11, size=200)
        diff = la - lb
        lo = np.maximum(-16, diff - 16)
        hi = np.minimum(16, diff + 16) if mode == GLOBAL else np.full(200, 16)
        diag = lo + (rng.random(200) * (hi - lo + 1)).astype(np.int64)
        return pc._from_lens(la, lb, 61), dict(mode=mode, align=what, band=16, diag=diag)

    return make


def _fit_windows(**kw):
    """Reads in windows: a of 40..80 in b of 300..600 at diag = -offset, band 12.  The fills get the band's rows only (row0 > 0)."""

    def make():
        rng = np.random.default_rng(70)
        la, lb = rng.integers(40, 81, size=200), rng.integers(300, 601, size=200)
        offset = (rng.random(200) * (lb - la + 1)).astype(np.int64)
        return pc._from_lens(la, lb, 71), dict(mode=FIT, band=12, diag=-offset, **kw)

    return make


def _local_spread(what):
    """LOCAL with diagonals over -(lb + 20) .. la + 20 at band 8: some bands miss the matrix (no fill), some lie below the origin."""

    def make():
        la, lb = _lens(200, 32, 300, 80)
        rng = np.random.default_rng(81)
        diag = -(lb + 20) + (rng.random(200) * (la + lb + 41)).astype(np.int64)
        return pc._from_lens(la, lb, 82), dict(mode=LOCAL, align=what, band=8, diag=diag)

    return make


def _zdrop(with_diag, **kw):
    def make():
        b = _dna(200, 32, 300, 90)
        diag = np.random.default_rng(91).integers(-16, 17, size=200) if with_diag else None
        return b, dict(mode=EXTEND, band=16, zdrop=50, diag=diag, **kw)

    return make


def _protein(mode, matrix, **kw):
    """Protein pairs of 20..300 (FIT: the shorter one is a) around per-pair diagonals at band 10; under the matrix the image holds
    codes + 1, without it the same bytes as they are."""

    def make():
        la, lb = _lens(200, 20, 300, 100)
        rng = np.random.default_rng(101)
        if mode == FIT:
            la, lb = np.minimum(la, lb), np.maximum(la, lb)
            diag = -(rng.random(200) * (lb - la + 1)).astype(np.int64)
        else:
            diag = rng.integers(-30, 31, size=200)
        return _protein_from_lens(la, lb, 102), dict(mode=mode, band=10, diag=diag, matrix=matrix, **kw)

    return make


def _plain(make_batch, mode, w, **kw):
    return lambda: (make_batch(), dict(mode=mode, band=w, **kw))


_threads = _plain(lambda: _dna(5000, 32, 512, 120), GLOBAL, 12)

# (name, group, maker of (batch, keyword arguments of agx.SwBatch beyond the batch)) -- "matrix": True stands for BLOSUM62 -11/-1
CASES = [
    # GLOBAL widens the band by the length difference: widths 17 .. 285, several (K, G), every fpad
    ("global_w8", "default", _plain(lambda: _dna(300, 32, 300, 110), GLOBAL, 8)),
    ("extend_w16", "default", _plain(lambda: _dna(300, 32, 300, 111), EXTEND, 16)),
    # one diagonal: K = 4, G = 1, 64 groups a wave
    ("extend_w0_one_diagonal", "default", _plain(lambda: _dna(300, 32, 300, 112), EXTEND, 0)),
    # exactly 2048 diagonals (-1023 .. 1024): K = 32, G = 64, the group has its wave to itself
    ("global_2048_diagonals", "default", _plain(lambda: pc._from_lens([3000], [2999], 113), GLOBAL, 1023)),
    ("empty_0_pairs", "default", _plain(lambda: synth.sw_from_seqs([]), GLOBAL, 8)),
    ("empty_sides_only", "default", _plain(lambda: synth.sw_from_seqs([b"", b"ACGT", b"ACGT", b"", b"", b""] * 3), GLOBAL, 8)),
    ("empty_side_and_1x1", "default", _plain(lambda: synth.sw_from_seqs([b"", b"ACGT", b"A", b"C"]), GLOBAL, 8)),
] + [
    ("diag_%s_%s" % (MODE_NAMES[mode], wname), "default", _pinned(mode, what))
    for mode in (GLOBAL, EXTEND, EXTEND_QUERY) for what, wname in ((ENDS, "ends"), (SPANS, "spans"))
] + [
    ("diag_fit_windows_ends", "default", _fit_windows(align=ENDS)),
    ("diag_fit_windows_spans", "default", _fit_windows(align=SPANS)),
    ("diag_local_spread_ends", "default", _local_spread(ENDS)),
    ("diag_local_spread_spans", "default", _local_spread(SPANS)),
    # diag = None, 0 for every pair: api.SwBatch passes it on as NULL for a z-drop batch
    ("zdrop_diag_none", "default", _zdrop(False)),
    ("zdrop_diags", "default", _zdrop(True)),
    ("matrix_local", "default", _protein(LOCAL, True)),
    ("matrix_fit", "default", _protein(FIT, True)),
    # the same bytes without the matrix: the same plan up to the constants, another image
    ("protein_local_no_matrix", "default", _protein(LOCAL, False)),
    ("protein_fit_no_matrix", "default", _protein(FIT, False)),
    # the four cigar builds: the digest also covers band_rec, band_cls and band_G
    ("cigar_global_w8", "default", _plain(lambda: _dna(300, 32, 300, 110), GLOBAL, 8, cigar=True)),
    ("cigar_diag_fit_windows", "default", _fit_windows(cigar=True)),
    ("cigar_matrix_local", "default", _protein(LOCAL, True, cigar=True)),
    ("cigar_zdrop", "default", _zdrop(True, cigar=True)),
    # the image is built by every host thread, a range of groups each
    ("global_w12_5000", "default", _threads),
    ("global_w12_5000_threads1", "threads_1", _threads),
    ("global_w12_5000_threads3", "threads_3", _threads),
]
assert len({c[0] for c in CASES}) == len(CASES) and all(c[1] in GROUPS for c in CASES) and all(n in {c[0] for c in CASES} for n in DEVICE_CASES)


def create(agx, ctx, name):
    """The named case as an agx.SwBatch on ctx (None: plan only)."""
    b, kw = next(c for c in CASES if c[0] == name)[2]()
    if kw.get("matrix"):
        kw["matrix"] = pc._blosum()
    else:
        kw.pop("matrix", None)
    return agx.SwBatch(ctx, b, **kw)


_LINES = {
    "kind": r"kind: (mode -?\d+ band \d+ align \d+ at \d+ zdrop -?\d+ cigar \d+ matrix \d+)$",
    "digest": r"plan digest ([0-9a-f]{16})$",
    "fpad": r"plan parts: .*; fpad (\d+/\d+/\d+/\d+); ",
    "trimmed_rows": r"plan parts: .*; trimmed rows (\d+); ",
    "launch_k": r"plan parts: .*; launch K (.*)$",
    "image": r"image digest ([0-9a-f]{16}), first bad pair -1$",
}


def parse(stderr, infos):
    return pc.parse(stderr, infos, _LINES, "agx_sw_batch_create_band", tuple(_LINES))


def run_group(group, lib_path=None, names=None, device=False):
    """One child process -> (name -> fixture entry, its whole stderr)."""
    return pc.run_group(group, lib_path, names, device, script=__file__, parse=parse)


def record(lib_path=None):
    """Every case, plan-only -> what tests/golden/sw_band_plan_digests.json holds."""
    out = {}
    for group in GROUPS:
        out.update(run_group(group, lib_path)[0])
    return {c[0]: out[c[0]] for c in CASES}


if __name__ == "__main__":
    pc.main(sys.argv, cases=CASES, create=create)
