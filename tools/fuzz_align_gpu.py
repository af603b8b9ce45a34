#!/usr/bin/env python3
"""Seeded sweep of every alignment family on the GPU box, open-ended: cases drawn by tests/sw_fuzz_cases.py (mode, scoring or
matrix or two gap pieces, alphabet, lengths, band, centre per pair, z-drop and batch size, jointly) through the batch, its
relaunch, the one-shot entry, two half batches and one pair alone, against the by-definition checkers; every comparison exact.
usage: python tools/fuzz_align_gpu.py [seconds] [seed] [family]          k = 0, 1, 2, ... round the families until the time is up
       python tools/fuzz_align_gpu.py --case family seed k [pair] [--bytes]   one case again (the line a failing test prints)
Prints FUZZ_ALIGN_OK with the cases per family.  A mismatch is written out -- the pair's two sequences in hex, the arguments, and
whether the pair ALONE reproduces it (run once, in a batch of its own) -- and ends the run with status 1.  Any HIP error or other
failure ends the run at once: nothing further is launched and nothing is run again."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accelerating_genomics_amd.api as agx  # noqa: E402
from tests import sw_fuzz_cases as fc  # noqa: E402


def _show(v):
    if isinstance(v, agx.SwMatrix):
        mapped = [x for x in range(256) if v.code[x] != 0xff]
        rows = [[int(v.score[a][c]) for c in range(v.n_symbols)] for a in range(v.n_symbols)]
        return "matrix(n=%d gap_open=%d gap_extend=%d bytes=%s scores=%s)" % (v.n_symbols, v.gap_open, v.gap_extend, bytes(mapped).hex(), rows)
    return repr(v)


def report(ctx, e):
    """the mismatch, the pair's inputs, and one run of the pair alone"""
    case, p = e.case, e.pair
    print("MISMATCH %s" % e, flush=True)
    print("  a = %s\n  b = %s" % (case.batch.seq(2 * p).hex(), case.batch.seq(2 * p + 1).hex()))
    sub, kw, _ = fc.take(case.batch, e.kw, None, [p])  # the arguments of the step that differed: a twin's are the other entry's
    for name, v in sorted(kw.items()):
        print("  %s = %s" % (name, _show(v)))
    if case.bad_pair is None:
        alone = fc.differ(fc.device(ctx, sub, kw), fc.reference(sub, kw))
        print("  the pair alone: %s" % ("agrees with the checker: the batch around it matters" if alone is None else
                                        "reproduces it (%s: got %s, want %s)" % (alone[0], alone[2], alone[3])), flush=True)


def main(argv):
    ctx = agx.Context(0)
    if argv[:1] == ["--case"]:
        fixed = dict(alphabet="01..ff", plant=False) if "--bytes" in argv else {}  # a case of test_every_byte_but_zero_is_a_symbol
        case = fc.draw(argv[1], int(argv[2]), int(argv[3]), **fixed)
        try:
            n = fc.check_case(ctx, case)
        except fc.Mismatch as e:
            report(ctx, e)
            return 1
        print("FUZZ_ALIGN_OK %s seed %d k %d: %d comparisons, %d pairs" % (case.family, case.seed, case.k, n, case.batch.n_pairs))
        return 0
    budget = float(argv[0]) if argv else 60.0
    seed = int(argv[1]) if len(argv) > 1 else 1
    families = [argv[2]] if len(argv) > 2 else list(fc.FAMILIES)
    assert all(f in fc.FAMILIES for f in families), "families: %s" % " ".join(fc.FAMILIES)
    t_end = time.time() + budget
    count = {f: 0 for f in families}
    k = 0
    while time.time() < t_end:
        for f in families:
            if time.time() >= t_end:
                break
            try:
                fc.check_case(ctx, fc.draw(f, seed, k))
            except fc.Mismatch as e:
                report(ctx, e)
                return 1
            count[f] += 1
        k += 1
    print("FUZZ_ALIGN_OK seed %d: %s" % (seed, " ".join("%s=%d" % (f, count[f]) for f in families)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
