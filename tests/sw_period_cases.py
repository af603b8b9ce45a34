"""The batches of tests/test_sw_period_gpu.py, built the same way in every process that scores them.

The test's own process scores the "natural" group on the shipped library.  Everything that needs a knob of the tuning build runs
this file as a program, in a child process: AGX_SW_FORCE_C pins the columns per lane (the planner on its own never tiles 28
columns as two lanes of 14, and gives a small batch narrow lanes), AGX_SW_PERIOD=4 forces the narrow kernel, AGX_TRACE_CREATE makes every create say which period it
runs.     usage: python tests/sw_period_cases.py GROUP OUT.npz      (stderr: "CASE name" ahead of each create's trace lines)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import accelerating_genomics_amd.synth as synth  # noqa: E402
from tests import sw_period_ref as pref  # noqa: E402

REF = (1, -1, -3, -1)           # the reference's scoring
GE3 = (12, -4, -10, -3)         # |ge| = 3, the wrap column's diagonal constant exactly 0 at period four
EDGE = (4, -1, -30, -5)         # a large |ge|: the wide rule's edge at a few thousand rows
NL = b"\n"
FORCED = {"c14": 14, "c38": 38, "c40": 40}  # group -> AGX_SW_FORCE_C
# group -> the knobs its child processes run under.  Small batches are planned for latency (narrow lanes, many of them): the
# mixed batch is planned for throughput, as a large one is, so that it reaches the one-launch kernel's wide classes.
KNOBS = dict({g: {"AGX_SW_FORCE_C": str(c)} for g, c in FORCED.items()}, natural={}, mixed={"AGX_SW_TAIL_BETA": "0"})
GROUPS = tuple(KNOBS)


def _rand(rng, alphabet, n):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def _related(rng, a, alphabet=b"ACGT"):
    b = bytearray(a)
    for _ in range(max(1, len(b) // 30)):
        pos = int(rng.integers(0, len(b)))
        b[pos:pos + int(rng.integers(0, 3))] = _rand(rng, alphabet, int(rng.integers(0, 3)))
    return bytes(b)


def _wave150(rng, n, with_n):
    """n pairs of 150 symbols and a final newline each: 4 lanes of 38 columns, 32 pairs to a wave."""
    seqs = []
    for k in range(n):
        a = _rand(rng, b"ACGT", 150)
        b = _related(rng, a)[:150].ljust(150, b"A") if k % 3 else _rand(rng, b"ACGT", 150)
        if with_n and k == 5:
            a = a[:70] + b"N" + a[71:]  # a fifth symbol: the pack kernel leaves this wave to the general cell
        seqs += [a + NL, b + NL]
    return seqs


def _rows(rng, rows):
    """150 columns (4 lanes of 38) against each of `rows` rows: steps = rows + 3, so 153 .. 156 leave 0 .. 3 tail steps."""
    seqs = []
    for r in rows:
        a = _rand(rng, b"ACGT", 150)
        y = _rand(rng, b"ACGT", max(0, r - 190)) + _related(rng, a)[-40:] + a  # the maximum is reached in the last rows
        seqs += [a, y[-r:]] if r % 2 else [y[-r:], a]
    return seqs


def _corners(rng, general):
    """The best cell in a chosen column of a lane: x has 150 symbols in 4 lanes of 38 columns -- DNA-coded waves hold x
    right-aligned (symbol i in column i + 2), general ones left-aligned (column i) --, y is unrelated to x but for a copy of
    x[:k], so that the only long diagonal ends in column k - 1 (+ 2).  Columns 19 (the wrap of period 19), 0 and 37 of a lane,
    and the last column of the last lane in the last step (y ends with the whole of x)."""
    ax, ay = (b"ARNDCQEG", b"HILKMFPS") if general else (b"AC", b"GT")
    shift = 0 if general else 2
    seqs = []
    for lane in range(4):
        for col in (19, 0, 37, 18, 20):
            k = 38 * lane + col - shift + 1
            if k < 8:
                continue
            x = _rand(rng, ax, 150)
            if general:
                x = ax + x[8:]
            seqs += [x, _rand(rng, ay, 30 + col) + x[:k] + _rand(rng, ay, 11 + lane)]
    x = _rand(rng, ax, 150)
    seqs += [x, _rand(rng, ay, 7) + x]                    # ... in the last step, no newline
    seqs += [x + NL, _rand(rng, ay, 9) + x + NL]          # ... and as the stripped sentinels' corner
    seqs += [x + NL, _rand(rng, ay, 9) + x[:-1] + b"T" + NL]
    return seqs


def _ties():
    """Every cell ties, or gaps and matches alternate: all-A against all-A, and x against x with every third symbol dropped,
    doubled, or replaced."""
    seqs = []
    for la, lb in ((150, 150), (150, 153), (151, 156), (38, 38), (14, 77)):
        seqs += [b"A" * la, b"A" * lb]
        seqs += [b"A" * la + NL, b"A" * lb + NL]
    x = b"ACGTTGCA" * 19
    seqs += [x[:150], bytes(c for i, c in enumerate(x[:156]) if i % 3)]
    seqs += [x[:150], b"".join(bytes([c, c]) if i % 3 == 0 else bytes([c]) for i, c in enumerate(x[:120]))]
    seqs += [x[:150], bytes(ord("T") if i % 3 == 0 else c for i, c in enumerate(x[:152]))]
    seqs += [b"AC" * 75, b"CA" * 78]
    seqs += [b"AAC" * 50 + NL, b"AC" * 80 + NL]
    return seqs


def _lane_groups(rng, C, lanes=(1, 2, 64)):
    """Columns per lane pinned at C: one full wave and a partly filled one (with a vacant half) of single-lane groups (no
    arrival), of groups of 2 and of 64 lanes; DNA, with and without final newlines, some pairs related, one group general."""
    seqs = []
    for G in lanes:
        full = (64 // G) * 2
        for k in range(full + max(1, full // 3) | 1):
            lx = int(rng.integers((G - 1) * C + 1, G * C + 1))
            ly = lx + int(rng.integers(0, 70))
            a = _rand(rng, b"ACGT", lx)
            y = _rand(rng, b"ACGT", ly - lx) + _related(rng, a)
            y = y[:ly] if len(y) >= ly else y + _rand(rng, b"ACGT", ly - len(y))
            if k % 4 == 1 and lx > 2:
                a, y = a[:-1] + NL, y[:-1] + NL
            if G == 2 and k == 3:
                a = a[:1] + b"N" + a[2:]
            seqs += [a, y] if k % 2 else [y, a]
    return seqs


def _short_rows(rng):
    """38 columns per lane pinned, longer sides of 1 .. 5 rows (one lane: steps 1 .. 5, a quad at most and every tail length) and
    of 153 .. 156 rows against 150 columns (4 lanes): the maxima rotate with 22 accumulators."""
    seqs = []
    for ly in (1, 2, 3, 4, 5):
        for lx in (1, min(ly, 3)):
            a = _rand(rng, b"ACGT", lx)
            seqs += [a, (_rand(rng, b"ACGT", ly) + a)[-ly:]]
    return seqs + _rows(rng, (153, 154, 155, 156, 200, 201, 202, 203))


def _edge(longest_rows):
    """One step inside the wide rule and one outside, at 38 columns per lane (period 19): the batch of tests/test_sw_range_gpu.py
    whose worst pair reaches match * ls in its last rows."""
    from tests.test_sw_range_gpu import ll_edge_batch

    L = pref.last_wide_ll(EDGE, 150, pref.period(38))
    b, _ = ll_edge_batch(EDGE, 150, L, L + longest_rows)
    return b


def cases(group):
    """-> [(name, scoring, SWBatch)]"""
    rng = np.random.default_rng({"natural": 81, "c14": 82, "c38": 83, "c40": 84, "mixed": 85}[group])
    out = []

    def add(name, scoring, seqs):
        out.append((name, scoring, synth.sw_from_seqs(seqs) if isinstance(seqs, list) else seqs))

    if group == "natural":  # 32 768 pairs: enough for the planner to give each pair 4 lanes of 38 columns on its own
        add("uniform150", REF, synth.sw_pairs(32768, 150, 150, seed=86, related_frac=0.25))
    elif group == "mixed":
        add("mixed4096", REF, synth.sw_pairs(4096, 32, 512, seed=85, related_frac=0.5))
    elif group == "c38":
        add("wave150", REF, _wave150(rng, 32, False))
        add("wave150_n", REF, _wave150(rng, 32, True))
        add("corners_dna", REF, _corners(rng, False))
        add("corners_general", REF, _corners(rng, True))
        add("ties_ref", REF, _ties())
        add("ties_ge3", GE3, _ties())
        add("short_rows", REF, _short_rows(rng))
        add("short_rows_ge3", GE3, _short_rows(rng))
        add("edge_inside", EDGE, _edge(0))
        add("edge_outside", EDGE, _edge(1))
    else:
        add("lane_groups", REF, _lane_groups(rng, FORCED[group]))
        # (match 12 on 64 lanes of 40 columns is beyond the biased kernel's range: 32 lanes)
        add("lane_groups_ge3", GE3, _lane_groups(rng, FORCED[group], (1, 2, 32)))
    return out


def main(group, path):
    import accelerating_genomics_amd.api as agx

    assert agx.LIB_PATH.endswith("libagx_tuning.so"), agx.LIB_PATH
    got = {}
    with agx.Context(0) as ctx:
        for name, scoring, b in cases(group):
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            dev = ctx.sw_batch(b, scoring)
            sys.stderr.write("LAUNCHES %d\n" % dev.info().n_launches)
            try:
                dev.launch()
                got[name] = dev.scores()
            finally:
                dev.close()
    np.savez(path, **got)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
