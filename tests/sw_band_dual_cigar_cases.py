"""What tests/test_sw_band_dual_cigar_cpu.py and tests/test_sw_band_dual_cigar_gpu.py share: the scoring of the small shapes, the
batches with adjacent planted gaps, and the child process that prints the plan digests of a two-piece cigar batch beside those of
the plain band-diag cigar batch on the same pairs:
    python tests/sw_band_dual_cigar_cases.py    (under AGX_TRACE_CREATE; stderr: "CASE name plain|dual" ahead of each create's lines)"""
import os
import re
import subprocess
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import accelerating_genomics_amd.synth as synth
from tests import sw_band_dual_cases as dc

# The pieces break even at L = 2 (-2 - 2L against -4 - L): piece 1 alone serves L = 1, piece 2 alone L >= 3, and at L = 2 they tie,
# so shapes of up to 10 x 10 meet piece 2, ties between the pieces and all five sources.
S_SMALL = (2, -4, -2, -2, -4, -1)
AC = np.frombuffer(b"AC", np.uint8)


def small(admits, mode, w, seed=1901, top=10):
    """len(a) x len(b) over 0..top x 0..top around every centre the mode admits at this w, over a two-letter alphabet."""
    rng = np.random.default_rng(seed)
    seqs, cs = [], []
    for la in range(top + 1):
        for lb in range(top + 1):
            for c in range(-lb - w - 1, la + w + 2):
                if not admits(mode, la, lb, c, w):
                    continue
                a = AC[rng.integers(0, 2, size=la)].tobytes()
                t = AC[rng.integers(0, 2, size=lb)].tobytes() if (la + lb + c) % 2 or not la else (a * (lb // la + 1))[:lb]
                seqs += [a, t]
                cs.append(c)
    return synth.sw_from_seqs(seqs), np.array(cs, np.int32)


def adjacent_gaps(seed=1902):
    """x + u + v + y against x + y (or the other way round), u of 1 .. 3 and v of 25 .. 40 random symbols, x and y random DNA of 50:
    two planted gaps with nothing between them are ONE run of len(u) + len(v) in any CIGAR.  -> (batch, the run's length per pair,
    1 where it is in a)"""
    rng = np.random.default_rng(seed)
    seqs, ls, in_a = [], [], []
    for k in range(48):
        x, y = dc._rand(rng, 50), dc._rand(rng, 50)
        u, v = dc._rand(rng, int(rng.integers(1, 4))), dc._rand(rng, int(rng.integers(25, 41)))
        mid = u + v if k % 4 < 2 else v + u
        a, t = (x + mid + y, x + y) if k % 2 == 0 else (x + y, x + mid + y)
        seqs += [a, t]
        ls.append(len(mid))
        in_a.append(1 - k % 2)
    return synth.sw_from_seqs(seqs), np.array(ls), np.array(in_a)


def run_digests():
    """One child process under AGX_TRACE_CREATE -> {name: {"plain" | "dual": the trace lines of that create, prefix stripped}}"""
    env = dict(os.environ, AGX_TRACE_CREATE="1")
    env.pop("AGX_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, timeout=600, env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-3000:]
    parts = re.split(r"^CASE (\w+) (\w+)\n", err, flags=re.M)[1:]
    out = {}
    for name, kind, text in zip(parts[0::3], parts[1::3], parts[2::3]):
        if name != "end":
            out.setdefault(name, {})[kind] = re.findall(r"^\[agx_sw_batch_create_band\] (.*)$", text, flags=re.M)
    return out


if __name__ == "__main__":
    import accelerating_genomics_amd.api as agx

    for case in dc.DIGEST_CASES:
        b, mode, w, diag = dc.digest_case(case)
        for kind, kw in (("plain", dict(scoring=dc.piece1(dc.S_MM2), cigar=True)), ("dual", dict(dual_cigar=dc.S_MM2))):
            sys.stderr.write("CASE %s %s\n" % (case, kind))
            sys.stderr.flush()
            agx.SwBatch(None, b, mode=mode, band=w, diag=diag, align=agx.SW_ALIGN_SPANS, **kw).close()
    sys.stderr.write("CASE end end\n")
