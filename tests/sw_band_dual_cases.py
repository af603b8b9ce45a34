"""What tests/test_sw_band_dual_cpu.py and tests/test_sw_band_dual_gpu.py share: the scorings of the two-piece tests, the batches
with planted gaps (whose properties the CPU test confirms with the checker alone before the GPU test relies on them), and the
child process that prints the plan digests of a two-piece batch beside those of the plain batch on the same pairs:
    python tests/sw_band_dual_cases.py      (under AGX_TRACE_CREATE; stderr: "CASE name plain|dual" ahead of each create's lines)"""
import os
import re
import subprocess
import sys

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import accelerating_genomics_amd.synth as synth

LOCAL, GLOBAL, FIT, EXTEND, EXTEND_QUERY = 0, 1, 2, 3, 4
ACGT = np.frombuffer(b"ACGT", np.uint8)
S_MM2 = (2, -4, -4, -2, -24, -1)  # the pieces break even at a gap of 20
S_SWAP = (2, -4, -24, -1, -4, -2)
S_EDGE = (12, -116, -1000, -1000, -1000, 0)
S_ZERO = (1, 0, 0, 0, 0, 0)
BREAK_EVEN = 20


def piece1(s):
    return s[:4]


def piece2(s):
    return (s[0], s[1], s[4], s[5])


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


PLANTED_SEED = 1801


def planted_gaps(seed=PLANTED_SEED):
    """x + ins(L) + y against x + y, x and y random DNA of 60, L = 1 .. 48, four pairs per L: the insertion stands in a for two of
    them (a gap along a: F, handed to the right) and in b for the other two (a gap along b: E, handed to the left).
    -> (batch, L per pair, 1 where the insertion is in a)"""
    rng = np.random.default_rng(seed)
    seqs, ls, in_a = [], [], []
    for L in range(1, 49):
        for k in range(4):
            x, y, ins = _rand(rng, 60), _rand(rng, 60), _rand(rng, L)
            a, t = (x + ins + y, x + y) if k % 2 == 0 else (x + y, x + ins + y)
            seqs += [a, t]
            ls.append(L)
            in_a.append(1 - k % 2)
    return synth.sw_from_seqs(seqs), np.array(ls), np.array(in_a)


BOTH_SEED = 1811


def both_pieces(seed=BOTH_SEED, n_pairs=64):
    """One planted gap of 1 .. 3 and one of 30 .. 60 in every pair, each on a side of its own choosing, flanks and middle of
    50 .. 70 symbols, no substitutions.  -> batch"""
    rng = np.random.default_rng(seed)
    seqs = []
    for p in range(n_pairs):
        x, y, z = (_rand(rng, int(rng.integers(50, 71))) for _ in range(3))
        g = [_rand(rng, int(rng.integers(1, 4))), _rand(rng, int(rng.integers(30, 61)))]
        if p % 2:
            g.reverse()  # the long gap first
        side = [int(rng.integers(0, 2)), int(rng.integers(0, 2))]
        a = x + (g[0] if side[0] == 0 else b"") + y + (g[1] if side[1] == 0 else b"") + z
        t = x + (g[0] if side[0] == 1 else b"") + y + (g[1] if side[1] == 1 else b"") + z
        seqs += [a, t]
    return synth.sw_from_seqs(seqs)


# ---- the digests' child process

DIGEST_CASES = {
    # name: (lengths lo, hi, pairs, mode, band, centre spread, seed)
    "fit_w16": (20, 300, 200, FIT, 16, 0, 1821),
    "local_w40_spread": (20, 400, 150, LOCAL, 40, 30, 1822),
    "global_w300": (500, 700, 40, GLOBAL, 300, 0, 1823),
    "extend_w0": (1, 200, 100, EXTEND, 0, 0, 1824),
    "extend_query_w1023": (2000, 2600, 4, EXTEND_QUERY, 1023, 0, 1825),
}


def digest_case(name):
    lo, hi, n, mode, w, spread, seed = DIGEST_CASES[name]
    rng = np.random.default_rng(seed)
    seqs, diag = [], []
    for p in range(n):
        a = _rand(rng, int(rng.integers(lo, hi + 1)))
        t = a if mode in (GLOBAL, EXTEND_QUERY) else _rand(rng, int(rng.integers(0, 40))) + a + _rand(rng, int(rng.integers(0, 40)))
        if p % 17 == 0:  # an empty side (a short enough for every mode's band condition)
            a, t = a[:min(3, w)], b""
        seqs += [a, t]
        diag.append(int(rng.integers(-spread, spread + 1)) if mode == LOCAL else 0)
    return synth.sw_from_seqs(seqs), mode, w, np.array(diag, np.int32)


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

    for case in DIGEST_CASES:
        b, mode, w, diag = digest_case(case)
        for kind, kw in (("plain", dict(scoring=piece1(S_MM2))), ("dual", dict(dual=S_MM2))):
            sys.stderr.write("CASE %s %s\n" % (case, kind))
            sys.stderr.flush()
            agx.SwBatch(None, b, mode=mode, band=w, diag=diag, align=agx.SW_ALIGN_SPANS, **kw).close()
    sys.stderr.write("CASE end end\n")
