"""What the substitution-matrix build of the banded fill costs beside the match/mismatch build: the same DNA
batches, the same cells, once under a scoring and once under the ACGT matrix that restates it; the fill alone, timed with the
context's HIP-event stopwatch around `launches` launches of the resident batch, the two builds alternating within one process.
Two batches: one 10 000-base read in a 60 000-base window, FIT at w = 64; 2 000 pairs of 2 000 x 2 000, GLOBAL at w = 32.
Needs a GPU.   usage: python tools/sw_band_matrix_cost.py [--rounds N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import accelerating_genomics_amd.api as agx  # noqa: E402
import accelerating_genomics_amd.synth as synth  # noqa: E402

SCORING = (1, -1, -3, -1)
ACGT = np.frombuffer(b"ACGT", np.uint8)
FIT, GLOBAL = 2, 1


def mutated(rng, a, sub=0.04, indel=0.005):
    out = bytearray()
    for x in a:
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out.append(ACGT[rng.integers(0, 4)])
        out.append(x if rng.random() >= sub else ACGT[rng.integers(0, 4)])
    return bytes(out)


def batches():
    rng = np.random.default_rng(4112)
    read = ACGT[rng.integers(0, 4, size=10000)].tobytes()
    window = ACGT[rng.integers(0, 4, size=25000)].tobytes() + mutated(rng, read)
    window += ACGT[rng.integers(0, 4, size=60000 - len(window))].tobytes()
    one = (synth.sw_from_seqs([read, window]), FIT, 64, np.array([-25000], np.int32), 100)
    seqs = []
    for _ in range(2000):
        a = ACGT[rng.integers(0, 4, size=2000)].tobytes()
        t = mutated(rng, a)
        seqs += [a, (t + ACGT[rng.integers(0, 4, size=40)].tobytes())[:2000]]
    many = (synth.sw_from_seqs(seqs), GLOBAL, 32, np.zeros(2000, np.int32), 50)
    return {"read 10000 in window 60000, FIT, w = 64": one, "2000 pairs of 2000 x 2000, GLOBAL, w = 32": many}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = len(ACGT)
    matrix = agx.SwMatrix.build(b"ACGT", [[SCORING[0] if a == c else SCORING[1] for c in range(n)] for a in range(n)], SCORING[2], SCORING[3])
    result = {"device": agx.device_name(0) if hasattr(agx, "device_name") else "", "scoring": SCORING, "rounds": args.rounds, "batches": {}}
    with agx.Context(0) as ctx:
        for name, (b, mode, w, diag, launches) in batches().items():
            plain = ctx.sw_batch(b, scoring=SCORING, mode=mode, align=agx.SW_ALIGN_ENDS, band=w, diag=diag)
            mat = ctx.sw_batch(b, matrix=matrix, mode=mode, align=agx.SW_ALIGN_ENDS, band=w, diag=diag)
            try:
                for dev in (plain, mat):  # warm up, and the results must not differ
                    dev.launch()
                hp, hm = plain.hits(), mat.hits()
                assert all(np.array_equal(hp[f], hm[f]) for f in ("score", "a_end", "b_end")), "the two builds disagree"
                times = {"match/mismatch": [], "matrix": []}
                for _ in range(args.rounds):
                    for key, dev in (("match/mismatch", plain), ("matrix", mat)):
                        ctx.timer_start()
                        for _ in range(launches):
                            dev.launch()
                        times[key].append(ctx.timer_stop() / launches)
                info = plain.info()
                row = {"padded_cells": int(info.padded_cells), "n_waves": int(info.n_waves), "launches_per_window": launches,
                       "min_score": int(hp["score"].min())}
                for key, t in times.items():
                    t = np.array(t)
                    row[key] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "all_ms": [float(v) for v in t]}
                row["ratio_of_medians"] = row["matrix"]["median_ms"] / row["match/mismatch"]["median_ms"]
                result["batches"][name] = row
            finally:
                plain.close()
                mat.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
