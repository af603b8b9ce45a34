"""What the substitution-matrix cell costs in the two align fills (agx_sw_batch_create_align_matrix): per mode the ENDS fill
under a matrix next to the match/mismatch ENDS fill of the same mode -- the parent's kernels, whose code objects the matrix
builds do not touch -- on the same batch in the same run.  Kernel only: HIP events round back-to-back launches, minimum
(and median) of 7 rounds.  DNA batches run a match/mismatch matrix over the bytes present (the same scores: the score sums
must agree), the protein batch BLOSUM62 -11/-1 against the reference scoring on the same bytes.  The score-only pair (matrix
fill against the int32 fill) is printed for the same batches as the prior.  Run on the GPU box."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
NAMES = {agx.SW_MODE_LOCAL: "local", agx.SW_MODE_GLOBAL: "global", agx.SW_MODE_FIT: "fit", agx.SW_MODE_EXTEND: "extend", agx.SW_MODE_EXTEND_QUERY: "extend-query"}
REF = (1, -1, -3, -1)
def kernel_ms(dev, reps, rounds=7):
    for _ in range(3): dev.launch()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps): dev.launch()
        t.append(ctx.timer_stop() / reps)
    return statistics.median(t), min(t)
def leg(name, b, m, reps, same_scores):
    cells = b.cells()
    for mode in NAMES:
        dev = ctx.sw_batch(b, scoring=REF, align=agx.SW_ALIGN_ENDS, mode=mode); k0 = kernel_ms(dev, reps); s0 = int(dev.hits()["score"].astype(np.int64).sum()); dev.close()
        dev = ctx.sw_batch(b, matrix=m, align=agx.SW_ALIGN_ENDS, mode=mode); k1 = kernel_ms(dev, reps); s1 = int(dev.hits()["score"].astype(np.int64).sum()); dev.close()
        assert not same_scores or s0 == s1, (s0, s1)
        print("| %s | %s | %.4f (%.4f) | %.4f (%.4f) | %.0f | %.3f x | %d / %d |" % (name, NAMES[mode], k0[1], k0[0], k1[1], k1[0], cells / k1[1] / 1e6, k1[1] / k0[1], s0, s1), flush=True)
    ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_INT32)
    dev = ctx.sw_batch(b, scoring=REF); k0 = kernel_ms(dev, reps); dev.close()
    ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
    dev = ctx.sw_batch(b, matrix=m); k1 = kernel_ms(dev, reps); dev.close()
    print("| %s | score-only (int32 fill / matrix fill) | %.4f (%.4f) | %.4f (%.4f) | %.0f | %.3f x | |" % (name, k0[1], k0[0], k1[1], k1[0], cells / k1[1] / 1e6, k1[1] / k0[1]), flush=True)
def dna_matrix(b):
    alphabet = bytes(sorted(set(b.bases.tobytes())))
    n = len(alphabet)
    return agx.SwMatrix.build(alphabet, [[REF[0] if a == c else REF[1] for c in range(n)] for a in range(n)], REF[2], REF[3], case_insensitive=False)
print("| batch | mode | match/mismatch ENDS ms, min (median) | matrix ENDS ms, min (median) | matrix GCUPS at min | matrix / match-mismatch | score sums |\n|---|---|---|---|---|---|---|")
b = synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25)
leg("config 2", b, dna_matrix(b), 50, True)
b = synth.sw_pairs(65536, 32, 512, seed=4)
leg("mixed 32-512", b, dna_matrix(b), 10, True)
leg("protein ~150x150, BLOSUM62", synth.protein_pairs(65536, 150, 150, seed=2, related_frac=0.25), agx.SwMatrix.build(synth.AMINO, synth.BLOSUM62, -11, -1), 50, False)
