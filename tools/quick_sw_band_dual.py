"""Timings of the banded fills under two-piece gap costs (agx_sw_batch_create_align_band_diag_dual), in the manner
of tools/quick_sw_band_stats.py and on its two uniform batches: 4 096 x 10 000 x 10 000 at w = 128 and 65 536 x 150 x 150 at w = 16.
Per mode, kernel only: the two-piece batch's fill under (2, -4, -4, -2, -24, -1) beside the fill of the plain
agx_sw_batch_create_align_band_diag batch on the same pairs, band and diag under the first piece -- HIP events (agx_ctx_timer_*)
round back-to-back launches after a warm-up, median and minimum of 7 rounds; the ratio is taken between the minima.  The scores of
the two batches are compared on the way: the two-piece score is never below the one-piece one.
Run on the GPU box; the table goes into DESIGN.md 4.1n."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
NAMES = {0: "local", 1: "global", 2: "fit", 3: "extend", 4: "extend-query"}
S_MM2 = (2, -4, -4, -2, -24, -1)
def kernel_ms(dev, reps, rounds=7):
    for _ in range(2): dev.launch()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps): dev.launch()
        t.append(ctx.timer_stop() / reps)
    return statistics.median(t), min(t)
def uniform(n, la, lb, seed, sub=0.03):
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(n, la))]
    t = ACGT[rng.integers(0, 4, size=(n, lb))]
    m = min(la, lb)
    t[:, :m] = a[:, :m]
    hit = rng.random((n, lb), dtype=np.float32) < sub
    t[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    bases = np.concatenate([a, t], axis=1).reshape(-1)
    lens = np.tile(np.array([la, lb], np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens)
print("| batch | mode | w | launches, waves | plain fill ms, median (min) | two-piece fill ms, median (min) | ratio of the minima |\n|---|---|---|---|---|---|---|",
      flush=True)
for name, make, w, reps in (("4096 x 10000 x 10000", lambda: uniform(4096, 10000, 10000, 1), 128, 1),
                            ("65536 x 150 x 150", lambda: uniform(65536, 150, 150, 2), 16, 10)):
    b = make()
    for mode in (1, 3, 0, 2, 4):
        plain = ctx.sw_batch(b, scoring=S_MM2[:4], mode=mode, align=agx.SW_ALIGN_ENDS, band=w, diag=0)
        kp = kernel_ms(plain, reps)
        sp = plain.scores()
        plain.close()
        du = ctx.sw_batch(b, mode=mode, align=agx.SW_ALIGN_ENDS, band=w, diag=0, dual=S_MM2)
        kd = kernel_ms(du, reps)
        sd = du.scores()
        info = du.info()
        du.close()
        assert np.all(sd >= sp), "a two-piece score lies below the one-piece score"
        print("| %s | %s | %d | %d launches, %d waves | %.3f (%.3f) | %.3f (%.3f) | %.2f |"
              % (name, NAMES[mode], w, info.n_launches, info.n_waves, kp[0], kp[1], kd[0], kd[1], kd[1] / kp[1]), flush=True)
    del b
