"""Timings of the banded fills around a diagonal (agx_sw_batch_create_align_band_diag): the batches of
tools/quick_sw_band.py (4 096 x 10 000 x 10 000 at w = 128, 65 536 x 150 x 150 at w = 16) in LOCAL, FIT and EXTEND_QUERY beside the
plain banded builds (agx_sw_batch_create_align_band, GLOBAL and EXTEND) on the same batches in the same run; one read-in-window
batch (4 096 reads of 2 000 in windows of 60 000 at w = 128, FIT around minus the read's offset) with the rows trimmed, and the
step count the same batch would have untrimmed; SPANS launch -> hits against ENDS on the host clock.
Kernel only where it says so: HIP events (agx_ctx_timer_*) round back-to-back launches after a warm-up, median and minimum of
7 rounds.  Run on the GPU box."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
NAMES = {0: "local", 1: "global", 2: "fit", 3: "extend", 4: "extend-query"}
def kernel_ms(dev, reps, rounds=7):
    for _ in range(2): dev.launch()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps): dev.launch()
        t.append(ctx.timer_stop() / reps)
    return statistics.median(t), min(t)
def uniform(n, la, lb, seed, sub=0.03, at=0):
    """n pairs of la x lb: b holds a (cut to fit) from offset `at` on, with `sub` substitutions; random elsewhere."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(n, la))]
    t = ACGT[rng.integers(0, 4, size=(n, lb))]
    m = min(la, lb - at)
    t[:, at:at + m] = a[:, :m]
    hit = rng.random((n, lb), dtype=np.float32) < sub
    t[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    bases = np.concatenate([a, t], axis=1).reshape(-1)
    lens = np.tile(np.array([la, lb], np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens)
def band_cells(la, lb, dlo, dhi):
    """In-band cells of one la x lb matrix, rows and columns 0 included."""
    i = np.arange(lb + 1)
    return int(np.maximum(np.minimum(la, i + dhi) - np.maximum(0, i + dlo) + 1, 0).sum())
def leg(name, b, mode, w, reps, diag=None, old=False):
    dev = ctx.sw_batch(b, mode=mode, band=w) if old else ctx.sw_batch(b, mode=mode, align=agx.SW_ALIGN_ENDS, band=w, diag=0 if diag is None else diag)
    k = kernel_ms(dev, reps)
    i = dev.info()
    chk = int(dev.hits()["score"].astype(np.int64).sum())
    dev.close()
    c = 0 if diag is None else int(diag)
    cells = band_cells(int(b.len[0]), int(b.len[1]), c - w, c + w) * b.n_pairs  # (uniform batches, one centre)
    print("%-24s %-12s %-9s w=%-4d kernel %.3f ms median %.3f min | %.1f G in-band cells/s at median (%.3g cells, %.3g issued, %d launches, %d waves) | score sum %d"
          % (name, NAMES[mode], "plain" if old else "diagonal", w, k[0], k[1], cells / k[0] / 1e6, cells, i.padded_cells, i.n_launches, i.n_waves, chk), flush=True)
    return i
def results_ms(b, mode, w, diag, what, rounds=7):
    """launch -> hits on the host clock, median of 7 after a warm-up"""
    dev = ctx.sw_batch(b, mode=mode, align=what, band=w, diag=diag)
    t = []
    for r in range(rounds + 1):
        ctx.sync()
        t0 = time.perf_counter()
        dev.launch()
        dev.hits()
        t.append((time.perf_counter() - t0) * 1e3)
    dev.close()
    return statistics.median(t[1:])
def spans_leg(name, b, w, diag):
    for mode in (agx.SW_MODE_FIT, agx.SW_MODE_LOCAL):
        e, s = results_ms(b, mode, w, diag, agx.SW_ALIGN_ENDS), results_ms(b, mode, w, diag, agx.SW_ALIGN_SPANS)
        print("%-24s %-12s w=%-4d launch -> hits, host clock: ENDS %.3f ms, SPANS %.3f ms (%.2f x)" % (name, NAMES[mode], w, e, s, s / e), flush=True)
for name, b, w, reps in (("4096 x 10000 x 10000", uniform(4096, 10000, 10000, 1), 128, 1), ("65536 x 150 x 150", uniform(65536, 150, 150, 2), 16, 10)):
    for mode in (agx.SW_MODE_GLOBAL, agx.SW_MODE_EXTEND):
        leg(name, b, mode, w, reps, old=True)
    for mode in (agx.SW_MODE_LOCAL, agx.SW_MODE_FIT, agx.SW_MODE_EXTEND_QUERY):
        leg(name, b, mode, w, reps)
    if b.n_pairs == 65536: spans_leg(name, b, w, 0)
    del b
# a read in a window: 2 000 symbols planted at offset 29 000 of 60 000, the band around minus the offset
win = uniform(4096, 2000, 60000, 3, at=29000)
i = leg("4096 x 2000 in 60000", win, agx.SW_MODE_FIT, 128, 3, diag=-29000)
K, G = 32, 9  # the tiling of 257 diagonals
print("%-24s steps per wave trimmed %d (issued cells / (64 K waves)), untrimmed lb + G = %d: %.1f x fewer [a count from the plan, not a time]"
      % ("", i.padded_cells // (64 * K * i.n_waves), 60000 + G, (60000 + G) / (i.padded_cells / (64 * K * i.n_waves))), flush=True)
spans_leg("4096 x 2000 in 60000", win, 128, -29000)
