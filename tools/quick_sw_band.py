"""Banded-fill timings (agx_sw_batch_create_align_band): in-band cells per second of the fill on long pairs
(4 096 x 10 000 x 10 000 at w = 128, GLOBAL) and on reads (65 536 x 150 x 150 at w = 16, both modes), and beside them, in the same
run, the anchored fill (agx_sw_batch_create_align_mode, GLOBAL, ENDS) on 4 096 pairs of 2 560 x 10 000 in cells per second.
Kernel only: HIP events (agx_ctx_timer_*) round back-to-back launches after a warm-up, median and minimum of 7 rounds.
Run on the GPU box."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
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
    """n pairs of la x lb: b is a (cut or extended to lb) with `sub` substitutions."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(n, la))]
    t = ACGT[rng.integers(0, 4, size=(n, lb))]
    m = min(la, lb)
    t[:, :m] = a[:, :m]
    hit = rng.random((n, lb)) < sub
    t[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    bases = np.concatenate([a, t], axis=1).reshape(-1)
    lens = np.tile(np.array([la, lb], np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens)
def band_cells(b, mode, w):
    """In-band cells of the matrix, rows and columns 0 included, summed over the pairs."""
    la, lb = b.len[0::2].astype(np.int64), b.len[1::2].astype(np.int64)
    total = 0
    for x, y in set(zip(la.tolist(), lb.tolist())):
        diff = x - y if mode == agx.SW_MODE_GLOBAL else 0
        i = np.arange(y + 1)
        row = np.minimum(x, i + max(0, diff) + w) - np.maximum(0, i + min(0, diff) - w) + 1
        total += int(np.maximum(row, 0).sum()) * int(np.count_nonzero((la == x) & (lb == y)))
    return total
def band_leg(name, b, mode, w, reps):
    dev = ctx.sw_batch(b, mode=mode, band=w)
    k = kernel_ms(dev, reps)
    i = dev.info()
    chk = int(dev.hits()["score"].astype(np.int64).sum())
    dev.close()
    cells = band_cells(b, mode, w)
    print("%-22s %-6s w=%-4d kernel %.3f ms median %.3f min | %.1f G in-band cells/s at median (%.3g cells, %.3g issued, %d launches, %d waves) | score sum %d"
          % (name, "global" if mode == agx.SW_MODE_GLOBAL else "extend", w, k[0], k[1], cells / k[0] / 1e6, cells, i.padded_cells, i.n_launches, i.n_waves, chk), flush=True)
def anch_leg(name, b, reps):
    dev = ctx.sw_batch(b, align=agx.SW_ALIGN_ENDS, mode=agx.SW_MODE_GLOBAL)
    k = kernel_ms(dev, reps)
    chk = int(dev.hits()["score"].astype(np.int64).sum())
    dev.close()
    print("%-22s anchored global ENDS kernel %.3f ms median %.3f min | %.1f G cells/s at median (%.3g cells) | score sum %d"
          % (name, k[0], k[1], b.cells() / k[0] / 1e6, b.cells(), chk), flush=True)
long_pairs = uniform(4096, 10000, 10000, 1)
band_leg("4096 x 10000 x 10000", long_pairs, agx.SW_MODE_GLOBAL, 128, 1)
del long_pairs
reads = uniform(65536, 150, 150, 2)
band_leg("65536 x 150 x 150", reads, agx.SW_MODE_GLOBAL, 16, 10)
band_leg("65536 x 150 x 150", reads, agx.SW_MODE_EXTEND, 16, 10)
anch_leg("65536 x 150 x 150", reads, 10)
del reads
anch_leg("4096 x 2560 x 10000", uniform(4096, 2560, 10000, 3), 1)
