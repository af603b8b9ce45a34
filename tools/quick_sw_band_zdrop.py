"""Timings of the banded EXTEND fill with z-drop termination (agx_sw_batch_create_align_band_zdrop), in the manner
of tools/quick_sw_band_diag.py and on its batches.
1. Cost of the rule: the z-drop build at zdrop = SW_ZDROP_MAX (it never fires) beside the plain EXTEND build through
   agx_sw_batch_create_align_band_diag, same batch, same run: 4 096 x 10 000 x 10 000 at w = 128 and 65 536 x 150 x 150 at w = 16.
2. What termination saves: 4 096 pairs of 10 000 whose second half is unrelated, w = 128, (2, -4, -4, -2): zdrop = 100 beside
   zdrop = SW_ZDROP_MAX of the same build, with the steps the stops say a pair needs (a wave runs as long as its slowest pair).
Kernel only: HIP events (agx_ctx_timer_*) round back-to-back launches after a warm-up, median and minimum of 7 rounds.  Run on the
GPU box; the output goes to profiles/sw_band_zdrop.md."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
DNA = (2, -4, -4, -2)
def kernel_ms(dev, reps, rounds=7):
    for _ in range(2): dev.launch()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps): dev.launch()
        t.append(ctx.timer_stop() / reps)
    return statistics.median(t), min(t)
def uniform(n, la, lb, seed, sub=0.03, related=None):
    """n pairs of la x lb: b holds a with `sub` substitutions in its first `related` symbols (None: all), random behind them."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(n, la))]
    t = ACGT[rng.integers(0, 4, size=(n, lb))]
    m = min(la, lb) if related is None else related
    t[:, :m] = a[:, :m]
    hit = rng.random((n, lb), dtype=np.float32) < sub
    t[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    bases = np.concatenate([a, t], axis=1).reshape(-1)
    lens = np.tile(np.array([la, lb], np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens)
def tiling(width):
    """(K, G) of a band of `width` diagonals on long pairs (agx_sw_band.cpp, band_tiling with rows >> lanes)"""
    best = None
    for K in (32, 16, 8, 4):
        g = -(-width // K)
        if g <= 64 and (best is None or (5 + K) / (64 // g) < best[0]): best = ((5 + K) / (64 // g), K, g)
    return best[1], best[2]
def leg(name, b, w, reps, zdrop, scoring=None):
    dev = ctx.sw_batch(b, scoring=scoring, mode=agx.SW_MODE_EXTEND, align=agx.SW_ALIGN_ENDS, band=w, diag=0, zdrop=zdrop)
    k = kernel_ms(dev, reps)
    hits = dev.hits()
    stops = dev.zdrop_stops() if zdrop is not None else np.full(b.n_pairs, -1, np.int32)
    dev.close()
    K, G = tiling(2 * w + 1)
    lb = b.len[1::2].astype(np.int64)
    steps = np.where(stops >= 0, np.minimum(lb + G, (stops.astype(np.int64) + 1 + G + 3) // 4 * 4), lb + G)
    what = "plain extend" if zdrop is None else "zdrop=max" if zdrop == agx.SW_ZDROP_MAX else "zdrop=%d" % zdrop
    print("| %s | %s | %d | %.3f | %.3f | %d of %d | %.0f of %.0f | %d |"
          % (name, what, w, k[0], k[1], int(np.count_nonzero(stops >= 0)), b.n_pairs, steps.mean(), (lb + G).mean(), int(hits["score"].astype(np.int64).sum())),
          flush=True)
    return k[0], hits
HEAD = "| batch | build | w | kernel ms, median | min | pairs terminated | steps a pair needs, mean, of lb + G | score sum |\n|---|---|---|---|---|---|---|---|"
print("## 1. Cost of the rule: the z-drop build that never fires beside the plain EXTEND build\n\n" + HEAD, flush=True)
ratios = []
for name, b, w, reps in (("4096 x 10000 x 10000", uniform(4096, 10000, 10000, 1), 128, 1), ("65536 x 150 x 150", uniform(65536, 150, 150, 2), 16, 10)):
    p, hp = leg(name, b, w, reps, None)
    z, hz = leg(name, b, w, reps, agx.SW_ZDROP_MAX)
    assert all(np.array_equal(hp[f], hz[f]) for f in ("score", "a_end", "b_end")), "zdrop = max differs from the plain build"
    ratios.append("%s: z-drop build / plain build = %.3f" % (name, z / p))
    del b
print("\n" + "\n".join(ratios), flush=True)
print("\n## 2. What termination saves: the second half of every pair is unrelated, (2, -4, -4, -2)\n\n" + HEAD, flush=True)
half = uniform(4096, 10000, 10000, 4, related=5000)
full, _ = leg("4096 x 10000, half related", half, 128, 1, agx.SW_ZDROP_MAX, DNA)
cut, _ = leg("4096 x 10000, half related", half, 128, 1, 100, DNA)
print("\nzdrop = 100 / zdrop = max = %.3f" % (cut / full), flush=True)
