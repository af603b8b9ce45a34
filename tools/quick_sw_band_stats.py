"""Timings of the banded fills with alignment statistics (agx_sw_batch_create_align_band_diag_stats), in the manner
of tools/quick_sw_band_diag.py and on its batches: 4 096 x 10 000 x 10 000 at w = 128, 65 536 x 150 x 150 at w = 16, and reads of
2 000 in windows of 60 000 around minus their start at w = 64.  Per mode, in one run:
  kernel only   the stats batch's forward fill beside the plain SPANS band-diag batch's: HIP events (agx_ctx_timer_*) round
                back-to-back launches after a warm-up, median and minimum of 7 rounds.  (LOCAL and FIT keep the plain forward fill:
                their statistics ride on the begin pass, which only the host clock below sees.)
  launch -> answer on the host clock, median of 3 after a warm-up: launch -> hits of the plain batch, launch -> stats of the stats
                batch, and launch -> cigars of the cigar batch on the same pairs -- what a caller who wants identities had to do.
Run on the GPU box; the output goes to profiles/sw_band_stats.md."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
from tests import sw_band_stats_ref as bs
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
def host_ms(dev, answer, rounds=3):
    dev.launch(); out = answer(); t = []
    for _ in range(rounds):
        t0 = time.perf_counter(); dev.launch(); out = answer(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), out
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
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens), None
def windows(n, la, lb, seed, sub=0.03):
    """n reads of la symbols planted in windows of lb; the centre is minus the plant's start"""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(n, la))]
    t = ACGT[rng.integers(0, 4, size=(n, lb))]
    start = rng.integers(100, lb - la - 100, size=n)
    for p in range(n):
        r = a[p].copy()
        hit = rng.random(la) < sub
        r[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
        t[p, start[p]:start[p] + la] = r
    bases = np.concatenate([a, t], axis=1).reshape(-1)
    lens = np.tile(np.array([la, lb], np.uint32), n)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens), (-start).astype(np.int32)
print("| batch | mode | w | plain fill ms, median (min) | stats batch's fill ms, median (min) | fill ratio | launch -> hits ms | launch -> stats ms | "
      "launch -> cigars ms | stats / cigars | mean identity |\n|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
slower = []
for name, make, w, reps, modes in (("4096 x 10000 x 10000", lambda: uniform(4096, 10000, 10000, 1), 128, 1, (1, 3, 0, 2, 4)),
                                   ("65536 x 150 x 150", lambda: uniform(65536, 150, 150, 2), 16, 10, (1, 3, 0, 2, 4)),
                                   ("2048 reads of 2000 in windows of 60000", lambda: windows(2048, 2000, 60000, 3), 64, 2, (2, 0))):
    b, diag = make()
    d = 0 if diag is None else diag
    for mode in modes:
        plain = ctx.sw_batch(b, mode=mode, align=agx.SW_ALIGN_SPANS, band=w, diag=d)
        kp = kernel_ms(plain, reps)
        hp, hits = host_ms(plain, plain.hits)
        plain.close()
        st = ctx.sw_batch(b, mode=mode, band=w, diag=d, band_stats=True)
        ks = kernel_ms(st, reps)
        hs, (shits, stats) = host_ms(st, st.stats)
        st.close()
        assert all(np.array_equal(hits[f], shits[f]) for f in hits.dtype.names), "the stats batch's hits differ from the plain batch's"
        cg = ctx.sw_batch(b, mode=mode, band=w, diag=d, cigar=True)
        hc, (chits, op_off, ops) = host_ms(cg, cg.cigars, rounds=1)
        cg.close()
        sample = np.arange(0, b.n_pairs, max(1, b.n_pairs // 256))
        cnt = np.zeros(sample.size, agx.SwStat)
        for k, p in enumerate(sample):
            o = ops[int(op_off[p]):int(op_off[p + 1])]
            cnt[k] = (int((o[(o & 15) == 7] >> 4).sum()), int((o[((o & 15) == 7) | ((o & 15) == 8)] >> 4).sum()))
        assert np.all(bs.lex_le(cnt, stats[sample])), "a CIGAR counts more than the stats"
        cols = (hits["a_end"] - hits["a_begin"] + 1).astype(np.int64) + (hits["b_end"] - hits["b_begin"] + 1) - stats["pairs"]
        ident = float(np.mean(stats["matches"][cols > 0] / cols[cols > 0])) if np.any(cols > 0) else 0.0
        print("| %s | %s | %d | %.3f (%.3f) | %.3f (%.3f) | %.2f | %.1f | %.1f | %.1f | %.2f | %.4f |"
              % (name, NAMES[mode], w, kp[0], kp[1], ks[0], ks[1], ks[0] / kp[0], hp, hs, hc, hs / hc, ident), flush=True)
        if hs >= hc: slower.append("%s, %s" % (name, NAMES[mode]))
    del b
print("\nlaunch -> stats does not beat launch -> cigars on: %s" % ("; ".join(slower) if slower else "no batch"), flush=True)
