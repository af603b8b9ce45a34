"""Alignment-statistics timings (agx_sw_batch_create_align_stats) on config 2's batch and on a mixed batch, per mode next to
the plain SPANS batch of the same mode (entry points and code objects the stats builds do not touch) on the same batch in
the same run: kernel-only for what agx_sw_batch_launch queues (HIP events round back-to-back launches, minimum and median of
7 rounds -- in the modes GLOBAL, EXTEND and EXTEND_QUERY that is the stats fill, in LOCAL and FIT the plain forward fill:
their stats fill is the begin pass, which runs inside agx_sw_batch_stats) and launch -> results (host clock: one launch, the
fetch, the begin pass; stats() against hits()).  Run on the GPU box."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
NAMES = {agx.SW_MODE_LOCAL: "local", agx.SW_MODE_GLOBAL: "global", agx.SW_MODE_FIT: "fit", agx.SW_MODE_EXTEND: "extend", agx.SW_MODE_EXTEND_QUERY: "extend-query"}
def kernel_ms(dev, reps, rounds=7):
    for _ in range(3): dev.launch()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps): dev.launch()
        t.append(ctx.timer_stop() / reps)
    return statistics.median(t), min(t)
def e2e_ms(dev, fetch, rounds=9):
    for _ in range(2): dev.launch(); fetch()
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter(); dev.launch(); fetch(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)
def leg(name, b, reps):
    for mode in NAMES:
        sp = ctx.sw_batch(b, align=agx.SW_ALIGN_SPANS, mode=mode); ks = kernel_ms(sp, reps); es = e2e_ms(sp, sp.hits); want = sp.hits(); sp.close()
        st = ctx.sw_batch(b, mode=mode, stats=True); kt = kernel_ms(st, reps); et = e2e_ms(st, st.stats); hits, stats = st.stats(); st.close()
        assert all(np.array_equal(hits[f], want[f]) for f in want.dtype.names)
        print("%-8s %-13s kernel: SPANS %.4f ms min (%.4f median), stats %.4f (%.4f) = %.3f x | launch->results: SPANS %.3f ms median, stats %.3f = %.3f x | matches %d pairs %d"
              % (name, NAMES[mode], ks[1], ks[0], kt[1], kt[0], kt[1] / ks[1], es[0], et[0], et[0] / es[0], int(stats["matches"].astype(np.int64).sum()),
                 int(stats["pairs"].astype(np.int64).sum())), flush=True)
leg("config2", synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25), 50)
leg("mixed", synth.sw_pairs(65536, 32, 512, seed=4), 10)
