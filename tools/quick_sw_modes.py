"""Alignment-mode timings (agx_sw_batch_create_align_mode) on config 2's batch and on a mixed batch, next to the LOCAL ENDS
fill of the same build (the locating fill, whose code object the modes do not touch) on the same batches in the same run:
kernel-only (HIP events round back-to-back launches, minimum and median of 7 rounds) and, for SPANS in modes LOCAL and FIT,
launch -> results (host clock: one launch, the fetch, the begin pass).  Run on the GPU box."""
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
    cells = b.cells()
    base = None
    for mode in NAMES:
        dev = ctx.sw_batch(b, align=agx.SW_ALIGN_ENDS, mode=mode); k = kernel_ms(dev, reps); chk = int(dev.hits()["score"].astype(np.int64).sum()); dev.close()
        base = base or k
        print("%-8s ENDS %-13s kernel %.4f ms median %.4f min (%.0f GCUPS at min) | %.3f x local ENDS (min / min) | score sum %d"
              % (name, NAMES[mode], k[0], k[1], cells / k[1] / 1e6, k[1] / base[1], chk), flush=True)
    for mode in (agx.SW_MODE_LOCAL, agx.SW_MODE_FIT):
        dev = ctx.sw_batch(b, align=agx.SW_ALIGN_SPANS, mode=mode); e = e2e_ms(dev, dev.hits); dev.close()
        print("%-8s SPANS %-12s launch->results %.3f ms median %.3f min" % (name, NAMES[mode], e[0], e[1]), flush=True)
leg("config2", synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25), 50)
leg("mixed", synth.sw_pairs(65536, 32, 512, seed=4), 10)
