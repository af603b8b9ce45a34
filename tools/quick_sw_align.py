"""Alignment-coordinate timings (agx_sw_batch_create_align) on config 2's batch and on a mixed batch, next to the score-only
int32 leg of the same build: kernel-only (HIP events round back-to-back launches) and launch -> results (host clock, one
launch and the fetch; for SPANS this holds the begin pass: end cells to the host, reversed prefixes, second fill).
Median and minimum of the repeats.  The begin pass's kernel is timed on its own through an ENDS batch of the reversed
prefixes, built here from the forward hits.  Run on the GPU box."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
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
def reversed_prefixes(b, hits):
    seqs = []
    for p in np.nonzero(hits["score"] > 0)[0]:
        seqs += [b.seq(2 * p)[: hits["a_end"][p] + 1][::-1], b.seq(2 * p + 1)[: hits["b_end"][p] + 1][::-1]]
    return synth.sw_from_seqs(seqs)
def leg(name, b, reps):
    cells = b.cells()
    line = lambda what, k, e: print("%-8s %-22s kernel %.4f ms median %.4f min (%.0f GCUPS at min, sentinel cells counted) | launch->results %.3f median %.3f min"
                                    % (name, what, k[0], k[1], cells / k[1] / 1e6, e[0], e[1]), flush=True)
    ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_INT32)
    dev = ctx.sw_batch(b); line("score-only int32", kernel_ms(dev, reps), e2e_ms(dev, dev.scores)); want = dev.scores(); dev.close()
    ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
    dev = ctx.sw_batch(b, align=agx.SW_ALIGN_ENDS); k_ends = kernel_ms(dev, reps); line("ENDS", k_ends, e2e_ms(dev, dev.hits)); ends = dev.hits(); dev.close()
    assert np.array_equal(ends["score"], want)
    rb = reversed_prefixes(b, ends)
    dev = ctx.sw_batch(rb, align=agx.SW_ALIGN_ENDS); k_rev = kernel_ms(dev, reps); dev.close()
    dev = ctx.sw_batch(b, align=agx.SW_ALIGN_SPANS); e = e2e_ms(dev, dev.hits); spans = dev.hits(); dev.close()
    line("SPANS (fwd + begin)", (k_ends[0] + k_rev[0], k_ends[1] + k_rev[1]), e)
    print("%-8s begin pass alone: kernel %.4f ms median %.4f min over %d pairs, %.3f of the forward cells; checksum %d" %
          (name, k_rev[0], k_rev[1], rb.n_pairs, rb.cells() / cells, int(spans["a_begin"].sum() + spans["b_begin"].sum())), flush=True)
leg("config2", synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25), 50)
leg("mixed", synth.sw_pairs(65536, 32, 512, seed=4), 10)
