"""CIGAR timings (agx_sw_batch_create_align_cigar) on config 2's batch and on a mixed batch, per mode next to the plain SPANS
batch of the same mode (the parent's entry points, unchanged) on the same batch in the same run: launch -> cigars against
launch -> hits on the host clock, minimum and median of 7 rounds, and -- the tuning build's AGX_TRACE_CIGAR line, set here --
the kernel-only times of the traced fill, the walk and the gather of every chunk (HIP events on the stream; the last round's
are printed).  Run on the GPU box."""
import os, statistics, subprocess, sys, time
if os.environ.get("AGX_TRACE_CIGAR") is None:  # the knob selects the tuning library when the package is imported: a fresh child
    sys.exit(subprocess.run([sys.executable] + sys.argv, env=dict(os.environ, AGX_TRACE_CIGAR="1")).returncode)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
NAMES = {agx.SW_MODE_LOCAL: "local", agx.SW_MODE_GLOBAL: "global", agx.SW_MODE_FIT: "fit", agx.SW_MODE_EXTEND: "extend", agx.SW_MODE_EXTEND_QUERY: "extend-query"}
def e2e_ms(dev, fetch, rounds=7, quiet=True):
    err = os.dup(2)
    if quiet:  # the trace line of every round but the one after would drown the table
        null = os.open(os.devnull, os.O_WRONLY); os.dup2(null, 2); os.close(null)
    try:
        for _ in range(2): dev.launch(); fetch()
        t = []
        for _ in range(rounds):
            t0 = time.perf_counter(); dev.launch(); fetch(); t.append((time.perf_counter() - t0) * 1e3)
    finally:
        os.dup2(err, 2); os.close(err)
    return statistics.median(t), min(t)
def leg(name, b):
    for mode in NAMES:
        sp = ctx.sw_batch(b, align=agx.SW_ALIGN_SPANS, mode=mode); es = e2e_ms(sp, sp.hits); want = sp.hits(); sp.close()
        cg = ctx.sw_batch(b, mode=mode, cigar=True); ec = e2e_ms(cg, cg.cigars)
        sys.stderr.flush(); cg.launch(); hits, op_off, ops = cg.cigars(); info = cg.cigar_info(); cg.close()  # (this round's trace line is shown)
        assert all(np.array_equal(hits[f], want[f]) for f in want.dtype.names)
        print("%-8s %-13s launch->hits (SPANS) %.3f ms min (%.3f median) | launch->cigars %.3f ms min (%.3f median) = %.2f x | %d traced pairs, %.3e cells, "
              "%d chunks, %.1f MB peak, %d operations" % (name, NAMES[mode], es[1], es[0], ec[1], ec[0], ec[1] / es[1], info.n_traced, info.trace_cells,
                                                           info.n_chunks, info.trace_bytes_peak / 1e6, ops.size), flush=True)
leg("config2", synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25))
leg("mixed", synth.sw_pairs(65536, 32, 512, seed=4))
