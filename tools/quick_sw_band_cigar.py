"""Banded-CIGAR timings (agx_sw_batch_create_align_band_cigar) on long pairs (4 096 x 10 000 x 10 000 at w = 128,
GLOBAL) and on reads (65 536 x 150 x 150 at w = 16, both modes).  Per batch, in one run: the UNTRACED banded fill of the plain
banded batch (the yardstick; HIP events round back-to-back launches), then of agx_sw_batch_cigars the traced fill, the walk and
the gather (the tuning build's AGX_TRACE_CIGAR lines, set here: HIP events on the stream, summed over the chunks of a round), the
whole call on the host clock, chunks and trace bytes; the long batch a second time with a budget that holds it in one chunk.
A warm-up, then the median of 7 rounds.  Run on the GPU box."""
import os, re, statistics, subprocess, sys, tempfile, time
if os.environ.get("AGX_TRACE_CIGAR") is None:  # the knob selects the tuning library when the package is imported: a fresh child
    sys.exit(subprocess.run([sys.executable] + sys.argv, env=dict(os.environ, AGX_TRACE_CIGAR="1")).returncode)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
LINE = re.compile(rb"chunk \d+: .*traced fill ([0-9.]+) ms, walk ([0-9.]+) ms, gather ([0-9.]+) ms")
def kernel_ms(dev, reps, rounds=7):
    for _ in range(2): dev.launch()
    ctx.sync()
    t = []
    for _ in range(rounds):
        ctx.timer_start()
        for _ in range(reps): dev.launch()
        t.append(ctx.timer_stop() / reps)
    return statistics.median(t)
def uniform(n, la, lb, seed, sub=0.03):
    """n pairs of la x lb: b is a (cut or extended to lb) with `sub` substitutions (tools/quick_sw_band.py's batches)."""
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
def cigar_rounds(dev, rounds=7):
    """-> per round (traced fill, walk, gather) in ms summed over its chunks, and the host-clock ms of agx_sw_batch_cigars."""
    parts, whole = [], []
    err = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            for r in range(rounds + 1):  # the first is the warm-up
                dev.launch(); ctx.sync()
                f.seek(0); f.truncate()
                t0 = time.perf_counter(); dev.cigars(); t1 = time.perf_counter()
                sys.stderr.flush(); f.seek(0)
                got = [tuple(float(v) for v in m.groups()) for m in LINE.finditer(f.read())]
                if r:
                    parts.append(tuple(sum(g[k] for g in got) for k in range(3)))
                    whole.append((t1 - t0) * 1e3)
        finally:
            os.dup2(err, 2); os.close(err)
    return [statistics.median(p[k] for p in parts) for k in range(3)], statistics.median(whole)
def leg(name, b, mode, w, reps, budget=None):
    ctx.set_option(agx.OPT_SW_TRACE_BYTES, budget or 1 << 30)  # (1 GiB is the default)
    word = "global" if mode == agx.SW_MODE_GLOBAL else "extend"
    plain = ctx.sw_batch(b, mode=mode, band=w); fill = kernel_ms(plain, reps); want = plain.hits(); plain.close()
    dev = ctx.sw_batch(b, mode=mode, band=w, cigar=True)
    (traced, walk, gather), whole = cigar_rounds(dev)
    hits, op_off, ops = dev.cigars(); info = dev.cigar_info(); dev.close()
    assert all(np.array_equal(hits[f], want[f]) for f in want.dtype.names)
    print("%-22s %-6s w=%-4d untraced fill %.3f ms | traced fill %.3f ms = %.2f x | walk %.3f ms (%.0f %% of fill + walk + gather) | gather %.3f ms | "
          "agx_sw_batch_cigars %.1f ms | %d traced pairs, %.3e in-band cells, %d chunks, %.1f MB peak, %d operations"
          % (name, word, w, fill, traced, traced / fill, walk, 100 * walk / (traced + walk + gather), gather, whole, info.n_traced, info.trace_cells,
             info.n_chunks, info.trace_bytes_peak / 1e6, ops.size), flush=True)
long_pairs = uniform(4096, 10000, 10000, 1)
leg("4096 x 10000 x 10000", long_pairs, agx.SW_MODE_GLOBAL, 128, 1)
leg("the same, 8 GiB a chunk", long_pairs, agx.SW_MODE_GLOBAL, 128, 1, 8 << 30)
del long_pairs
reads = uniform(65536, 150, 150, 2)
leg("65536 x 150 x 150", reads, agx.SW_MODE_GLOBAL, 16, 10)
leg("65536 x 150 x 150", reads, agx.SW_MODE_EXTEND, 16, 10)
