"""Timings of CIGARs for batches banded around a diagonal (agx_sw_batch_create_align_band_diag_cigar).
1. The traced build that starts inside the image (sw_fill_band_trace_at<K>) against the existing one (sw_fill_band_trace<K>, the
   yardstick) in the same run on the same GLOBAL spans from (0, 0): 65 536 x 150 x 150 at w = 16 and 4 096 x 10 000 x 10 000 at
   w = 128, la == lb, so that the banded cigar batch and the band-diag cigar batch at c = 0 trace the same band; also the two walks.
2. A read in its window: 4 096 reads of 2 000 in windows of 60 000 at w = 128, FIT (and LOCAL) around -29 000 (-29 001 .. -28 998
   from pair to pair, so that the spans begin at all four start phases): traced fill, walk, gather, and launch -> CIGARs on the
   host clock beside launch -> hits of the band-diag SPANS batch on the same input.
Kernel times are the tuning build's AGX_TRACE_CIGAR lines (set here: HIP events on the stream, summed over the chunks of a
round); a warm-up, then the median of 7 rounds.  Run on the GPU box."""
import os, re, statistics, subprocess, sys, tempfile, time
if os.environ.get("AGX_TRACE_CIGAR") is None:  # the knob selects the tuning library when the package is imported: a fresh child
    sys.exit(subprocess.run([sys.executable] + sys.argv, env=dict(os.environ, AGX_TRACE_CIGAR="1")).returncode)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
LINE = re.compile(rb"chunk \d+: .*traced fill ([0-9.]+) ms, walk ([0-9.]+) ms, gather ([0-9.]+) ms")
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
def cigar_rounds(dev, rounds=7):
    """-> per part (traced fill, walk, gather) the median and the spread (max - min) in ms, a round summed over its chunks;
    the host-clock ms of launch -> agx_sw_batch_cigars (median)."""
    parts, whole = [], []
    err = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            for r in range(rounds + 1):  # the first is the warm-up
                ctx.sync()
                f.seek(0); f.truncate()
                t0 = time.perf_counter(); dev.launch(); dev.cigars(); t1 = time.perf_counter()
                sys.stderr.flush(); f.seek(0)
                got = [tuple(float(v) for v in m.groups()) for m in LINE.finditer(f.read())]
                if r:
                    parts.append(tuple(sum(g[k] for g in got) for k in range(3)))
                    whole.append((t1 - t0) * 1e3)
        finally:
            os.dup2(err, 2); os.close(err)
    med = [statistics.median(p[k] for p in parts) for k in range(3)]
    spread = [max(p[k] for p in parts) - min(p[k] for p in parts) for k in range(3)]
    return med, spread, statistics.median(whole)
def hits_ms(b, mode, w, diag, rounds=7):
    """launch -> hits of the band-diag SPANS batch on the host clock, median of 7 after a warm-up"""
    dev = ctx.sw_batch(b, mode=mode, align=agx.SW_ALIGN_SPANS, band=w, diag=diag)
    t = []
    for r in range(rounds + 1):
        ctx.sync()
        t0 = time.perf_counter(); dev.launch(); dev.hits(); t.append((time.perf_counter() - t0) * 1e3)
    dev.close()
    return statistics.median(t[1:])
def builds(name, b, w):
    old = ctx.sw_batch(b, mode=agx.SW_MODE_GLOBAL, band=w, cigar=True)
    (f0, w0, _), (sf0, sw0, _), _ = cigar_rounds(old)
    want = old.cigars(); old.close()
    new = ctx.sw_batch(b, mode=agx.SW_MODE_GLOBAL, band=w, diag=0, cigar=True)
    (f1, w1, _), (sf1, sw1, _), _ = cigar_rounds(new)
    got = new.cigars(); info = new.cigar_info(); new.close()
    assert all(np.array_equal(x, y) for x, y in zip(got, want))  # the same hits and operations
    print("%-22s global w=%-4d traced fill: sw_fill_band_trace %.3f ms (spread %.3f), sw_fill_band_trace_at %.3f ms (spread %.3f) = %+.2f %% | "
          "walk: sw_walk_band %.3f ms (spread %.3f), sw_walk_band_at %.3f ms (spread %.3f) = %+.2f %% | %d chunks, %.3e in-band cells"
          % (name, w, f0, sf0, f1, sf1, 100 * (f1 - f0) / f0, w0, sw0, w1, sw1, 100 * (w1 - w0) / w0, info.n_chunks, info.trace_cells), flush=True)
reads = uniform(65536, 150, 150, 2)
builds("65536 x 150 x 150", reads, 16)
del reads
long_pairs = uniform(4096, 10000, 10000, 1)
builds("4096 x 10000 x 10000", long_pairs, 128)
del long_pairs
win = uniform(4096, 2000, 60000, 3, at=29000)
centre = (-29000 + (np.arange(win.n_pairs) & 3) - 1).astype(np.int32)
row0 = -(centre.astype(np.int64) + 128)  # the first row the band touches
for mode, word in ((agx.SW_MODE_FIT, "fit"), (agx.SW_MODE_LOCAL, "local")):
    spans = hits_ms(win, mode, 128, centre)
    dev = ctx.sw_batch(win, mode=mode, band=128, diag=centre, cigar=True)
    (fill, walk, gather), (sf, sw, _), whole = cigar_rounds(dev)
    hits, op_off, ops = dev.cigars(); info = dev.cigar_info(); dev.close()
    print("%-22s %-6s w=128  traced fill %.3f ms (spread %.3f) | walk %.3f ms (spread %.3f) | gather %.3f ms | launch -> CIGARs %.1f ms, launch -> hits of "
          "the SPANS batch %.1f ms (%.2f x) | %d traced pairs, %.3e in-band cells, %d chunks, %.1f MB peak, %d operations, start phases %s"
          % ("4096 x 2000 in 60000", word, fill, sf, walk, sw, gather, whole, spans, whole / spans, info.n_traced, info.trace_cells, info.n_chunks,
             info.trace_bytes_peak / 1e6, ops.size, np.bincount((hits["b_begin"] - row0) & 3, minlength=4).tolist()), flush=True)
