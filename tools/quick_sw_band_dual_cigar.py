"""Timings of CIGARs for batches banded around a diagonal under two-piece gap costs
(agx_sw_batch_create_align_band_diag_dual_cigar).  The yardstick is the plain band-diag cigar batch
(agx_sw_batch_create_align_band_diag_cigar) under piece 1 on the same pairs, band and diag, in the same run: on the two uniform
batches of 4.1m / 4.1n -- 4 096 x 10 000 x 10 000 at w = 128 and 65 536 x 150 x 150 at w = 16, GLOBAL around 0 --
  traced two-piece fill (sw_fill_band_trace_dual) against traced plain fill (sw_fill_band_trace_at),
  walk (sw_walk_band_dual) against walk (sw_walk_band_at),
  launch -> CIGARs against launch -> hits of the two-piece SPANS batch, on the host clock,
  chunks and peak block of both,
  and the two-piece batch of the long pairs once more under twice the default chunk budget (the plain batch's number of chunks).
Kernel times are the tuning build's AGX_TRACE_CIGAR lines (set here: HIP events on the stream, summed over the chunks of a
round); a warm-up, then median and minimum of 7 rounds.  Run on the GPU box."""
import os, re, statistics, subprocess, sys, tempfile, time
if os.environ.get("AGX_TRACE_CIGAR") is None:  # the knob selects the tuning library when the package is imported: a fresh child
    sys.exit(subprocess.run([sys.executable] + sys.argv, env=dict(os.environ, AGX_TRACE_CIGAR="1")).returncode)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
ctx = agx.Context(0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
S_MM2 = (2, -4, -4, -2, -24, -1)
LINE = re.compile(rb"chunk \d+: .*traced fill ([0-9.]+) ms, walk ([0-9.]+) ms, gather ([0-9.]+) ms")
def uniform(n, la, lb, seed, sub=0.03):
    """n pairs of la x lb: b is a (cut to fit) with `sub` substitutions"""
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
    return synth.SWBatch(np.ascontiguousarray(bases), off, lens)
def cigar_rounds(dev, rounds=7):
    """-> per part (traced fill, walk, gather) median and minimum in ms, a round summed over its chunks; the host-clock ms of
    launch -> agx_sw_batch_cigars (median, minimum)"""
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
    low = [min(p[k] for p in parts) for k in range(3)]
    return med, low, (statistics.median(whole), min(whole))
def hits_ms(b, w, rounds=7):
    """launch -> hits of the two-piece SPANS batch on the host clock -> (median, minimum) of 7 after a warm-up"""
    dev = ctx.sw_batch(b, mode=agx.SW_MODE_GLOBAL, align=agx.SW_ALIGN_SPANS, band=w, diag=0, dual=S_MM2)
    t = []
    for r in range(rounds + 1):
        ctx.sync()
        t0 = time.perf_counter(); dev.launch(); dev.hits(); t.append((time.perf_counter() - t0) * 1e3)
    dev.close()
    return statistics.median(t[1:]), min(t[1:])
def leg(name, b, w):
    plain = ctx.sw_batch(b, mode=agx.SW_MODE_GLOBAL, band=w, diag=0, cigar=True, scoring=S_MM2[:4])
    (f0, w0, _), (lf0, lw0, _), (c0, lc0) = cigar_rounds(plain)
    i0 = plain.cigar_info(); plain.close()
    dual = ctx.sw_batch(b, mode=agx.SW_MODE_GLOBAL, band=w, diag=0, dual_cigar=S_MM2)
    (f1, w1, g1), (lf1, lw1, _), (c1, lc1) = cigar_rounds(dual)
    i1 = dual.cigar_info(); dual.close()
    h, lh = hits_ms(b, w)
    print("%-22s global w=%-4d traced fill: plain %.3f ms (min %.3f), two-piece %.3f ms (min %.3f) = %.2f x | walk: plain %.3f ms (min %.3f), "
          "two-piece %.3f ms (min %.3f) = %.2f x | gather %.3f ms | launch -> CIGARs: plain %.1f ms (min %.1f), two-piece %.1f ms (min %.1f); launch -> hits "
          "of the two-piece SPANS batch %.1f ms (min %.1f) = %.2f x | chunks %d -> %d, peak block %.1f MB -> %.1f MB, %.3e in-band cells"
          % (name, w, f0, lf0, f1, lf1, f1 / f0, w0, lw0, w1, lw1, w1 / w0, g1, c0, lc0, c1, lc1, h, lh, c1 / h, i0.n_chunks, i1.n_chunks,
             i0.trace_bytes_peak / 1e6, i1.trace_bytes_peak / 1e6, i1.trace_cells), flush=True)
def dual_at_budget(name, b, w, budget):
    """the two-piece batch again under a chunk budget of its own, so that it makes the plain batch's number of chunks"""
    ctx.set_option(agx.OPT_SW_TRACE_BYTES, budget)
    dual = ctx.sw_batch(b, mode=agx.SW_MODE_GLOBAL, band=w, diag=0, dual_cigar=S_MM2)
    (f1, w1, _), (lf1, lw1, _), (c1, lc1) = cigar_rounds(dual)
    i1 = dual.cigar_info(); dual.close()
    print("%-22s global w=%-4d two-piece under AGX_OPT_SW_TRACE_BYTES = %d: traced fill %.3f ms (min %.3f) | walk %.3f ms (min %.3f) | launch -> CIGARs "
          "%.1f ms (min %.1f) | chunks %d, peak block %.1f MB" % (name, w, budget, f1, lf1, w1, lw1, c1, lc1, i1.n_chunks, i1.trace_bytes_peak / 1e6), flush=True)
reads = uniform(65536, 150, 150, 2)
leg("65536 x 150 x 150", reads, 16)
del reads
long_pairs = uniform(4096, 10000, 10000, 1)
leg("4096 x 10000 x 10000", long_pairs, 128)
dual_at_budget("4096 x 10000 x 10000", long_pairs, 128, 2 << 30)
