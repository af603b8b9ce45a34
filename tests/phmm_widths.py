"""Shared by tests/test_phmm_widths_cpu.py and tests/test_phmm_widths_gpu.py: the plain-DNA batches that place a PairHMM
pair on a chosen number of lanes per group, and the child process that runs them with the kernel width pinned.

The PairHMM fills are template families, one build per number of columns per lane C, each as a build for 16-lane groups and a
general one.  AGX_PHMM_FORCE_C pins C; it exists in the tuning build only and is read once per process, so every width runs in
a child of its own (run_child).  A class table that lacks the width ignores the knob, hence FAMILIES: which precisions obey it.

For a width C, a pair lands on G = ceil(H / C) lanes; shapes(C, G) lists the (R, H) at which a fill can go wrong: the last lane
full or holding one real column, fewer rows than the skew of G - 1 steps, one row, two.  A launch runs the 16-lane build only
when ALL its groups have 16 lanes, so every G has a batch (and so a launch) of its own.

Everything here is plain DNA -- reads over ACGTN, haplotypes over ACGT -- so the double modes run the fill with looked-up
priors and the packed float mode its fast cell; twin() changes one haplotype byte to N, which moves the whole batch to the
selecting fill and the plain packed cell."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
GS = (1, 2, 3, 16, 17, 64)
RING_GS = (3, 16)
RING_READS = (364, 600, 1000)  # 364: the first ring length (366 rows > AGX_PH_LUT_FULL_ROWS); the others reuse every ring row
WHOLE_READ = 363               # R + 2 = 365 rows: the longest whole table
GATK_GS = (3, 16)
# family -> (precision, widths its class table has, pairs per lane group)
FAMILIES = {"f64": (agx.PHMM_F64, tuple(range(4, 33, 2)), 1), "f64fma": (agx.PHMM_F64_FMA, tuple(range(4, 33, 2)), 1),
            "f32": (agx.PHMM_F32, tuple(range(4, 41, 2)), 1), "pk": (agx.PHMM_F32_FMA, tuple(range(4, 33)), 2)}
WIDTHS = tuple(range(4, 33)) + (34, 36, 38, 40)
CHILD_TIMEOUT = 300  # seconds, as the other child processes of the suite


def families(C):
    return [f for f, (_, widths, _) in FAMILIES.items() if C in widths]


def shapes(C, G):
    """(R, H) of the pairs that sit on G lanes of C columns."""
    hs = sorted({G * C, (G - 1) * C + 1})
    rs = sorted({r for r in (1, 2, G - 1, G, 2 * G + 3) if r >= 1})
    return [(R, H) for H in hs for R in rs]


def steps(R, G, R2=None):
    """Steps of a wave whose longest group has R rows on G lanes; with a second read of R2 rows behind the first (a train)."""
    return R + G - 1 if R2 is None else R + 1 + R2 + 1 + G - 2


def _q(rng, n, lo, hi):
    return (rng.integers(lo, hi, size=n) + 33).astype(np.uint8).tobytes()


def region(rng, read_lens, n_haps, H, alphabet=ACGT, gaps=(39, 46), gcp=10):
    """One region: a random haplotype and variants of it (up to three SNPs), reads = windows of one of them (of its repetition
    where the read is longer) with 1 % substitutions and 2 % N."""
    base = alphabet[rng.integers(0, alphabet.size, size=H)]
    haps = []
    for k in range(n_haps):
        h = base.copy()
        for _ in range(int(rng.integers(1, 4)) if k else 0):
            h[int(rng.integers(H))] = alphabet[int(rng.integers(alphabet.size))]
        haps.append(h.tobytes())
    reads = []
    for R in read_lens:
        src = np.tile(np.frombuffer(haps[int(rng.integers(n_haps))], np.uint8), R // H + 2)
        st = int(rng.integers(0, src.size - R + 1))
        r = src[st:st + R].copy()
        m = rng.random(R) < 0.01
        r[m] = ACGT[rng.integers(0, 4, size=int(m.sum()))]
        r[rng.random(R) < 0.02] = ord("N")
        reads.append((r.tobytes(), _q(rng, R, 6, 42), _q(rng, R, *gaps), _q(rng, R, *gaps), bytes([gcp + 33]) * R))
    return reads, haps


def width_batch(C, G):
    """Every shape of shapes(C, G) as a region of 3 reads x 3 haplotypes (an odd count: a vacant packed half, an unpaired read
    in a train) and one region of 2 x 2.  G = 16: one more read, unrelated to its haplotypes (all A against haplotypes of
    C, G, T, base and gap-continuation qualities of Phred 41: four orders of magnitude per base whether it mismatches or is
    inserted, about 1e-140), which underflows in float and goes through the rescue plan."""
    rng = np.random.default_rng(1000 * C + G)
    regions = []
    for R, H in shapes(C, G):
        far = G == 16 and (R, H) == (2 * G + 3, G * C)
        reads, haps = region(rng, [R] * 3, 3, H, alphabet=ACGT[1:] if far else ACGT)
        if far:
            reads.append((b"A" * R, b"J" * R, _q(rng, R, 39, 46), _q(rng, R, 39, 46), b"J" * R))
        regions.append((reads, haps))
    regions.append(region(rng, [2 * G + 3] * 2, 2, G * C))
    b = synth.phmm_from_regions(regions)
    b.read_bases[int(b.roff[2]) - 1] = ord("N")  # 2 % of a handful of bases may be none: the second read ends in N
    return b


# ring batches: gap qualities of Phred 1 .. 4 keep a read of 1000 bases against a haplotype of a dozen within the double range
# (about 0.8 per inserted base), so that what the ring rows hold reaches the sums
_RING_Q = dict(gaps=(1, 5), gcp=1)


def ring_batches(C, G):
    """-> {"whole": the longest whole table, "ring": the first ring length, two lengths that reuse every ring row, and a ring
    and a whole table in one region (one launch)}, haplotypes of G * C columns."""
    rng = np.random.default_rng(5000 * C + G)
    H = G * C
    whole = synth.phmm_from_regions([region(rng, [WHOLE_READ] * 3, 3, H, **_RING_Q)])
    ring = synth.phmm_from_regions([region(rng, [R] * 3, 3, H, **_RING_Q) for R in RING_READS] + [region(rng, [364, 40], 3, H, **_RING_Q)])
    return {"whole": whole, "ring": ring}


def uniform_batch(C, G, R, n_regions=1, n_reads=3, n_haps=3):
    """n_regions x n_reads x n_haps pairs of one shape, (R, G * C)."""
    rng = np.random.default_rng(C * 64 + G)
    reads, haps = region(rng, [R] * n_reads, n_haps, G * C)
    return synth.phmm_from_regions([(reads, haps)] * n_regions)


def twin(b):
    """The batch with the last byte of its last haplotype set to N -> (batch, mask of the pairs that do not use that haplotype)."""
    t = synth.PhmmBatch(*(getattr(b, f.name).copy() for f in dataclasses.fields(b)))
    t.hap_bases[-1] = ord("N")
    keep = []
    last = int(b.hreg[-1]) - 1
    for g in range(b.n_regions):
        nr = int(b.rreg[g + 1]) - int(b.rreg[g])
        keep += [h != last for _ in range(nr) for h in range(int(b.hreg[g]), int(b.hreg[g + 1]))]
    return t, np.array(keep, bool)


def figures(prec, l, s, l_ref, s_ref):
    """What a result is judged by (meets()): the finite / -inf pattern, and per precision bit equality, the relative error of
    log10 L, or the number of pairs outside 1e-6 relative on log10 L and 1e-6 / ln 10 absolute (tools/fuzz_gpu.py's rule)."""
    fin = np.isfinite(l_ref)
    out = {"pattern": bool(np.array_equal(np.isfinite(l), fin) and np.array_equal(l[~fin], l_ref[~fin])), "n": int(l.size)}
    base = prec & 0xff
    fin = fin & np.isfinite(l)  # (a wrong pattern already fails: the errors are those of the pairs finite on both sides)
    d = np.abs(l[fin] - l_ref[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = d / np.abs(l_ref[fin])
    if base == agx.PHMM_F64:
        out["equal"] = bool(np.array_equal(s, s_ref) and np.array_equal(l, l_ref))
    elif base == agx.PHMM_F64_FMA:
        out["rel"] = float(np.max(rel[np.isfinite(rel)], initial=0.0))
        out["zero_ref_off"] = int(np.sum((l_ref[fin] == 0) & (d > 0)))
    else:
        out["bad"] = int(np.sum((d > 1e-6 * np.abs(l_ref[fin])) & (d > 1e-6 / np.log(10))))
        out["worst"] = float(np.max(d, initial=0.0))
    return out


def meets(prec, fig):
    base = prec & 0xff
    if not fig["pattern"]:
        return False
    if base == agx.PHMM_F64:
        return fig["equal"]
    if base == agx.PHMM_F64_FMA:
        return fig["rel"] <= 1e-12 and fig["zero_ref_off"] == 0
    return fig["bad"] == 0


def _info(dev):
    i = dev.info()
    return {"n_waves": i.n_waves, "padded": i.padded_cells, "n_launches": i.n_launches, "cells": i.cells}


def plan(b, prec):
    dev = agx.PhmmBatchDev(None, b, prec)
    i = _info(dev)
    dev.close()
    return i


def run(ctx, b, prec, trains=None):
    """-> (log10 L, sums, info) of one launch; trains: AGX_OPT_PHMM_TRAINS for this batch (then back to the default)."""
    if trains is not None:
        ctx.set_option(agx.OPT_PHMM_TRAINS, trains)
    try:
        dev = ctx.phmm_batch(b, prec)
    finally:
        if trains is not None:
            ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_AUTO)
    i = _info(dev)
    dev.launch()
    l, s = dev.results()
    i["n_rescued"] = dev.info().n_rescued
    dev.close()
    return l, s, i


def legs(ctx, orc, b, fams, gatk, where, out):
    """Every leg of one plain-DNA batch and of its twin; appends {"where", "leg", "prec", figures, info} records to out."""
    refs = {0: orc.phmm_batch(b, 0)}
    t, keep = twin(b)
    trefs = {0: orc.phmm_batch(t, 0)}
    if gatk:
        refs[3], trefs[3] = orc.phmm_batch(b, 3), orc.phmm_batch(t, 3)

    def one(leg, bb, rr, prec, trains=None, same_plan=True):
        l, s, i = run(ctx, bb, prec, trains)
        s_ref, l_ref = rr[3 if prec & agx.PHMM_GATK_PRIOR else 0]
        rec = dict(where=where, leg=leg, prec=prec, **figures(prec, l, s, l_ref, s_ref), **i)
        if same_plan:  # the plan made without a device is the one that ran
            p = plan(bb, prec)
            rec["plan_same"] = all(p[k] == i[k] for k in p)
        out.append(rec)
        return l, s, i

    for fam in fams:
        prec = FAMILIES[fam][0]
        flags = (0, agx.PHMM_GATK_PRIOR) if gatk and fam in ("f64", "pk") else (0,)
        for flag in flags:
            tag = fam + ("+gatk" if flag else "")
            if fam == "pk":
                l0, s0, i0 = one(tag + " trains off", b, refs, prec | flag, agx.PHMM_TRAINS_OFF)
                l1, s1, i1 = one(tag + " trains on", b, refs, prec | flag, agx.PHMM_TRAINS_ON, same_plan=False)
                out[-1]["same_bits_as_off"] = bool(np.array_equal(s0, s1) and np.array_equal(l0, l1))
                out[-1]["waves_off"] = i0["n_waves"]
                _, _, j0 = one(tag + " twin trains off", t, trefs, prec | flag, agx.PHMM_TRAINS_OFF)
                one(tag + " twin trains on", t, trefs, prec | flag, agx.PHMM_TRAINS_ON, same_plan=False)
                out[-1]["waves_off"] = j0["n_waves"]
            else:
                _, s, _ = one(tag, b, refs, prec | flag)
                _, st, _ = one(tag + " twin", t, trefs, prec | flag)
                if fam == "f64":  # two different kernels, the same bits
                    out[-1]["same_bits_as_plain_dna"] = bool(np.array_equal(s[keep], st[keep]))


def gpu_width(C):
    from tests import oracle_api

    orc = oracle_api.load()
    fams, out = families(C), []
    with agx.Context(0) as ctx:
        for G in GS:
            legs(ctx, orc, width_batch(C, G), fams, G in GATK_GS, "G%d" % G, out)
        dbl = [f for f in fams if f in ("f64", "f64fma")]
        for G in RING_GS if dbl else ():
            for name, b in ring_batches(C, G).items():
                s_ref, l_ref = orc.phmm_batch(b, 0)
                for fam in dbl:
                    l, s, i = run(ctx, b, FAMILIES[fam][0])
                    out.append(dict(where="G%d %s" % (G, name), leg=fam, prec=FAMILIES[fam][0], all_finite=bool(np.isfinite(l_ref).all()),
                                    **figures(FAMILIES[fam][0], l, s, l_ref, s_ref), **i))
    return out


def plan_width(C):
    """Plans only (no device): every shape alone, every batch gpu_width runs, and what shows trains and the looked-up-prior
    tables in a plan."""
    out = {"shapes": [], "batches": [], "trains": None, "tables": []}
    for fam in families(C):
        prec = FAMILIES[fam][0]
        for G in GS:
            for R, H in shapes(C, G):
                rng = np.random.default_rng(R * 4099 + H)
                b = synth.phmm_from_regions([region(rng, [R] * 3, 3, H)])
                out["shapes"].append([fam, G, R, H, plan(b, prec)])
            b = width_batch(C, G)
            out["batches"].append([fam, "G%d" % G, plan(b, prec), plan(twin(b)[0], prec)])
        if fam in ("f64", "f64fma"):
            for G in RING_GS:
                for name, b in ring_batches(C, G).items():
                    out["batches"].append([fam, "G%d %s" % (G, name), plan(b, prec), None])
            # 40 reads of 30 bases, one haplotype of two lanes each: 32 groups fit a wave, but only as many as have their tables
            # in 20 KB of LDS -- rows of 56 bytes (looked-up priors) or of 33 (selecting fill)
            rng = np.random.default_rng(C)
            b = synth.phmm_from_regions([region(rng, [30], 1, 2 * C) for _ in range(40)])
            out["tables"].append([fam, plan(b, prec), plan(twin(b)[0], prec)])
    if "pk" in families(C):
        # config 3's count of pairs on 16 lanes: enough waves for trains to form by themselves (no device: AGX_PHMM_TRAINS_AUTO)
        b = uniform_batch(C, 16, 10, 64, 64, 16)
        out["trains"] = [plan(b, agx.PHMM_F32_FMA), plan(twin(b)[0], agx.PHMM_F32_FMA)]
    return out


CHILD = """
import json, sys
sys.path.insert(0, %r)
import accelerating_genomics_amd.api as agx
from tests import phmm_widths as pw
assert agx.LIB_PATH.endswith("libagx_tuning.so"), agx.LIB_PATH
mode, C = sys.argv[1], int(sys.argv[2])
print("RESULT " + json.dumps({"plan": pw.plan_width, "gpu": pw.gpu_width}[mode](C)))
""" % ROOT


class ChildDied(Exception):
    pass


def run_child(mode, C):
    """One fresh process with AGX_PHMM_FORCE_C = C -> what it printed as JSON.  ChildDied: it ended by a signal, at its time
    limit or without a result (the message carries its last output)."""
    env = dict(os.environ, AGX_PHMM_FORCE_C=str(C))
    env.pop("AGX_LIB_PATH", None)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, mode, str(C)], capture_output=True, timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired as e:
        raise ChildDied("width %d: no result within %d s\n%s" % (C, CHILD_TIMEOUT, ((e.stdout or b"") + (e.stderr or b"")).decode(errors="replace")[-2000:]))
    lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or len(lines) != 1:
        raise ChildDied("width %d: exit status %d\n%s" % (C, r.returncode, (r.stdout + r.stderr).decode(errors="replace")[-2000:]))
    return json.loads(lines[0][len("RESULT "):])


def one_shape_waves(fam, G, n_regions=1, n_reads=3, n_haps=3):
    """Waves of n_regions x n_reads x n_haps pairs of one shape on G lanes: 64 // G groups per wave, a group = one pair, or one
    read with two haplotypes (packed float fill: an odd haplotype count leaves a half vacant)."""
    groups = n_regions * n_reads * ((n_haps + 1) // 2 if FAMILIES[fam][2] == 2 else n_haps)
    return -(-groups // (64 // G))
