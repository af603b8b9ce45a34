"""Shared by tests/test_phmm_range_cpu.py and tests/test_phmm_range_gpu.py: PairHMM batches at the edges of the quality range
(Phred 0 ... 93, '!' ... '~') and of the float range (the rescue threshold AGX_PHMM_F32_RESCUE and the accuracy guard).

A PROFILE is a tuple of inclusive Phred ranges (base, insertion, deletion, gap continuation); a quality is drawn per read
position.  CLEAN profiles keep Qi + Qd <= 1 in every row: the recurrence is sub-stochastic, every state stays below its
initial constant.  RUNAWAY profiles have rows with Qi + Qd > 1 (both gap qualities of Phred 0 ... 3; 3 + 3 is over 1, 3 + 4 is
not): 1 - (Qi + Qd) < 0, the state alternates in sign and grows, the reference itself gives negative sums and NaN -- garbage
in, but legal bytes, and a read train must not hand such a read's state to the next read.

The batches take their structure from tests/phmm_widths.py (plain DNA: the looked-up-prior double fill and the packed float
fill's fast cell; twin() moves a batch to the selecting fill and the plain packed cell); qualify() then redraws the quality
tracks of the reads it is given."""
import numpy as np

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import phmm_widths as pw

USUAL = ((6, 41), (39, 45), (39, 45), (10, 10))
CLEAN = {
    "del93": ((6, 41), (39, 45), (93, 93), (10, 10)),
    "del80-93 gcp1": ((6, 41), (39, 45), (80, 93), (1, 1)),  # the fast cell's smallest D = Qd (1 - Qg+): about 1e-10
    "ins93": ((6, 41), (93, 93), (39, 45), (10, 10)),
    "gcp1": ((6, 41), (39, 45), (39, 45), (1, 1)),
    "gcp1-3": ((6, 41), (39, 45), (39, 45), (1, 3)),
    "gcp93": ((6, 41), (39, 45), (39, 45), (93, 93)),
    "base0": ((0, 0), (39, 45), (39, 45), (10, 10)),  # Qr = 1: a match has prior 0, a mismatch 1
    "base0-2": ((0, 2), (39, 45), (39, 45), (10, 10)),
    "base93": ((93, 93), (39, 45), (39, 45), (10, 10)),
    "gaps3-4": ((6, 41), (3, 4), (4, 4), (10, 10)),  # Qi + Qd up to 0.899: the last pair of gap qualities below the boundary
    "all4-93": ((4, 93), (4, 93), (4, 93), (1, 93)),
}
RUNAWAY = {
    "gaps0": ((6, 41), (0, 0), (0, 0), (10, 10)),
    "gaps1": ((6, 41), (1, 1), (1, 1), (10, 10)),
    "all1-93": ((1, 93), (1, 93), (1, 93), (1, 93)),
}
PROFILES = dict(CLEAN, usual=USUAL, **RUNAWAY)
LUT = 10.0 ** (-np.arange(94) / 10.0)
WIDTHS, LANES = (4, 19, 32), (3, 16)  # the narrowest class, config 3's, config 5's; the general build and the 16-lane one
RING_SHAPE = (364, 48)                # the first ring length of the looked-up-prior double fill
STRIPE_HAPS = (2100, 2600)            # beyond the single-pass span of the double and packed fills (2048), of the float fill (2560)
TRAIN_READS = (100, 250, 290)         # against haplotypes of R + 200: the shapes at which read trains pay
FLOAT_C = float(np.finfo(np.float32).max) / 16
RESCUE = 1e-28                        # AGX_PHMM_F32_RESCUE
RESCUE_LOG10 = float(np.log10(RESCUE / FLOAT_C))  # -65.33: log10 L of a pair whose scaled float sum is the threshold
LADDER_PROFILES = ("usual", "del93", "del80-93 gcp1", "gcp93")
GUARD_K = {0: 0.18, agx.PHMM_GATK_PRIOR: 0.40}  # kGuardRef, kGuardGatk of agx_phmm.cpp


def is_clean(profile):
    (_, _), (i0, _), (d0, _), (_, _) = profile
    return LUT[i0] + LUT[d0] <= 1


def runaway_rows(b):
    """Rows of the batch's reads with Qi + Qd > 1."""
    return LUT[b.q_ins.astype(int) - 33] + LUT[b.q_del.astype(int) - 33] > 1


def qualify(b, profile, rng, reads=None):
    """Redraws the four quality tracks of the batch's reads (all, or those listed) from the profile, in place -> b."""
    for r in range(b.roff.size - 1) if reads is None else reads:
        a, z = int(b.roff[r]), int(b.roff[r + 1])
        for track, (lo, hi) in zip((b.q_base, b.q_ins, b.q_del, b.q_gcp), profile):
            track[a:z] = rng.integers(lo, hi + 1, size=z - a) + 33
    return b


def _seed(name):
    return sum((k + 1) * c for k, c in enumerate(name.encode()))  # (hash() of a string changes from process to process)


def shape_batch(name, C, G):
    """Every shape of pw.shapes(C, G) as a region of 3 reads x 3 haplotypes, qualities from the profile."""
    rng = np.random.default_rng([_seed(name), C, G])
    b = synth.phmm_from_regions([pw.region(rng, [R] * 3, 3, H) for R, H in pw.shapes(C, G)])
    return qualify(b, PROFILES[name], rng)


def ring_batch(name):
    """One read of the first ring length against three short haplotypes (double modes)."""
    rng = np.random.default_rng([_seed(name), 364])
    R, H = RING_SHAPE
    return qualify(synth.phmm_from_regions([pw.region(rng, [R], 3, H)]), PROFILES[name], rng)


def stripe_batch(name):
    """One read against a haplotype beyond each single-pass span: the striped launch."""
    rng = np.random.default_rng([_seed(name), 12])
    haps = [pw.ACGT[rng.integers(0, 4, size=H)].tobytes() for H in STRIPE_HAPS]
    rd = np.frombuffer(haps[0], np.uint8)[1000:1012].tobytes()
    return qualify(synth.phmm_from_regions([([(rd,) * 5], haps)]), PROFILES[name], rng)


def clean_batches(name):
    """-> [(where, batch, families)] of one clean profile."""
    out = [("C%d G%d" % (C, G), shape_batch(name, C, G), tuple(pw.FAMILIES)) for C in WIDTHS for G in LANES]
    return out + [("ring", ring_batch(name), ("f64", "f64fma")), ("stripes", stripe_batch(name), tuple(pw.FAMILIES))]


N_TRAIN_REGIONS, N_TRAIN_READS, N_TRAIN_HAPS = 6, 7, 16


def train_batch(name, R):
    """Regions of 7 reads x 16 haplotypes of (R, R + 200) whose FIRST read has the (runaway) profile and whose other reads
    the usual one: with AGX_PHMM_TRAINS_ON the first read shares its lane groups with the second -> (batch, mask of the clean
    reads' pairs)."""
    b = synth.phmm_regions(N_TRAIN_REGIONS, N_TRAIN_READS, N_TRAIN_HAPS, R, R + 200, seed=_seed(name) + R)
    first = [int(b.rreg[g]) for g in range(b.n_regions)]
    qualify(b, PROFILES[name], np.random.default_rng([_seed(name), R]), first)
    clean = np.tile(np.repeat(np.arange(N_TRAIN_READS) > 0, N_TRAIN_HAPS), N_TRAIN_REGIONS)
    return b, clean


def auto_train_batch(name=None, rows=None):
    """Config 3's shape and size (64 regions x 64 reads x 16 haplotypes of 100 x 300), which forms read trains by itself; with a
    profile, the first read of every region has it; rows = (q_ins, q_del): ONE row of the first read has these qualities."""
    b = synth.phmm_regions(64, 64, 16, 100, 300, seed=3)
    if name:
        qualify(b, PROFILES[name], np.random.default_rng(_seed(name)), [int(b.rreg[g]) for g in range(b.n_regions)])
    if rows:
        b.q_ins[17], b.q_del[17] = rows[0] + 33, rows[1] + 33
    return b


LADDER_K = tuple(range(10, 22))


def rescue_ladder(name):
    """Config 3's shape, one haplotype: reads = one window of it with k mismatches of base quality 40 (four decades each) and one
    more whose base quality steps through 1 ... 40 (a tenth of a decade each); the mismatches of k are those of k - 1 and one
    more, every other quality is drawn once from the profile and shared by all reads -- so log10 L falls from about -40 to -88
    in steps of a tenth of a decade, across RESCUE_LOG10.  All reads sit in one region: with trains on they pair."""
    rng = np.random.default_rng([_seed(name), 100, 300])
    hap = pw.ACGT[rng.integers(0, 4, size=300)]
    window = hap[100:200]
    at = rng.permutation(100)[:LADDER_K[-1] + 1]
    wrong = pw.ACGT[(np.searchsorted(pw.ACGT, window[at]) + 1 + rng.integers(0, 3, size=at.size)) % 4]
    drawn = [(rng.integers(lo, hi + 1, size=100) + 33).astype(np.uint8) for lo, hi in PROFILES[name]]
    reads = []
    for k in LADDER_K:
        for q in range(1, 41):
            rd, qb = window.copy(), drawn[0].copy()
            rd[at[:k + 1]] = wrong[:k + 1]
            qb[at[:k]] = 40 + 33
            qb[at[k]] = q + 33
            reads.append((rd.tobytes(), qb.tobytes()) + tuple(t.tobytes() for t in drawn[1:]))
    return synth.phmm_from_regions([(reads, [hap.tobytes()])])


# Under a gap-continuation quality of Phred 1 the mismatch ladder cannot reach the threshold: inserting the whole read costs
# Qi Qg^(R - 1) = 1e-4 x 0.794^99, about 1e-14, whatever the read holds.  That floor is itself a ladder -- a tenth of a decade
# per read base -- and crosses RESCUE_LOG10 near R = 590.
INSERTION_READS = tuple(range(548, 629))


def insertion_ladder(name="del80-93 gcp1"):
    """Two regions of reads of 548 ... 628 bases of C and G against one haplotype of 100 A and T; a region's reads are the
    prefixes of one read (bases and qualities): log10 L is the all-insertion floor, from about -60 to -70 in steps of an eighth
    of a decade, the two regions offset by what their qualities differ."""
    rng = np.random.default_rng([_seed(name), 612])
    regions = []
    for _ in range(2):
        hap = pw.ACGT[[0, 3]][rng.integers(0, 2, size=100)].tobytes()
        whole = (pw.ACGT[[1, 2]][rng.integers(0, 2, size=INSERTION_READS[-1])],) + tuple(
            (rng.integers(lo, hi + 1, size=INSERTION_READS[-1]) + 33).astype(np.uint8) for lo, hi in PROFILES[name])
        regions.append(([tuple(t[:R].tobytes() for t in whole) for R in INSERTION_READS], [hap]))
    return synth.phmm_from_regions(regions)


def ladders(name):
    """-> [(what, batch)]: the ladders of one profile across the rescue threshold."""
    return [("mismatches", rescue_ladder(name))] + ([("insertions", insertion_ladder(name))] if name == "del80-93 gcp1" else [])


def rescued_range(l_ref):
    """-> (fewest, most) pairs that may go to the double pass: those whose scaled fp64 sum is below 0.99e-28, below 1.01e-28
    (sums that are 0 in fp64 included)."""
    scaled = l_ref + np.log10(FLOAT_C)
    return int(np.sum(scaled < np.log10(0.99 * RESCUE))), int(np.sum(scaled < np.log10(1.01 * RESCUE)))


GUARD_READS, GUARD_HAPS = (1, 2, 4, 8, 16, 30), tuple(range(1, 13))


def guard_ladder():
    """Reads of 1 ... 30 bases against haplotypes of 1 ... 12, perfect and with one mismatch, usual qualities: |log10 L| on both
    sides of the accuracy guard's bound GUARD_K sqrt(R + 8) -> (batch, R per pair)."""
    rng = np.random.default_rng(1830)
    regions = []
    for R in GUARD_READS:
        for H in GUARD_HAPS:
            hap = pw.ACGT[rng.integers(0, 4, size=H)]
            src = np.tile(hap, R // H + 2)
            reads = []
            for mism in (0, 0, 1, 1):
                st = int(rng.integers(0, H))
                rd = src[st:st + R].copy()
                if mism:
                    at = int(rng.integers(R))
                    rd[at] = pw.ACGT[(np.searchsorted(pw.ACGT, rd[at]) + 1 + int(rng.integers(3))) % 4]
                reads.append((rd.tobytes(),) + tuple((rng.integers(lo, hi + 1, size=R) + 33).astype(np.uint8).tobytes() for lo, hi in USUAL))
            regions.append((reads, [hap.tobytes()]))
    b = synth.phmm_from_regions(regions)
    return b, b.pair_lengths()[0]


def rel_err(l, l_ref):
    """Worst relative error of log10 L over the pairs finite on both sides that are outside 1e-6 / ln 10 of the reference in
    absolute terms or not (all of them: the figure the summary quotes), and the worst absolute one."""
    fin = np.isfinite(l) & np.isfinite(l_ref) & (l_ref != 0)
    d = np.abs(l[fin] - l_ref[fin])
    return float(np.max(d / np.abs(l_ref[fin]), initial=0.0)), float(np.max(d, initial=0.0))


def legs(ctx, orc, where, b, fams, out):
    """Every leg of one clean batch and of its twin with one N in a haplotype: F64, F64_FMA, F32, F32_FMA with trains off and on,
    F64 and F32_FMA with the GATK prior; appends {"where", "leg", "prec", pw.figures, "rel_log", info} records to out."""
    t, _ = pw.twin(b)
    refs = {0: orc.phmm_batch(b, 0), 3: orc.phmm_batch(b, 3)}
    trefs = {0: orc.phmm_batch(t, 0), 3: orc.phmm_batch(t, 3)}

    def one(leg, bb, rr, prec, trains=None):
        l, s, i = pw.run(ctx, bb, prec, trains)
        s_ref, l_ref = rr[3 if prec & agx.PHMM_GATK_PRIOR else 0]
        out.append(dict(where=where, leg=leg, prec=prec, rel_log=rel_err(l, l_ref)[0], **pw.figures(prec, l, s, l_ref, s_ref), **i))
        return l, s, i

    for fam in fams:
        prec = pw.FAMILIES[fam][0]
        for flag in (0, agx.PHMM_GATK_PRIOR) if fam in ("f64", "pk") else (0,):
            tag = fam + ("+gatk" if flag else "")
            if fam != "pk":
                one(tag, b, refs, prec | flag)
                one(tag + " twin", t, trefs, prec | flag)
                continue
            for bb, rr, tw in ((b, refs, ""), (t, trefs, " twin")):
                l0, s0, i0 = one(tag + tw + " trains off", bb, rr, prec | flag, agx.PHMM_TRAINS_OFF)
                l1, s1, _ = one(tag + tw + " trains on", bb, rr, prec | flag, agx.PHMM_TRAINS_ON)
                out[-1]["same_bits_as_off"] = bool(np.array_equal(s0, s1) and np.array_equal(l0, l1))
                out[-1]["waves_off"] = i0["n_waves"]
