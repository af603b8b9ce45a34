"""GPU parity of the PairHMM forward fill (through the C-ABI) against the oracle and the
reference's outputs.  Bars: AGX_PHMM_F64 raw sums bit-identical (stronger than BASELINE's
1e-12); AGX_PHMM_F64_FMA <= 1e-12 relative on log10; AGX_PHMM_F32 <= 1e-6 relative on log10
(BASELINE config 3), with underflowed pairs rescued in double."""
import ctypes as C
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import oracle_api

pytestmark = pytest.mark.gpu

NAMES = ["phmm_test", "phmm_10s", "phmm_synth", "phmm_far", "phmm_long"]


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


def g17(golden_dir, name):
    return np.array([float(x) for x in open(os.path.join(golden_dir, name + ".g17.out")).read().split()])


def relerr(a, b):
    return np.max(np.abs((a - b) / b)) if a.size else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_f64_bit_identical_to_reference_output(ctx, golden_dir, name):
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, name + ".in"))
    got = ctx.phmm_forward(b, agx.PHMM_F64)
    ref = g17(golden_dir, name)
    assert got.size == ref.size
    assert np.array_equal(got, ref)  # %.17g round-trips: every double equal


def test_quality_bytes_above_0x7f_read_as_signed_char(ctx, golden_dir):
    """the reference holds quality bytes in plain `char` (signed on x86-64, antidiagsPairHMM.c:99-107), so a
    byte of 200 is Phred -89.  phmm_hibit.in has such bytes; its %.17g output comes from the compiled pairHMMmatrix.c.
    Finite values bit for bit, the others (negative sums) NaN where the reference's are."""
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, "phmm_hibit.in"))
    ref = g17(golden_dir, "phmm_hibit")
    fin = np.isfinite(ref)
    assert 6 <= fin.sum() < ref.size
    got = ctx.phmm_forward(b, agx.PHMM_F64)
    assert np.array_equal(got[fin], ref[fin]) and np.array_equal(np.isnan(got), np.isnan(ref))
    for prec in (agx.PHMM_F64_FMA, agx.PHMM_F32, agx.PHMM_F32_FMA):  # garbage never crashes the other modes either
        other = ctx.phmm_forward(b, prec)
        clean = fin & (np.arange(ref.size) // 3 % 4 == 0)  # the reads without such a byte (first of every region)
        assert relerr(other[clean], ref[clean]) <= (1e-12 if prec == agx.PHMM_F64_FMA else 1e-6)


def test_reference_kat(ctx, golden_dir):
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, "phmm_test.in"))
    assert "%f" % ctx.phmm_forward(b)[0] == open(os.path.join(golden_dir, "phmm_test.out")).read().strip() == "-4.485565"


@pytest.mark.parametrize("name", NAMES)
def test_f64_text_output_identical(ctx, golden_dir, name):
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, name + ".in"))
    txt = "".join("%f\n" % v for v in ctx.phmm_forward(b))
    assert txt == open(os.path.join(golden_dir, name + ".f.out")).read()


@pytest.mark.parametrize("name", NAMES)
def test_f64_fma_within_1e12(ctx, golden_dir, name):
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, name + ".in"))
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F64_FMA), g17(golden_dir, name)) <= 1e-12


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("prec", [agx.PHMM_F32, agx.PHMM_F32_FMA])
def test_f32_within_1e6_with_rescue(ctx, golden_dir, name, prec):
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, name + ".in"))
    dev = ctx.phmm_batch(b, prec)
    dev.launch()
    got, _ = dev.results()
    assert np.all(np.isfinite(got))
    assert relerr(got, g17(golden_dir, name)) <= 1e-6
    if name == "phmm_far":
        assert dev.info().n_rescued == b.n_pairs  # all eight sit near 1e-96: float underflows
    dev.close()


def test_f32_fill_matches_f32_oracle_where_not_rescued(ctx, oracle, golden_dir):
    """Same float cells as the oracle's float restatement; the last row is summed in double by both, the
    kernel lane-wise and the oracle left to right, so the sums agree to double rounding, not bit for bit."""
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, "phmm_10s.in"))
    dev = ctx.phmm_batch(b, agx.PHMM_F32)
    dev.launch()
    _, sums = dev.results()
    s32, _ = oracle.phmm_batch(b, 2)
    keep = s32 >= 1e-28
    assert keep.sum() > 3000
    assert np.max(np.abs(sums[keep] - s32[keep]) / s32[keep]) <= 1e-14
    dev.close()


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (3, 200), (64, 64), (65, 63), (130, 40), (250, 500),
                                   (400, 1000), (1000, 130), (17, 2048),
                                   # haplotypes no class spans: striped kernel (1536 columns per stripe)
                                   (100, 2100), (40, 3073), (250, 5000), (1000, 5000), (5, 9000)])
def test_shapes_vs_oracle(ctx, oracle, shape):
    R, H = shape
    b = synth.phmm_regions(2, 3, 3, R, H, seed=R * 7 + H, jitter=min(R, H) // 3)
    rng = np.random.default_rng(R + H)
    for arr in (b.read_bases, b.hap_bases):
        arr[rng.random(arr.size) < 0.02] = ord("N")
    s_ref, l_ref = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b, agx.PHMM_F64)
    dev.launch()
    l, s = dev.results()
    assert np.array_equal(s, s_ref) and np.array_equal(l, l_ref)
    dev.close()
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F32), l_ref) <= 1e-6
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F32_FMA), l_ref) <= 1e-6


def test_striped_and_single_pass_pairs_in_one_batch(ctx, oracle):
    """Haplotypes on either side of every span (2048 packed and f64, 2560 f32) in one region; the
    reference's line buffer allows haplotypes up to 5000 (antidiagsPairHMM.c:8,353)."""
    rng = np.random.default_rng(5)
    hap_lens = [300, 1920, 1921, 2048, 2049, 2560, 2561, 3072, 3073, 4608, 4999]
    haps = [synth._ACGT[rng.integers(0, 4, size=n)].tobytes() for n in hap_lens]
    reads = []
    for R in (1, 63, 64, 65, 129, 300):
        src = np.frombuffer(haps[-1], dtype=np.uint8)
        st = int(rng.integers(0, src.size - R))
        q = lambda lo, hi: (rng.integers(lo, hi, size=R) + 33).astype(np.uint8).tobytes()
        reads.append((src[st : st + R].tobytes(), q(6, 42), q(39, 46), q(39, 46), bytes([43]) * R))
    plain = synth.phmm_from_regions([(reads, haps)])
    with_n = synth.phmm_from_regions([(reads, haps)])
    with_n.hap_bases[rng.random(with_n.hap_bases.size) < 0.01] = ord("N")
    # with N in the haplotypes the main launch is the selecting fill's (plain packed cell); without, the striped launch runs
    # beside a looked-up-prior main launch (fast packed cell)
    for b in (with_n, plain):
        assert (bytes(b.hap_bases).count(b"N") > 0) == (b is with_n)
        s_ref, l_ref = oracle.phmm_batch(b, 0)
        for prec, tol in ((agx.PHMM_F64, 0.0), (agx.PHMM_F64_FMA, 1e-12), (agx.PHMM_F32, 1e-6), (agx.PHMM_F32_FMA, 1e-6)):
            dev = ctx.phmm_batch(b, prec)
            dev.launch()
            dev.launch()  # the boundary scratch is reused
            l, s = dev.results()
            assert dev.info().n_launches >= 2
            dev.close()
            if prec == agx.PHMM_F64:
                assert np.array_equal(s, s_ref) and np.array_equal(l, l_ref)
            else:
                assert relerr(l, l_ref) <= tol
        s3, l3 = oracle.phmm_batch(b, 3)
        dev = ctx.phmm_batch(b, agx.PHMM_F64 | agx.PHMM_GATK_PRIOR)
        dev.launch()
        _, s = dev.results()
        dev.close()
        assert np.array_equal(s, s3)


def test_striped_gatk_prior_on_the_longest_reads(ctx, oracle):
    """Reads beyond 3 870 bases against a striped haplotype under the GATK prior: the five-column read table would take more
    than the 160 KiB of LDS (AGX_E_LIMIT until round 3), so the striped launch keeps four columns and divides Qr by 3 in
    its step head -- the results are the five-column table's, bit for bit (checked against the oracle's variant 3; a
    shorter read rides in the same launch: one batch, one table layout)."""
    rng = np.random.default_rng(77)
    hap = synth._ACGT[rng.integers(0, 4, size=4200)].tobytes()
    reads = []
    for R in (4096, 3871, 500):
        src = np.frombuffer(hap, dtype=np.uint8)
        st = int(rng.integers(0, src.size - R + 1))
        rd = src[st : st + R].copy()
        rd[rng.random(R) < 0.02] = ord("N")
        q = lambda lo, hi: (rng.integers(lo, hi, size=R) + 33).astype(np.uint8).tobytes()
        reads.append((rd.tobytes(), q(6, 42), q(39, 46), q(39, 46), bytes([43]) * R))
    hap2 = np.frombuffer(hap, dtype=np.uint8).copy()
    snp = rng.random(hap2.size) < 0.01
    hap2[snp] = synth._ACGT[rng.integers(0, 4, size=int(snp.sum()))]
    hap2 = hap2.tobytes() + synth._ACGT[rng.integers(0, 4, size=300)].tobytes()
    b = synth.phmm_from_regions([(reads, [hap, hap2])])
    s3, l3 = oracle.phmm_batch(b, 3)
    assert np.all(np.isfinite(l3))
    dev = ctx.phmm_batch(b, agx.PHMM_F64 | agx.PHMM_GATK_PRIOR)
    dev.launch()
    l, s = dev.results()
    dev.close()
    assert np.array_equal(s, s3) and np.array_equal(l, l3)
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F32_FMA | agx.PHMM_GATK_PRIOR), l3) <= 1e-6
    # without the prior the four-column table always fitted
    s0, _ = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b, agx.PHMM_F64)
    dev.launch()
    _, s = dev.results()
    dev.close()
    assert np.array_equal(s, s0)


def test_long_reads_keep_a_ring_of_table_rows(ctx, oracle):
    """Reads beyond 363 bases in the double modes: the looked-up-prior kernel keeps a ring of 256 table rows in LDS and refills
    it 64 rows at a time as the wave advances (a whole table would take more than a wave's LDS share).  Ring and whole
    tables in one launch, reads up to the 4096-base limit, every row of the ring reused many times: sums bit for bit against
    the oracle; the GATK prior on a 4096-base read, which no other kernel's table could hold beside a single-pass haplotype."""
    rng = np.random.default_rng(404)
    hap_lens = [600, 590, 333, 37]
    haps = [synth._ACGT[rng.integers(0, 4, size=n)].tobytes() for n in hap_lens]
    long_hap = synth._ACGT[rng.integers(0, 4, size=2000)].tobytes()
    reads = []
    for R in (4096, 2500, 1000, 500, 366, 365, 364, 300, 120, 64, 7):
        src = np.frombuffer(long_hap * 3, dtype=np.uint8)
        st = int(rng.integers(0, src.size - R + 1))
        rd = src[st : st + R].copy()
        rd[rng.random(R) < 0.02] = ord("N")
        q = lambda lo, hi: (rng.integers(lo, hi, size=R) + 33).astype(np.uint8).tobytes()
        reads.append((rd.tobytes(), q(6, 42), q(39, 46), q(39, 46), bytes([43]) * R))
    b = synth.phmm_from_regions([(reads, haps + [long_hap[:1900]])])
    s_ref, l_ref = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b, agx.PHMM_F64)
    dev.launch()
    dev.launch()
    l, s = dev.results()
    dev.close()
    assert np.array_equal(s, s_ref) and np.array_equal(l, l_ref)
    ok = np.isfinite(l_ref)
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F64_FMA)[ok], l_ref[ok]) <= 1e-12
    s3, _ = oracle.phmm_batch(b, 3)
    dev = ctx.phmm_batch(b, agx.PHMM_F64 | agx.PHMM_GATK_PRIOR)
    dev.launch()
    _, s = dev.results()
    dev.close()
    assert np.array_equal(s, s3)
    # uniform long reads fill whole waves of ring tables
    u = synth.phmm_regions(3, 6, 8, 900, 1000, seed=405)
    su, _ = oracle.phmm_batch(u, 0)
    dev = ctx.phmm_batch(u, agx.PHMM_F64)
    dev.launch()
    _, s = dev.results()
    dev.close()
    assert np.array_equal(s, su)


def test_many_striped_pairs_share_the_scratch(ctx, oracle):
    """More long pairs than resident workgroups (8 per CU): every workgroup walks several pairs."""
    b = synth.phmm_regions(3, 40, 20, 12, 2300, seed=9, jitter=4)
    s_ref, _ = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b)
    assert dev.info().n_waves == 2400
    dev.launch()
    _, s = dev.results()
    dev.close()
    assert np.array_equal(s, s_ref)


def test_many_small_regions_and_table_sharing(ctx, oracle):
    """Regions with 1-2 haplotypes force several read tables per wave."""
    parts = [synth.phmm_regions(1, int(n), int(h), int(R), int(H), seed=100 + k, jitter=5)
             for k, (n, h, R, H) in enumerate([(7, 1, 30, 50), (5, 2, 60, 41), (9, 1, 10, 263), (4, 3, 247, 100), (1, 1, 12, 12)] * 6)]
    regions = []
    for p in parts:
        regions += _as_regions(p)
    b = synth.phmm_from_regions(regions)
    s_ref, l_ref = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b)
    dev.launch()
    _, s = dev.results()
    assert np.array_equal(s, s_ref)
    dev.close()
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F32_FMA), l_ref) <= 1e-6  # odd haplotype counts: vacant packed halves


def test_planner_paths_wide_window_and_threaded_pieces(ctx, oracle):
    """The planner counts shapes in a dense table over the batch's window of lengths (<= 2^20 cells) or through a hash
    map (wider windows), and fills waves on pieces of the ordered pair list that are laid end to end afterwards: both
    paths, and a mixed batch large enough for several pieces, against the oracle in every precision."""
    wide = []
    for k, (n, h, R, H) in enumerate([(3, 2, 20, 30), (2, 3, 900, 1990), (4, 5, 150, 300), (1, 1, 4, 7), (2, 2, 640, 33)]):
        wide += _as_regions(synth.phmm_regions(1, n, h, R, H, seed=700 + k, jitter=3))
    big = synth.phmm_regions(40, 48, 14, 150, 380, seed=84, jitter=100)  # 26 880 pairs, nearly all shapes distinct
    for b in (synth.phmm_from_regions(wide), big):
        s_ref, l_ref = oracle_api.phmm_batch_mt(oracle, b, 0) if b is big else oracle.phmm_batch(b, 0)
        for prec, tol in ((agx.PHMM_F64, 0.0), (agx.PHMM_F64_FMA, 1e-12), (agx.PHMM_F32, 1e-6), (agx.PHMM_F32_FMA, 1e-6)):
            dev = ctx.phmm_batch(b, prec)
            dev.launch()
            l, s = dev.results()
            dev.close()
            if prec == agx.PHMM_F64:
                assert np.array_equal(s, s_ref) and np.array_equal(l, l_ref)
            else:
                assert relerr(l, l_ref) <= tol


def test_packed_rescue_plan_is_made_on_first_underflow_and_reused(ctx, oracle, golden_dir):
    """A packed float batch plans and uploads its double rescue pass when a fill first counts a pair below the float
    range (phmm_far: every pair), then reuses it: results of the first, second and third launch agree with the oracle."""
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, "phmm_far.in"))
    _, l_ref = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b, agx.PHMM_F32_FMA)
    got = []
    for _ in range(3):
        dev.launch()
        got.append(dev.results()[0])
    assert dev.info().n_rescued > 0
    dev.close()
    assert relerr(got[0], l_ref) <= 1e-6 and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def _as_regions(p):
    out = []
    for g in range(p.n_regions):
        reads = []
        for r in range(int(p.rreg[g]), int(p.rreg[g + 1])):
            a, z = int(p.roff[r]), int(p.roff[r + 1])
            reads.append(tuple(x[a:z].tobytes() for x in (p.read_bases, p.q_base, p.q_ins, p.q_del, p.q_gcp)))
        haps = [p.hap_bases[int(p.hoff[h]) : int(p.hoff[h + 1])].tobytes() for h in range(int(p.hreg[g]), int(p.hreg[g + 1]))]
        out.append((reads, haps))
    return out


def test_packed_float_cell_variants(ctx, oracle):
    """AGX_PHMM_F32_FMA runs the fast cell (X, Y stored times the next row's 1 - Qg; bases as two-bit codes, the match a
    table lookup) on plain DNA -- haplotypes of A, C, G, T, reads of A, C, G, T, N -- unless a read has a gap-continuation
    quality of Phred 0 ('!': 1 - Qg = 0, the scaling would divide by it); everything else takes the plain cell.  All
    three kinds of batch against the oracle: 1e-6 relative on log10 L, or on L itself where log10 L is near 0."""
    rng = np.random.default_rng(77)
    acgtn = np.frombuffer(b"ACGTN", np.uint8)

    def seq(n, p_n):
        s = acgtn[rng.integers(0, 4, size=n)].copy()
        s[rng.random(n) < p_n] = ord("N")
        return s.tobytes()

    def q(n, lo, hi):
        return (rng.integers(lo, hi, size=n) + 33).astype(np.uint8).tobytes()

    def batch(gcp_lo, hap_n):
        regions = []
        for R, H, nr, nh in ((1, 86, 3, 2), (3, 86, 3, 3), (40, 120, 5, 4), (100, 300, 4, 4), (120, 33, 3, 1)):
            reads = [(seq(R, 0.05), q(R, 2, 42), q(R, 20, 46), q(R, 20, 46), q(R, gcp_lo, 20)) for _ in range(nr)]
            regions.append((reads, [seq(H + int(rng.integers(0, 9)), hap_n) for _ in range(nh)]))
        return synth.phmm_from_regions(regions)

    for gcp_lo, hap_n in ((1, 0.0), (0, 0.0), (1, 0.3)):  # fast; plain because of '!'; plain because of N haplotypes
        b = batch(gcp_lo, hap_n)
        assert (b.q_gcp.min() == 33) == (gcp_lo == 0) and (bytes(b.hap_bases).count(b"N") > 0) == (hap_n > 0)
        _, l_ref = oracle.phmm_batch(b, 0)
        got = ctx.phmm_forward(b, agx.PHMM_F32_FMA)
        ok = np.isfinite(l_ref)
        assert np.array_equal(np.isfinite(got), ok)
        d = np.abs(got[ok] - l_ref[ok])
        assert not (d > 1e-6 * np.abs(l_ref[ok])).any()  # relative only: likelihoods near 1 go through the accuracy guard


def test_read_trains_change_nothing(ctx, oracle):
    """AGX_OPT_PHMM_TRAINS: two reads of a region may share their lane groups in the packed float fill (the second enters
    behind a reset row as the first leaves).  The state behind the reset row is the state a fresh group starts with, so
    forcing trains on must give the results of the plain schedule BIT FOR BIT -- uniform regions, odd haplotype and read
    counts, mixed lengths, N in reads, the GATK prior, underflowing pairs (rescue plan), bound results -- and within 1e-6
    of the oracle."""
    far = synth.phmm_regions(2, 8, 4, 100, 300, seed=81)
    far.read_bases[:] = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(82).integers(0, 4, far.read_bases.size)]
    nread = synth.phmm_regions(3, 7, 6, 80, 200, seed=93)
    nread.read_bases[np.random.default_rng(94).random(nread.read_bases.size) < 0.03] = ord("N")
    cases = [("uniform", synth.phmm_regions(6, 16, 16, 100, 300, seed=90), agx.PHMM_F32_FMA),
             ("odd counts", synth.phmm_regions(5, 7, 5, 100, 300, seed=91), agx.PHMM_F32_FMA),
             ("mixed lengths", synth.phmm_regions(6, 12, 8, 120, 260, seed=92, jitter=60), agx.PHMM_F32_FMA),
             ("N in reads", nread, agx.PHMM_F32_FMA),
             ("gatk prior", synth.phmm_regions(4, 8, 6, 100, 300, seed=95), agx.PHMM_F32_FMA | agx.PHMM_GATK_PRIOR),
             ("long reads", synth.phmm_regions(2, 6, 4, 290, 400, seed=96), agx.PHMM_F32_FMA),
             ("underflow", far, agx.PHMM_F32_FMA)]
    waves_off = {}
    try:
        for name, p, prec in cases:
            _, ref = oracle.phmm_batch(p, 3 if prec & agx.PHMM_GATK_PRIOR else 0)
            res = {}
            for opt in (agx.PHMM_TRAINS_OFF, agx.PHMM_TRAINS_ON):
                ctx.set_option(agx.OPT_PHMM_TRAINS, opt)
                dev = ctx.phmm_batch(p, prec)
                waves = dev.info().n_waves
                dev.launch()
                l, s = dev.results()
                dev.close()
                res[opt] = (l, s, waves)
            l0, s0, w0 = res[agx.PHMM_TRAINS_OFF]
            waves_off[name] = w0
            l1, s1, w1 = res[agx.PHMM_TRAINS_ON]
            assert np.array_equal(s0, s1) and np.array_equal(l0, l1), name
            if name in ("uniform", "odd counts"):
                assert w1 < w0, (name, w0, w1)  # trains were formed: fewer waves (mixed regions may need as many, or more)
            ok = np.isfinite(ref)
            assert relerr(l1[ok], ref[ok]) <= 1e-6, name
        # bound results through a train launch
        ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_ON)
        p = cases[1][1]
        dev = ctx.phmm_batch(p, agx.PHMM_F32_FMA)
        out = agx.host_array(p.n_pairs + 2, np.float64)
        out[:] = 7.0
        dev.bind_results(out[:p.n_pairs])
        dev.launch()
        dev.results((out[:p.n_pairs], None), want_sums=False)
        dev.close()
        ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_OFF)
        plain = ctx.phmm_forward(p, agx.PHMM_F32_FMA)
        assert np.array_equal(out[:p.n_pairs], plain) and np.all(out[p.n_pairs:] == 7.0)
    finally:
        ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_AUTO)
    # the default: config 3's shape and size forms trains by itself, small batches do not; at that size too the sums are
    # the plain schedule's bit for bit (all 65 536 pairs)
    big = synth.phmm_regions(64, 64, 16, 100, 300, seed=3)
    dev = ctx.phmm_batch(big, agx.PHMM_F32_FMA)
    assert dev.info().n_waves == 4096
    dev.launch()
    l_auto, s_auto = dev.results()
    dev.close()
    try:
        ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_OFF)
        dev = ctx.phmm_batch(big, agx.PHMM_F32_FMA)
        assert dev.info().n_waves == 8192
        dev.launch()
        l_off, s_off = dev.results()
        dev.close()
    finally:
        ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_AUTO)
    assert np.array_equal(s_auto, s_off) and np.array_equal(l_auto, l_off)
    small = ctx.phmm_batch(cases[0][1], agx.PHMM_F32_FMA)
    assert small.info().n_waves == waves_off["uniform"]
    small.close()


def test_plain_packed_cell_on_a_config3_sized_batch(ctx, oracle):
    """The plain cell of the packed float fill (one Phred-0 gap-continuation quality in the batch keeps the fast cell out) in
    the build for 16-lane groups, whose last-row sum is taken behind the loop: config 3's shape and size, the first two
    regions against the oracle, everything against the fast cell's results of the unmodified batch."""
    p = synth.phmm_regions(64, 64, 16, 100, 300, seed=11)
    fast = ctx.phmm_forward(p, agx.PHMM_F32_FMA)
    q = synth.phmm_regions(64, 64, 16, 100, 300, seed=11)
    q.q_gcp[int(q.roff[-1]) - 1] = ord("!")  # the last read's last base
    dev = ctx.phmm_batch(q, agx.PHMM_F32_FMA)
    assert dev.info().n_waves == 8192  # the plain cell does not pair reads
    dev.launch()
    plain, _ = dev.results()
    dev.close()
    _, ref = oracle.phmm_batch(q.regions(0, 2), 0)
    assert relerr(plain[: ref.size], ref) <= 1e-6
    same = np.ones(p.n_pairs, bool)
    same[-16:] = False  # the changed read's pairs
    assert relerr(plain[same], fast[same]) <= 1e-6


def test_degenerate_pairs(ctx, oracle):
    b = synth.phmm_from_regions([([(b"", b"", b"", b"", b""), (b"A", b"I", b"I", b"I", b"+")], [b"", b"A", b"ACGT"])])
    got = ctx.phmm_forward(b)
    _, ref = oracle.phmm_batch(b, 0)
    assert got.size == 6
    assert np.array_equal(np.isneginf(got), np.isneginf(ref))
    ok = np.isfinite(ref)
    assert np.array_equal(got[ok], ref[ok])
    assert ctx.phmm_forward(synth.phmm_from_regions([])).size == 0


def test_limits_fail_loudly(ctx):
    b = synth.phmm_regions(1, 1, 1, 10, 16385, seed=1)
    with pytest.raises(agx.AgxError) as e:
        ctx.phmm_forward(b)
    assert e.value.code == agx.E_LIMIT


def test_function_seam_matches_reference_signature(ctx, oracle, golden_dir):
    """agx_pairHMM() has the argument list of antidiagsPairHMM.c:120 and takes probabilities."""
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, "phmm_test.in"))
    R, H = int(b.roff[1]), int(b.hoff[1])
    lut = np.array([oracle.lib.oracle_phred_to_prob(c) for c in range(256)])
    q = [np.ascontiguousarray(lut[t[:R]]) for t in (b.q_base, b.q_ins, b.q_del, b.q_gcp)]
    lh = C.c_double(123.0)
    scratch = np.zeros(9 * (min(R, H) + 1))
    rd = b.read_bases[:R].tobytes()
    hp = b.hap_bases[:H].tobytes()
    agx.lib().agx_pairHMM(C.addressof(lh), scratch.ctypes.data, scratch.ctypes.data, scratch.ctypes.data, rd, hp, R, H,
                          *(x.ctypes.data for x in q))
    assert lh.value == g17(golden_dir, "phmm_test")[0]
    # a haplotype of the reference's maximum line length goes through the striped kernel
    big = synth.phmm_regions(1, 1, 1, 120, 5000, seed=21)
    R, H = int(big.roff[1]), int(big.hoff[1])
    q = [np.ascontiguousarray(lut[t[:R]]) for t in (big.q_base, big.q_ins, big.q_del, big.q_gcp)]
    agx.lib().agx_pairHMM(C.addressof(lh), scratch.ctypes.data, scratch.ctypes.data, scratch.ctypes.data,
                          big.read_bases[:R].tobytes(), big.hap_bases[:H].tobytes(), R, H, *(x.ctypes.data for x in q))
    assert lh.value == oracle.phmm_batch(big, 0)[1][0]


def test_relaunch_is_idempotent_and_info(ctx, oracle):
    b = synth.phmm_regions(8, 16, 8, 100, 300, seed=3)
    dev = ctx.phmm_batch(b, agx.PHMM_F32)
    dev.launch()
    first, _ = dev.results()
    dev.launch()
    dev.launch()
    again, _ = dev.results()
    assert np.array_equal(first, again)
    _, ref = oracle.phmm_batch(b, 0)
    assert relerr(first, ref) <= 1e-6
    i = dev.info()
    assert i.n_pairs == 8 * 16 * 8 and i.cells == b.cells() and i.padded_cells >= i.cells
    dev.close()


@pytest.mark.parametrize("prec", [agx.PHMM_F32, agx.PHMM_F32_FMA])
def test_full_size_config3_sample_and_linearity(ctx, oracle, prec):
    """BASELINE config 3 at full size (65 536 pairs, R=100, H=300, fp32).  EVERY pair against the fp64 oracle
    (threaded over the host cores) within 1e-6 relative on the log10 likelihood -- SURVEY 8d's definition; on the raw
    likelihood that is about 1e-5 relative at log10 = -4 -- and a size-independent property: results do not depend on
    how pairs are grouped into regions/waves (region order reversed => same values)."""
    b = synth.phmm_regions(64, 64, 16, 100, 300, seed=3)
    assert b.n_pairs == 65536
    got = ctx.phmm_forward(b, prec)
    _, ref = oracle_api.phmm_batch_mt(oracle, b, 0)
    assert relerr(got, ref) <= 1e-6
    rev = synth.phmm_from_regions(_as_regions(b)[::-1])
    got_rev = ctx.phmm_forward(rev, prec)
    assert np.array_equal(got_rev.reshape(64, -1)[::-1].reshape(-1), got)


def test_full_size_config5_fp64(ctx, oracle):
    """BASELINE config 5 at full size (262 144 pairs, R=250, H=500, fp64, tolerance 1e-12 vs
    pairHMMmatrix.c semantics).  The threaded oracle checks 32 768 pairs (every 8th of the 512 regions) -- bit for
    bit, which implies the tolerance; the rest is checked by regrouping invariance (regions in
    reverse order give the same values) and by F64_FMA agreeing to 1e-12 everywhere."""
    b = synth.phmm_regions(512, 32, 16, 250, 500, seed=5)
    assert b.n_pairs == 262144
    got = ctx.phmm_forward(b, agx.PHMM_F64)
    regs = _as_regions(b)
    sample = synth.phmm_from_regions(regs[::8])
    _, ref = oracle_api.phmm_batch_mt(oracle, sample, 0)
    assert np.array_equal(got.reshape(512, -1)[::8].reshape(-1), ref)
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F64_FMA), got) <= 1e-12
    rev = synth.phmm_from_regions(_as_regions(b)[::-1])
    assert np.array_equal(ctx.phmm_forward(rev, agx.PHMM_F64).reshape(512, -1)[::-1].reshape(-1), got)


def test_largest_supported_shapes(ctx, oracle):
    """R = 4096 needs a 139 KB read table (most of the 160 KB LDS); H = 2048 spans 64 lanes x 32 columns."""
    b = synth.phmm_regions(1, 2, 2, 4096, 2048, seed=77)
    s_ref, l_ref = oracle.phmm_batch(b, 0)
    dev = ctx.phmm_batch(b, agx.PHMM_F64)
    dev.launch()
    l, s = dev.results()
    assert np.array_equal(s, s_ref)
    dev.close()
    got32 = ctx.phmm_forward(b, agx.PHMM_F32)
    assert relerr(got32, l_ref) <= 1e-6
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F64_FMA), l_ref) <= 1e-12
    b2 = synth.phmm_regions(1, 2, 3, 4096, 1900, seed=78)  # packed float kernel: 64 lanes x 30 columns
    assert relerr(ctx.phmm_forward(b2, agx.PHMM_F32_FMA), oracle.phmm_batch(b2, 0)[1]) <= 1e-6
    # a read of the full 4096 rows against short haplotypes (R > H): too long for the looked-up-prior fill's tables, so
    # the double modes take phmm_fill; a 700-row read beside it in another batch still runs the looked-up priors
    rng = np.random.default_rng(79)
    for R in (4096, 700):
        q = lambda lo, hi: bytes(rng.integers(lo + 33, hi + 33, size=R).astype(np.uint8))
        # (R > H by thousands of rows underflows even in double, in the reference too: sums 0, log10 -inf on both sides;
        # the 700-row read is a window of its first haplotype with 1 % substitutions: finite likelihoods)
        haps = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in ((300, 200, 37) if R == 4096 else (900, 800, 750))]
        src = np.frombuffer(haps[0], np.uint8)[50:50 + R].copy() if R == 700 else rng.choice(np.frombuffer(b"ACGT", np.uint8), R)
        flip = rng.random(R) < 0.01
        src[flip] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(flip.sum()))
        bases = bytes(src)
        b3 = synth.phmm_from_regions([([(bases, q(6, 42), q(39, 46), q(39, 46), bytes([43]) * R)], haps)])
        s_ref, l_ref = oracle.phmm_batch(b3, 0)
        dev = ctx.phmm_batch(b3, agx.PHMM_F64)
        dev.launch()
        l, s = dev.results()
        dev.close()
        assert np.array_equal(s, s_ref) and np.array_equal(l, l_ref)
        fma, pk = ctx.phmm_forward(b3, agx.PHMM_F64_FMA), ctx.phmm_forward(b3, agx.PHMM_F32_FMA)
        fin = np.isfinite(l_ref)
        for got, tol in ((fma, 1e-12), (pk, 1e-6)):
            assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], l_ref[~fin])
            assert relerr(got[fin], l_ref[fin]) <= tol


def test_gatk_prior_option(ctx, oracle, golden_dir):
    """8f n4, default off: mismatch prior Qr/3.  Not the reference's behaviour -- checked against the
    oracle's own restatement (variant 3); the reference-mode result must differ."""
    b, _, _ = agx.read_phmm_text(os.path.join(golden_dir, "phmm_10s.in"))
    s_ref, l_ref = oracle.phmm_batch(b, 3)
    dev = ctx.phmm_batch(b, agx.PHMM_F64 | agx.PHMM_GATK_PRIOR)
    dev.launch()
    l, s = dev.results()
    dev.close()
    assert np.array_equal(s, s_ref)
    assert not np.array_equal(l, g17(golden_dir, "phmm_10s"))
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F32 | agx.PHMM_GATK_PRIOR), l_ref) <= 1e-6
    # (the packed float fill alone reaches 1.2e-6 on ten of this file's pairs with this prior -- long reads that fit
    # well: the accuracy guard sends them through the double rescue plan)
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F32_FMA | agx.PHMM_GATK_PRIOR), l_ref) <= 1e-6
    assert relerr(ctx.phmm_forward(b, agx.PHMM_F64_FMA | agx.PHMM_GATK_PRIOR), l_ref) <= 1e-12


def test_one_shot_forward_of_a_large_batch_runs_in_pieces(ctx, oracle):
    """agx_phmm_forward sends a batch of more than 8e9 cells through in pieces of whole regions (piece k + 1 planned and
    uploaded beside the fill of piece k): the results are those of the one-batch path, bit for bit in double."""
    p = synth.phmm_regions(150, 32, 16, 250, 500, seed=61, jitter=20)
    assert p.cells() > 8.0e9 * 1.05
    for prec in (agx.PHMM_F64, agx.PHMM_F32_FMA):
        got = ctx.phmm_forward(p, prec)
        dev = ctx.phmm_batch(p, prec)
        dev.launch()
        want, _ = dev.results()
        dev.close()
        assert np.array_equal(got, want)
    sub = p.regions(140, 143)
    first = int(sum((p.rreg[g + 1] - p.rreg[g]) * (p.hreg[g + 1] - p.hreg[g]) for g in range(140)))
    _, l_ref = oracle.phmm_batch(sub, 0)
    assert np.array_equal(ctx.phmm_forward(p, agx.PHMM_F64)[first:first + sub.n_pairs], l_ref)


@pytest.mark.parametrize("seed", [101, 202, 303])
def test_float_modes_hold_1e6_across_read_lengths(ctx, oracle, seed):
    """the packed float fill with its accuracy guard (pairs whose |log10 L| is below 0.18 sqrt(R + 8) --
    0.40 with the GATK prior -- are recomputed in double) and the order-exact float fill, over read lengths 8 ... 2000
    with perfect, 1 % and 5 % mismatching reads, against the device's bit-identical double mode: 1e-6 relative on
    log10 L everywhere, and the guard must not send config 3's shape to the double pass.  That yardstick is itself held
    against the oracle, bit for bit, at reads of 8, 100 and 1000 bases (VERDICT weak 3: a comparison of the device with itself)."""
    worst = 0.0
    for R in (8, 30, 100, 250, 600, 1000, 2000):
        H = R + 120
        n_regions = max(1, min(16, int(1.5e9 / (R * H) / 256)))
        for sub in (0.0, 0.01, 0.05):
            b = synth.phmm_regions(n_regions, 16, 16, R, H, seed=seed * 100 + R, sub_rate=sub, jitter=max(1, R // 5))
            for flag in (0, agx.PHMM_GATK_PRIOR):
                ref = ctx.phmm_forward(b, agx.PHMM_F64 | flag)
                if R in (8, 100, 1000):  # the yardstick itself, against the oracle: not a comparison of the device with itself
                    assert np.array_equal(ref, oracle_api.phmm_batch_mt(oracle, b, 3 if flag else 0)[1]), (R, sub, flag)
                ok = np.isfinite(ref)
                for prec in (agx.PHMM_F32_FMA, agx.PHMM_F32):
                    got = ctx.phmm_forward(b, prec | flag)
                    e = float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])))
                    assert e <= 1e-6, (R, sub, flag, prec, e)
                    worst = max(worst, e)
    c3 = synth.phmm_regions(8, 64, 16, 100, 300, seed=seed)
    dev = ctx.phmm_batch(c3, agx.PHMM_F32_FMA)
    dev.launch()
    dev.results()
    assert dev.info().n_rescued == 0
    dev.close()


def test_bound_results_arrive_in_the_callers_page_locked_array(ctx, oracle):
    """agx_phmm_batch_bind_results: a packed float batch in output order computes log10(sum) - log10(C) in its fill and
    writes it into the caller's page-locked array; odd haplotype counts (vacant halves), pairs that go to the rescue plan
    (the flag sends the host the long way), rebinding, a mixed batch and the double mode (both: a hint)."""
    for haps in (16, 5):
        p = synth.phmm_regions(6, 16, haps, 100, 300, seed=70 + haps)
        _, ref = oracle.phmm_batch(p, 0)
        dev = ctx.phmm_batch(p, agx.PHMM_F32_FMA)
        out = agx.host_array(p.n_pairs + 4, np.float64)
        out[:] = 7.0
        dev.bind_results(out[:p.n_pairs])
        for _ in range(2):
            dev.launch()
            got, _ = dev.results((out[:p.n_pairs], None), want_sums=False)
            assert relerr(out[:p.n_pairs], ref) <= 1e-6 and np.all(out[p.n_pairs:] == 7.0) and dev.info().n_rescued == 0
        plain = ctx.phmm_forward(p, agx.PHMM_F32_FMA)
        assert np.array_equal(out[:p.n_pairs], plain)      # the fill's log10 is the log10 kernel's
        other, sums = dev.results()                           # fetched elsewhere, with the sums: the usual path
        assert np.array_equal(other, plain) and np.all(sums > 0)
        dev.bind_results(None)
        dev.launch()
        assert np.array_equal(dev.results()[0], plain)
        with pytest.raises(agx.AgxError):
            dev.bind_results(np.empty(p.n_pairs, np.float64))
        dev.close()
    # unrelated reads underflow float: every pair is rescued in double, bound or not
    far = synth.phmm_regions(2, 8, 4, 100, 300, seed=81)
    far.read_bases[:] = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(82).integers(0, 4, far.read_bases.size)]
    _, ref = oracle.phmm_batch(far, 0)
    dev = ctx.phmm_batch(far, agx.PHMM_F32_FMA)
    out = agx.host_array(far.n_pairs, np.float64)
    dev.bind_results(out)
    dev.launch()
    dev.results((out, None), want_sums=False)
    assert relerr(out, ref) <= 1e-6 and dev.info().n_rescued == far.n_pairs
    dev.close()
    for p, prec in ((synth.phmm_regions(4, 8, 4, 100, 300, seed=83, jitter=30), agx.PHMM_F32_FMA), (synth.phmm_regions(2, 8, 4, 100, 300, seed=84), agx.PHMM_F64)):
        _, ref = oracle.phmm_batch(p, 0)
        dev = ctx.phmm_batch(p, prec)
        out = agx.host_array(p.n_pairs, np.float64)
        dev.bind_results(out)                                 # a hint for these
        dev.launch()
        dev.results((out, None), want_sums=False)
        assert relerr(out, ref) <= 1e-6
        dev.close()


ODD_BYTES = [ord(c) for c in "acgtnRY-*"] + [0x01, 0xff]


@pytest.mark.parametrize("byte", ODD_BYTES, ids=lambda v: "0x%02x" % v)
def test_bytes_outside_the_alphabets(ctx, oracle, byte):
    """One byte outside ACGTN (reads) / ACGT (haplotypes) -- lower case, IUPAC codes, gap characters, control and high bytes --
    as the first byte of the first sequence or the last of the last, in a read or in a haplotype, takes the batch off the
    plain-DNA kernels.  The reference compares bytes (n is not N, a matches only a): every precision at its usual bar."""
    base = synth.phmm_regions(2, 3, 3, 40, 120, seed=600, jitter=9)
    for track, at in (("read_bases", 0), ("read_bases", -1), ("hap_bases", 0), ("hap_bases", -1)):
        b = synth.PhmmBatch(*(getattr(base, f).copy() for f in ("read_bases", "q_base", "q_ins", "q_del", "q_gcp", "roff", "hap_bases", "hoff", "rreg", "hreg")))
        getattr(b, track)[at] = byte
        s_ref, l_ref = oracle.phmm_batch(b, 0)
        assert np.all(np.isfinite(l_ref))
        dev = ctx.phmm_batch(b, agx.PHMM_F64)
        dev.launch()
        l, s = dev.results()
        dev.close()
        assert np.array_equal(s, s_ref) and np.array_equal(l, l_ref), (track, at)
        assert relerr(ctx.phmm_forward(b, agx.PHMM_F64_FMA), l_ref) <= 1e-12, (track, at)
        for prec in (agx.PHMM_F32, agx.PHMM_F32_FMA):
            assert relerr(ctx.phmm_forward(b, prec), l_ref) <= 1e-6, (track, at, prec)


def test_a_quality_byte_below_the_phred_range_keeps_trains_out(ctx, oracle):
    """A quality byte below '!' is a "probability" above 1: a first read whose state ran to infinity there would hand NaN to
    the second read of a train.  With AGX_PHMM_TRAINS_ON such a batch must plan as with trains off (the same waves) and give the
    oracle's results wherever those are finite; the same batch without the byte does form trains."""
    clean = synth.phmm_regions(5, 7, 5, 100, 300, seed=91)
    wild = synth.phmm_regions(5, 7, 5, 100, 300, seed=91)
    wild.q_ins[int(wild.roff[3]) + 17] = ord(" ")
    _, ref = oracle.phmm_batch(wild, 0)
    res = {}
    try:
        for name, b in (("clean", clean), ("wild", wild)):
            for opt in (agx.PHMM_TRAINS_OFF, agx.PHMM_TRAINS_ON):
                ctx.set_option(agx.OPT_PHMM_TRAINS, opt)
                dev = ctx.phmm_batch(b, agx.PHMM_F32_FMA)
                waves = dev.info().n_waves
                dev.launch()
                res[(name, opt)] = (waves, dev.results()[0])
                dev.close()
    finally:
        ctx.set_option(agx.OPT_PHMM_TRAINS, agx.PHMM_TRAINS_AUTO)
    assert res[("clean", agx.PHMM_TRAINS_ON)][0] < res[("clean", agx.PHMM_TRAINS_OFF)][0]
    assert res[("wild", agx.PHMM_TRAINS_ON)][0] == res[("wild", agx.PHMM_TRAINS_OFF)][0]
    ok = np.isfinite(ref)
    assert ok.sum() >= ref.size - 5  # (the byte sits in one read: at most its five pairs)
    for opt in (agx.PHMM_TRAINS_OFF, agx.PHMM_TRAINS_ON):
        assert relerr(res[("wild", opt)][1][ok], ref[ok]) <= 1e-6


def test_plan_on_a_device_is_the_plan_only_plan():
    """A plan does not depend on whether a device is there: one small case of tests/phmm_plan_cases.py per kernel family -- F64
    with looked-up priors, F32, F32_FMA -- created on device 0 in a child process under AGX_TRACE_CREATE prints the main and
    image digests, the flags and the info fields of tests/golden/phmm_plan_digests.json.  Plan-only batches are tiled for 256
    CUs, an MI355X's count; on a device of another count the test skips.
    The same child launches the packed mismatch ladder of tests/phmm_range_cases.py, which crosses the rescue threshold
    (tests/test_phmm_range_gpu.py: n_rescued > 0): its rescue plan, made at that first underflow, prints the digest that the
    same batch planned as F64 under AGX_PHMM_NO_LUT has as its main one."""
    import json
    import re

    from tests import phmm_plan_cases as pc

    with open(os.path.join(os.path.dirname(__file__), "golden", "phmm_plan_digests.json")) as f:
        golden = json.load(f)
    names = ["jitter_f64", "corpus_f32", "jitter_pk", "ladder_pk"]
    got, err = pc.run_group("default", names=names, device=True, run=("ladder_pk",), timeout=120)
    assert sorted(got) == sorted(names), err[-2000:]
    n_cu = set(re.findall(r"^\[agx_phmm_batch_create\] planned for (\d+) CUs$", err, flags=re.M))
    if n_cu != {"256"}:
        pytest.skip("the context reports %s CUs: its plans are tiled for that count, the fixture's for 256" % sorted(n_cu))
    for name in names:
        want = golden[name]
        for k in ("main", "image", "flags"):
            assert got[name][k] == want[k], (name, k, got[name], want, err[-2000:])
        assert {k: v for k, v in got[name]["info"].items() if k != "n_rescued"} == {k: v for k, v in want["info"].items() if k != "n_rescued"}, name
    assert _flags_of(golden["jitter_f64"])["lut_prior"] == 1
    assert got["ladder_pk"]["info"]["n_rescued"] > 0, got["ladder_pk"]
    assert got["ladder_pk"]["rescue"] == golden["ladder_f64_no_lut"]["main"], (got["ladder_pk"], err[-2000:])
    assert all("rescue" not in got[n] for n in names[:3])


def _flags_of(entry):
    words = entry["flags"].split()
    return dict(zip(words[0::2], (int(v) for v in words[1::2])))
