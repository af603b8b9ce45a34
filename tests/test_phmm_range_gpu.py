"""Every PairHMM fill at the edges of its quality range (Phred 0 ... 93) and of the float range, against the fp64 oracle.

The cases are those of tests/phmm_range_cases.py; tests/test_phmm_range_cpu.py proves from the oracle alone that they stand
where they are meant to.  Bars (tests/phmm_widths.py figures / meets): AGX_PHMM_F64 sums and log10 L bit for bit, the NaN / -inf
pattern included; AGX_PHMM_F64_FMA 1e-12 relative on log10 L; the float modes 1e-6 relative on log10 L, or 1e-6 / ln 10
absolute near 0.

* Clean profiles (Qi + Qd <= 1 in every row): the lengths that widths 4, 19 and 32 make on 3 and 16 lanes, a ring read (double
  modes), a striped pair per span; every precision, the GATK prior, the twin with one N in a haplotype (the selecting fill, the
  plain packed cell), and read trains forced on: the plain schedule's results bit for bit.
* Runaway profiles (rows with Qi + Qd > 1: legal bytes, but the state grows without bound; the reference gives negative sums and
  NaN): AGX_PHMM_F64 has the oracle's bits and its NaN pattern, the other modes end without error -- and a region whose FIRST
  read runs away must leave its clean reads alone, whether read trains are asked for or not.
* The rescue ladders: log10 L in steps of a tenth of a decade across log10(AGX_PHMM_F32_RESCUE / (FLT_MAX / 16)) = -65.33, also
  under deletion qualities of Phred 80 ... 93, where the fast packed cell's stored M x Qd (1 - Qg+) is ten decades below the sum.
  Every pair at the float bar, and as many pairs sent to the double pass as the oracle's sums say.
* The guard ladder: |log10 L| on both sides of the accuracy guard's 0.18 sqrt(R + 8) (0.40 with the GATK prior)."""
import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
from tests import oracle_api
from tests import phmm_range_cases as rc
from tests import phmm_widths as pw

pytestmark = pytest.mark.gpu

FLOATS = (agx.PHMM_F32, agx.PHMM_F32_FMA)
TRAINS = (agx.PHMM_TRAINS_OFF, agx.PHMM_TRAINS_ON)


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


def _report(what, recs):
    """The worst float error of a case, per leg: printed (pytest -s), asserted by the caller."""
    worst = {}
    for r in recs:
        if r["prec"] & 0xff in FLOATS:
            worst[r["leg"]] = max(worst.get(r["leg"], 0.0), r["rel_log"])
    print("RANGE %s: worst relative error of log10 L %.3g; per leg %s" % (what, max(worst.values(), default=0.0), {k: "%.3g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("name", list(rc.CLEAN))
def test_clean_profile_in_every_fill(ctx, oracle, name):
    recs = []
    for where, b, fams in rc.clean_batches(name):
        rc.legs(ctx, oracle, where, b, fams, recs)
    _report(name, recs)
    assert len(recs) == 6 * 16 + 6 + 16
    for r in recs:
        assert pw.meets(r["prec"], r), r
        assert r.get("same_bits_as_off", True), r  # read trains change nothing
        if "waves_off" in r:
            assert r["n_waves"] <= r["waves_off"], r
            if "twin" in r["leg"]:
                assert r["n_waves"] == r["waves_off"], r  # the plain cell has no trains
            elif r["where"] in ("C19 G16", "C32 G16"):
                # haplotypes of 289 ... 512 columns take ten lanes or more: at most six groups a wave, and a region's three
                # reads fill six groups without trains, four with -- trains did form
                assert r["n_waves"] < r["waves_off"], r


@pytest.mark.parametrize("name", list(rc.RUNAWAY))
def test_runaway_profile_ends_in_every_fill(ctx, oracle, name):
    """Garbage in: the bars of test_quality_bytes_above_0x7f_read_as_signed_char."""
    nan = 0
    for G in rc.LANES:
        b = rc.shape_batch(name, 19, G)
        s_ref, l_ref = oracle.phmm_batch(b, 0)
        fin = np.isfinite(l_ref)
        nan += int(np.isnan(l_ref).sum())
        l, s, _ = pw.run(ctx, b, agx.PHMM_F64)
        assert np.array_equal(l[fin], l_ref[fin]) and np.array_equal(s[fin], s_ref[fin]), G
        assert np.array_equal(np.isnan(l), np.isnan(l_ref)) and np.array_equal(l[~fin], l_ref[~fin], equal_nan=True), G
        for prec, trains in ((agx.PHMM_F64_FMA, None), (agx.PHMM_F32, None), (agx.PHMM_F32_FMA, agx.PHMM_TRAINS_OFF), (agx.PHMM_F32_FMA, agx.PHMM_TRAINS_ON)):
            assert pw.run(ctx, b, prec, trains)[0].size == l_ref.size
    assert nan > 0 or name == "all1-93"  # (one row in a thousand runs away there: the short shapes may have none that shows)


@pytest.mark.parametrize("R", rc.TRAIN_READS)
@pytest.mark.parametrize("name", list(rc.RUNAWAY))
def test_runaway_first_read_leaves_the_clean_reads_alone(ctx, oracle, name, R):
    """Regions of seven reads whose first runs away: with read trains asked for, the batch plans the waves it plans without
    (the host keeps trains out of a batch with such a row), and the clean reads' pairs are at the float bar against the oracle
    and the same bits under both options."""
    b, clean = rc.train_batch(name, R)
    s_ref, l_ref = oracle_api.phmm_batch_mt(oracle, b, 0)
    assert np.all(np.isfinite(l_ref[clean]))
    got = {}
    for opt in TRAINS:
        l, s, i = pw.run(ctx, b, agx.PHMM_F32_FMA, opt)
        fig = pw.figures(agx.PHMM_F32_FMA, l[clean], s[clean], l_ref[clean], s_ref[clean])
        print("RANGE %s first, R %d, trains %d: %s, worst relative %.3g, %d waves" % (name, R, opt, fig, rc.rel_err(l[clean], l_ref[clean])[0], i["n_waves"]))
        got[opt] = (l, s, i, fig)
    for opt in TRAINS:
        assert pw.meets(agx.PHMM_F32_FMA, got[opt][3]), (opt, got[opt][3])
    assert np.array_equal(got[TRAINS[0]][0][clean], got[TRAINS[1]][0][clean]) and np.array_equal(got[TRAINS[0]][1][clean], got[TRAINS[1]][1][clean])
    assert got[TRAINS[0]][2]["n_waves"] == got[TRAINS[1]][2]["n_waves"]
    # the same regions with the usual qualities on every read do pair their reads
    u = rc.qualify(b, rc.USUAL, np.random.default_rng(R), [int(b.rreg[g]) for g in range(b.n_regions)])
    assert pw.run(ctx, u, agx.PHMM_F32_FMA, TRAINS[1])[2]["n_waves"] < pw.run(ctx, u, agx.PHMM_F32_FMA, TRAINS[0])[2]["n_waves"]


@pytest.mark.parametrize("name", rc.LADDER_PROFILES)
def test_rescue_ladder(ctx, oracle, name):
    for what, b in rc.ladders(name):
        s_ref, l_ref = oracle.phmm_batch(b, 0)
        lo, hi = rc.rescued_range(l_ref)
        waves = {}
        for prec in FLOATS:
            for opt in TRAINS:
                l, s, i = pw.run(ctx, b, prec, opt)
                fig = pw.figures(prec, l, s, l_ref, s_ref)
                print("RANGE ladder %s, %s, precision %d, trains %d: %s, worst relative %.3g, %d rescued of %d ... %d" % (name, what, prec, opt, fig, rc.rel_err(l, l_ref)[0], i["n_rescued"], lo, hi))
                assert pw.meets(prec, fig), (what, prec, opt, fig)
                assert lo <= i["n_rescued"] <= hi, (what, prec, opt, i["n_rescued"], lo, hi)
                waves[(prec, opt)] = i["n_waves"]
        if what == "mismatches":
            # one region of equal reads: forced trains pair them.  (Not fewer waves here -- 120 of two trains against 96 of five
            # reads, every read with a table of its own; forced trains skip the planner's comparison.  Other waves than
            # without: the train launch did run.)
            assert waves[(agx.PHMM_F32_FMA, TRAINS[1])] != waves[(agx.PHMM_F32_FMA, TRAINS[0])], (what, waves)


def test_guard_ladder(ctx, oracle):
    b, _ = rc.guard_ladder()
    for flag, variant in ((0, 0), (agx.PHMM_GATK_PRIOR, 3)):
        s_ref, l_ref = oracle.phmm_batch(b, variant)
        for prec in FLOATS:
            l, s, i = pw.run(ctx, b, prec | flag)
            fig = pw.figures(prec, l, s, l_ref, s_ref)
            print("RANGE guard ladder, precision %d, prior %d: %s, %d rescued" % (prec, flag, fig, i["n_rescued"]))
            assert pw.meets(prec, fig), (prec, flag, fig)
            if prec == agx.PHMM_F32_FMA:  # the guard did send pairs to the double pass, and not all of them
                assert 0 < i["n_rescued"] < l.size, (flag, i)
