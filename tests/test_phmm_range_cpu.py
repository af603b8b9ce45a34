"""What tests/test_phmm_range_gpu.py relies on, proven without a device from the oracle and from plans (tests/phmm_range_cases.py).

* The clean profiles are clean: no row with Qi + Qd > 1, every fp64 sum finite and not negative.  A sum is exactly 0 (log10 L =
  -inf, the pattern the kernels must reproduce) only where a base quality of Phred 0 gives a matching base the prior 0, or where
  the ring read's 316 insertions underflow the double range.
* The 1e-6 bar of the float modes is one the reference's own arithmetic has room under: the oracle's plain-float restatement
  (variant 2) stays within 5e-7 relative on log10 L on every kept pair (float sum >= AGX_PHMM_F32_RESCUE) of the clean cases.
  Worst found: 3.4e-7 (base0, C4 G16); per profile del93 1.9e-7, del80-93 gcp1 1.2e-7, ins93 1.5e-7, gcp1 1.1e-7, gcp1-3 9.1e-8,
  gcp93 2.8e-7, base0 3.4e-7, base0-2 2.2e-7, base93 5.8e-8, gaps3-4 8.6e-8, all4-93 8.3e-8.
* The ladders straddle what they are built for: at least 4 pairs within half a decade on either side of the rescue threshold,
  |log10 L| on both sides of the accuracy guard's bound.
* A runaway read does run away: with both gap qualities at Phred 0 the float restatement's sum is not finite, so a read train
  that handed this state on would show.
* The host keeps read trains out of a batch exactly when some row has Qi + Qd > 1 (plans of config 3's size, where trains form
  by themselves), and the striped and ring cases reach those launches."""
import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
from tests import oracle_api
from tests import phmm_range_cases as rc
from tests import phmm_widths as pw


def test_profiles_are_on_their_side_of_the_boundary():
    assert all(rc.is_clean(p) for p in rc.CLEAN.values()) and rc.is_clean(rc.USUAL)
    assert not any(rc.is_clean(p) for p in rc.RUNAWAY.values())
    assert rc.LUT[3] + rc.LUT[3] > 1 >= rc.LUT[3] + rc.LUT[4]
    assert abs(rc.RESCUE_LOG10 + 65.33) < 0.005


@pytest.mark.parametrize("name", list(rc.CLEAN))
def test_clean_profiles_are_finite_and_float_has_room_under_1e6(oracle, name):
    worst = 0.0
    for where, b, _ in rc.clean_batches(name):
        assert not rc.runaway_rows(b).any(), where
        for bb in (b, pw.twin(b)[0]):
            for variant in (0, 3):
                s, l = oracle.phmm_batch(bb, variant)
                assert np.all(np.isfinite(s)) and np.all(s >= 0), (where, variant)
                if where != "ring" and not name.startswith("base0"):
                    assert np.all(np.isfinite(l)), (where, variant)
                else:
                    assert np.array_equal(np.isfinite(l), s > 0), (where, variant)
        s, l = oracle.phmm_batch(b, 0)
        s32, l32 = oracle.phmm_batch(b, 2)
        keep = (s32 >= rc.RESCUE) & np.isfinite(l) & (l != 0)
        assert where == "ring" or keep.sum() >= keep.size // 2, where
        worst = max(worst, float(np.max(np.abs(l32[keep] - l[keep]) / np.abs(l[keep]), initial=0.0)))
    print("float restatement, %s: worst %.3g relative on log10 L" % (name, worst))
    assert worst <= 5e-7


def _near(l):
    d = l - rc.RESCUE_LOG10
    return int(np.sum((d < 0) & (d > -0.5))), int(np.sum((d >= 0) & (d < 0.5)))


@pytest.mark.parametrize("name", rc.LADDER_PROFILES)
def test_rescue_ladders_straddle_the_threshold(oracle, name):
    for what, b in rc.ladders(name):
        _, l = oracle.phmm_batch(b, 0)
        assert np.all(np.isfinite(l))
        below, above = _near(l)
        lo, hi = rc.rescued_range(l)
        if name == "del80-93 gcp1" and what == "mismatches":
            # a gap-continuation quality of Phred 1: inserting the whole read costs Qi Qg^99, about 1e-14, and no number of
            # mismatches takes the pair below that -- this profile crosses the threshold on its insertion ladder
            assert l.min() > -16 and (lo, hi) == (0, 0)
            continue
        assert below >= 4 and above >= 4, (what, below, above)
        assert 0 < lo <= hi < l.size, (what, lo, hi)
    assert len(rc.ladders("del80-93 gcp1")) == 2


def test_guard_ladder_straddles_the_guard(oracle):
    b, Rs = rc.guard_ladder()
    for flag, variant in ((0, 0), (agx.PHMM_GATK_PRIOR, 3)):
        _, l = oracle.phmm_batch(b, variant)
        assert np.all(np.isfinite(l))
        inside = np.abs(l) < rc.GUARD_K[flag] * np.sqrt(Rs + 8)
        assert inside.sum() >= 20 and (~inside).sum() >= 20, flag
        for R in (1, 2):  # (from four bases on, without the prior, every pair is outside: one base costs more than the bound grows)
            assert inside[Rs == R].any() and not inside[Rs == R].all(), (flag, R)
        assert not inside[Rs == 30].any()


@pytest.mark.parametrize("name", list(rc.RUNAWAY))
def test_runaway_reads_run_away(oracle, name):
    blown = {}
    for R in rc.TRAIN_READS:
        b, clean = rc.train_batch(name, R)
        rows = rc.runaway_rows(b)
        first = np.zeros(rows.size, bool)
        for g in range(b.n_regions):
            r = int(b.rreg[g])
            first[int(b.roff[r]):int(b.roff[r + 1])] = True
        assert rows.any() and not rows[~first].any()  # the first read of a region, and only that one
        assert clean.sum() == rc.N_TRAIN_REGIONS * (rc.N_TRAIN_READS - 1) * rc.N_TRAIN_HAPS
        _, l = oracle_api.phmm_batch_mt(oracle, b, 0)
        assert np.all(np.isfinite(l[clean]))
        s32, _ = oracle_api.phmm_batch_mt(oracle, b, 2)
        assert np.all(np.isfinite(s32[clean]))
        blown[R] = int(np.sum(~np.isfinite(s32[~clean])))
    print("runaway reads with a float sum that is not finite, %s: %s" % (name, blown))
    if name == "gaps0":  # the profile that proves the train case: inf - inf in the float state, at every length
        assert all(n > 0 for n in blown.values()), blown
    # the short shapes: negative sums (log10 NaN) in the reference itself (all1-93: one row in a thousand, few of these batches have one)
    short = [rc.shape_batch(name, C, G) for C in rc.WIDTHS for G in rc.LANES]
    assert all(rc.runaway_rows(b).any() for b in short) or name == "all1-93"
    assert any(np.isnan(oracle.phmm_batch(b, 0)[1]).any() for b in short)


# (q_ins, q_del) of ONE row of a config-3-sized batch -> whether read trains still form by themselves
BOUNDARY = [((3, 4), True), ((4, 3), True), ((3, 3), False), ((2, 5), True), ((2, 4), False), ((1, 7), True), ((1, 6), False),
            ((0, 93), False), ((93, 0), False), ((0, 0), False)]


@pytest.mark.parametrize("rows,trains", BOUNDARY, ids=lambda v: str(v))
def test_one_runaway_row_keeps_read_trains_out(rows, trains):
    """64 x 64 x 16 pairs of 100 x 300 pair their reads by themselves: 4096 waves of two reads, 8192 without trains."""
    assert (rc.LUT[rows[0]] + rc.LUT[rows[1]] <= 1) == trains
    assert pw.plan(rc.auto_train_batch(rows=rows), agx.PHMM_F32_FMA)["n_waves"] == (4096 if trains else 8192)


@pytest.mark.parametrize("name", ["usual", "gaps3-4", "del80-93 gcp1", "all4-93"] + list(rc.RUNAWAY))
def test_profiles_and_read_trains(name):
    waves = pw.plan(rc.auto_train_batch(name), agx.PHMM_F32_FMA)["n_waves"]
    assert waves == (8192 if name in rc.RUNAWAY else 4096)


def test_striped_and_ring_cases_reach_those_launches():
    b = rc.stripe_batch("usual")
    R = int(b.roff[1])
    striped = lambda hs: sum(-(-H // (64 * 24)) * (R + 63) * 64 * 24 for H in hs)  # stripes of 64 lanes x 24 columns, R + 63 steps
    for fam in ("f64", "f64fma", "pk"):
        i = pw.plan(b, pw.FAMILIES[fam][0])
        assert (i["n_waves"], i["n_launches"], i["padded"]) == (2, 1, striped(rc.STRIPE_HAPS)), (fam, i)
    i = pw.plan(b, agx.PHMM_F32)  # 2100 columns in one pass, 2600 striped, and the double pass
    assert i["n_launches"] == 3 and i["padded"] < striped(rc.STRIPE_HAPS) and i["padded"] > striped(rc.STRIPE_HAPS[1:]), i
    # the ring: a table of R + 2 rows beyond the longest whole table (AGX_PH_LUT_FULL_ROWS = 365), plain DNA
    ring = rc.ring_batch("usual")
    assert int(ring.roff[1]) == rc.RING_SHAPE[0] == pw.RING_READS[0] == pw.WHOLE_READ + 1
    assert set(bytes(ring.read_bases)) <= set(b"ACGTN") and set(bytes(ring.hap_bases)) <= set(b"ACGT")
