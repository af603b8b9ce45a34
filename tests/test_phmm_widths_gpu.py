"""Every width of every PairHMM fill family, in its 16-lane build and its general one, on plain DNA against the fp64 oracle.

One child process per width with AGX_PHMM_FORCE_C (tests/phmm_widths.py; tests/test_phmm_widths_cpu.py proves that the width
asked for is the width planned).  Per width: pairs on 1, 2, 3, 16, 17 and 64 lanes, the last lane full or holding one column, reads
shorter than the skew; the looked-up-prior double fill with whole and ring tables; the packed float fill's fast cell without and with
read trains; and each batch's twin with one N in a haplotype, which runs the selecting fill and the plain packed cell instead.
Bars: AGX_PHMM_F64 bit for bit, AGX_PHMM_F64_FMA 1e-12 relative on log10 L, the float modes 1e-6 relative on log10 L or
1e-6 / ln 10 absolute where log10 L is near 0, the finite / -inf pattern the oracle's."""
import pytest

import accelerating_genomics_amd.api as agx
from tests import phmm_widths as pw

pytestmark = pytest.mark.gpu

_DIED = []  # a child that ended by a signal, at its time limit or without a result: nothing more is started on the GPU


def check(C, recs):
    fams = pw.families(C)
    by = {(r["where"], r["leg"]): r for r in recs}
    for r in recs:
        assert pw.meets(r["prec"], r), (C, r)
        assert r.get("plan_same", True), (C, r)  # the plan made without a device is the one that ran
        assert r["padded"] % (64 * C * (2 if r["prec"] & 0xff == agx.PHMM_F32_FMA else 1)) == 0, (C, r)
        assert r.get("same_bits_as_plain_dna", True) and r.get("same_bits_as_off", True) and r.get("all_finite", True), (C, r)
    for G in pw.GS:
        w = "G%d" % G
        for fam in fams:
            tags = [fam] + ([fam + "+gatk"] if G in pw.GATK_GS and fam in ("f64", "pk") else [])
            for tag in tags:
                if fam != "pk":
                    assert (w, tag) in by and (w, tag + " twin") in by, (C, w, tag)
                    if fam == "f64":
                        assert "same_bits_as_plain_dna" in by[(w, tag + " twin")]
                    continue
                on, t_on = by[(w, tag + " trains on")], by[(w, tag + " twin trains on")]
                assert "same_bits_as_off" in on
                # forced trains pair the reads of a region wherever they share their groups: never more waves, and fewer where a
                # wave holds at most four groups (three reads x two groups: six groups without, four with)
                assert on["n_waves"] <= on["waves_off"], (C, on)
                if G >= 16:
                    assert on["n_waves"] < on["waves_off"], (C, on)
                assert t_on["n_waves"] == t_on["waves_off"], (C, t_on)  # the plain cell has no trains
                if G == 16:
                    assert on["n_rescued"] >= 3, (C, on)  # the unrelated read, against its three haplotypes
    dbl = [f for f in fams if f in ("f64", "f64fma")]
    assert {(r["where"], r["leg"]) for r in recs if " " in r["where"]} == {("G%d %s" % (G, n), f) for G in pw.RING_GS for n in ("whole", "ring") for f in dbl}


@pytest.mark.parametrize("C", pw.WIDTHS)
def test_width(C):
    if _DIED:
        pytest.skip("the child of width %d died: no more GPU work" % _DIED[0])
    try:
        recs = pw.run_child("gpu", C)
    except pw.ChildDied as e:
        _DIED.append(C)
        pytest.fail(str(e))
    check(C, recs)


@pytest.mark.parametrize("fam", list(pw.FAMILIES))
def test_shipped_planner_on_the_same_shapes(fam, oracle):
    """Without the knob, in this process (libagx.so): the lengths that widths 4, 19 and 32 make -- the narrowest class, config 3's,
    config 5's -- tiled as the planner likes (tests/test_phmm_widths_cpu.py records which builds that reaches)."""
    if _DIED:
        pytest.skip("the child of width %d died: no more GPU work" % _DIED[0])
    assert agx.LIB_PATH.endswith("libagx.so"), agx.LIB_PATH
    recs = []
    with agx.Context(0) as ctx:
        for C in (4, 19, 32):
            for G in pw.GS:
                pw.legs(ctx, oracle, pw.width_batch(C, G), [fam], G in pw.GATK_GS, "C%d G%d" % (C, G), recs)
    assert len(recs) >= 3 * len(pw.GS) * 2
    for r in recs:
        assert pw.meets(r["prec"], r), r
        assert r.get("plan_same", True) and r.get("same_bits_as_plain_dna", True) and r.get("same_bits_as_off", True), r
