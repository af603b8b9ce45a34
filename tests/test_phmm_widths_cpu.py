"""Which PairHMM kernel build a pair runs in, proven from plans made without a device.

tests/test_phmm_widths_gpu.py runs every width of every fill family with AGX_PHMM_FORCE_C; this file is what proves that the
width asked for is the width planned, for every shape that test runs: a batch of one (R, H) shape has
padded_cells == n_waves x steps x 64 x C (x 2 for the packed float fill), steps = R + G - 1 with G = ceil(H / C) lanes per group,
and n_waves = groups / (64 // G) rounded up -- only width C on G lanes satisfies both.  A launch whose groups all have 16 lanes
runs the 16-lane build (ROW16 / all_g16), any other the general one; every width of every family must be reached in both.

Without the knob, against the shipped library, the same shapes are planned as the planner likes: the (width, build) pairs it
reaches are recorded as a frozen set, so that a change to the planner has to look at what the suite then still covers."""
import pytest

import accelerating_genomics_amd.api as agx
from tests import phmm_widths as pw

# kPhClassCost / kPhPkClassCost of agx_phmm.h, restated; used only to tell apart tilings of equal padding (planned_width)
_PK = (1.834, 1.541, 1.454, 1.332, 1.293, 1.220, 1.195, 1.141, 1.137, 1.098, 1.093, 1.083, 1.073, 1.059, 1.063, 1.073, 1.068, 1.044, 1.034,
       1.049, 1.034, 1.024, 1.024, 1.029, 1.020, 1.005, 1.000, 1.015, 1.005)
_EVEN = {"f64": (1.569, 1.330, 1.232, 1.176, 1.144, 1.101, 1.096, 1.071, 1.058, 1.060, 1.035, 1.053, 1.005, 1.000, 1.015),
         "f64fma": (1.801, 1.457, 1.331, 1.258, 1.185, 1.136, 1.089, 1.099, 1.073, 1.086, 1.050, 1.066, 1.007, 1.017, 1.000),
         "f32": (1.872, 1.500, 1.346, 1.248, 1.184, 1.158, 1.132, 1.109, 1.090, 1.075, 1.090, 1.068, 1.045, 1.023, 1.011, 1.000, 1.071, 1.056, 1.045)}
COST = dict({f: dict(zip(range(4, 41, 2), row)) for f, row in _EVEN.items()}, pk=dict(zip(range(4, 33), _PK)))
TAB_BUDGET = 20 * 1024  # LDS bytes a wave may spend on several read tables (agx_phmm.cpp)


@pytest.mark.parametrize("C", pw.WIDTHS)
def test_pinned_width_is_the_planned_width(C):
    got = pw.run_child("plan", C)
    fams = pw.families(C)
    assert fams and {s[0] for s in got["shapes"]} == set(fams)
    reached = set()
    for fam, G, R, H, i in got["shapes"]:
        slots = pw.FAMILIES[fam][2]
        assert G == -(-H // C) and (R, H) in pw.shapes(C, G)
        waves = pw.one_shape_waves(fam, G)
        assert i["n_waves"] == waves and i["padded"] == waves * pw.steps(R, G) * 64 * C * slots, (fam, G, R, H, i)
        assert i["cells"] == 9 * R * H and i["n_launches"] == (2 if fam == "f32" else 1), (fam, G, R, H, i)  # (f32: fill + double pass)
        reached.add((fam, "g16" if G == 16 else "general"))
    assert reached == {(fam, build) for fam in fams for build in ("g16", "general")}  # no exceptions
    # the batches the GPU test runs, and their twins with one N in a haplotype: one class, whole waves of width C
    for fam, where, i, t in got["batches"]:
        unit = 64 * C * pw.FAMILIES[fam][2]
        for p in (i, t) if t else (i,):
            assert p["padded"] % unit == 0 and p["padded"] >= unit * p["n_waves"] and p["n_launches"] == (2 if fam == "f32" else 1), (fam, where, p)
        assert not t or t["cells"] == i["cells"]
    assert {(f, w) for f, w, _, _ in got["batches"]} >= {(f, "G%d" % G) for f in fams for G in pw.GS}
    # where a plan shows which kernel it is for.  Double modes: the looked-up-prior fill's table rows have 56 bytes, the
    # selecting fill's 33 (rows = steps + G - 1 = 32), and a wave holds as many tables as fit 20 KB
    lut_tab, sel_tab = 56 * (30 + 2), (33 * 32 + 15) & ~15
    for fam, i, t in got["tables"]:
        assert i["n_waves"] == -(-40 // (TAB_BUDGET // lut_tab)) == 4 and t["n_waves"] == -(-40 // (TAB_BUDGET // sel_tab)) == 3, (fam, i, t)
    assert [f for f, _, _ in got["tables"]] == [f for f in fams if f in ("f64", "f64fma")]
    # packed float fill: 65 536 pairs of 10 x 16 C form read trains by themselves -- two reads of 10 rows take
    # 2 (R + 1) + G - 2 = 36 steps -- except at widths 31 and 32, which do not pair unless told to, and in the twin: the plain cell
    if "pk" in fams:
        i, t = got["trains"]
        if C <= 30:
            assert i["n_waves"] == 4096 and i["padded"] == 4096 * pw.steps(10, 16, 10) * 64 * C * 2 and pw.steps(10, 16, 10) == 36
        else:
            assert i["n_waves"] == 8192 and i["padded"] == 8192 * pw.steps(10, 16) * 64 * C * 2
        assert t["n_waves"] == 8192 and t["padded"] == 8192 * pw.steps(10, 16) * 64 * C * 2
    else:
        assert got["trains"] is None


def planned_width(fam, R, H, plans):
    """The (width, lanes per group) of one-shape plans of one read x n haplotypes, plans = {n: info}: the only class of the family
    that satisfies the identity for every n (three pairs alone can be 2 lanes of 4 columns or 1 of 6: the same padded cells; 130
    fill a different number of waves).  One read: one table per wave, so 64 // G groups always fit.  Batches this small are all
    tiled by the same rule, whatever their count."""
    _, widths, slots = pw.FAMILIES[fam]
    fits = []
    for C in widths:
        G = -(-H // C)
        if G <= 64 and all(i["n_waves"] == pw.one_shape_waves(fam, G, 1, 1, n) and i["padded"] == i["n_waves"] * pw.steps(R, G) * 64 * C * slots
                           for n, i in plans.items()):
            fits.append((C, G))
    assert fits, (fam, R, H, plans)
    # tilings that pad to the same cells and fill the same waves (16 lanes x 28 columns, 14 x 32 at H = 442) cannot be told apart
    # from a plan: among those the planner takes the lowest lane time per slot, 64 / (64 // G) x the class's measured cost
    fits.sort(key=lambda f: (64 / (64 // f[1]) * COST[fam][f[0]], f[0]))
    return fits[0]


def natural_choices():
    """{family: {build: widths}} the shipped planner reaches on the shapes of every width's table."""
    assert agx.LIB_PATH.endswith("libagx.so"), agx.LIB_PATH
    out = {fam: {"g16": set(), "general": set()} for fam in pw.FAMILIES}
    seen = set()
    for C in range(4, 33):
        for G in pw.GS:
            for R, H in pw.shapes(C, G):
                if (R, H) in seen:
                    continue
                seen.add((R, H))
                for fam, (prec, _, _) in pw.FAMILIES.items():
                    # (one lane of H columns: the lengths only)
                    W, lanes = planned_width(fam, R, H, {n: pw.plan(pw.uniform_batch(H, 1, R, 1, 1, n), prec) for n in (3, 130)})
                    out[fam]["g16" if lanes == 16 else "general"].add(W)
    return out


# (width, build) pairs that the shipped planner chooses by itself on these shapes; everything else is reached only through the knob
NATURAL = {
    "f64": {"g16": [20, 24, 26, 28, 30, 32], "general": list(range(4, 33, 2))},
    "f64fma": {"g16": [20, 24, 26, 28, 30, 32], "general": list(range(4, 33, 2))},
    "f32": {"g16": [20, 26, 28, 30, 32, 34, 36, 40], "general": list(range(4, 41, 2))},
    "pk": {"g16": [20, 22, 24, 25, 26, 27, 28, 29, 30, 31, 32], "general": list(range(4, 33))},
}


def test_the_shipped_planners_own_choices_are_the_recorded_ones():
    got = natural_choices()
    assert {f: {b: sorted(w) for b, w in v.items()} for f, v in got.items()} == NATURAL
