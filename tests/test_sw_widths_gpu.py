"""Every columns-per-lane class of every column-owning Smith-Waterman fill, on 1, 2, 3, 16, 17, 33 and 64 lanes a pair, against the
oracle and the by-definition checkers.  Everything is integers: the bar is equality.

One child process per class with AGX_SW_FORCE_C (tests/sw_widths.py; tests/test_sw_widths_cpu.py proves that the width asked for is
the width planned and that the table of built classes is the library's).  Per class and G: the packed biased fill at period four
and at its wide period, rising 1, rising 0, the general cell in every wave and in the wave of one N; the packed signed fill; the
int32 fills with the coded match (and one N), with the byte compare (also the classes 80, 120, 160) and with the matrix lookup; the locating
and the anchored fill in five modes, ENDS and SPANS, plain, under a four-symbol matrix and under BLOSUM62; the same with statistics
(4 .. 28) and with the traced fill and the walk (4 .. 32).  Every batch is launched and fetched twice.  Scores against the oracle
(sw_batch, sw_batch_matrix); hits, statistics, CIGARs and operation offsets against sw_fuzz_cases.reference through differ; every
CIGAR through path_check.  From the child's own AGX_TRACE_CREATE lines: every create of a leg -- the begin pass and the traced
fill of the spans included, which only exist on the device -- ran the family and the class asked for.

test_shipped_planner_on_the_same_shapes: the same batches of classes 4, 22 and 38 in this process on libagx.so, tiled as the planner
likes; the fills that only a knob of the tuning build reaches are not in it."""
import collections

import pytest

import accelerating_genomics_amd.api as agx
from tests import sw_fuzz_cases as fc
from tests import sw_widths as sw

pytestmark = pytest.mark.gpu

_DIED = []  # a child that ended by a signal, at its time limit or without a result: nothing more is started on the GPU


def creates(f):
    """-> (the leg's own create, the creates a fetch may add): the begin pass of a LOCAL or FIT batch that answers spans is the
    same fill over the reversed prefixes (FIT: in EXTEND_QUERY, the anchored fill), a cigar batch's traced fill the anchored one"""
    own = [f.family, f.rising]
    later = []
    if f.kind != "score" and f.what == fc.SPANS and f.mode in (fc.LOCAL, fc.FIT):
        later.append([f.family, 0])
    if f.kind == "cigar":
        later.append([5, 0])
    return own, later


def check(C, recs):
    by = {(r["leg"], int(r["where"][1:])): r for r in recs}
    assert len(by) == len(recs) and set(by) == set(sw.legs(C)), (C, set(by) ^ set(sw.legs(C)))  # no leg silently left out
    for (name, G), r in by.items():
        f = sw.FAMILIES[name]
        what = {k: v for k, v in r.items() if k != "scores"}
        assert r["differs"] is None, (C, what)
        assert r["relaunch_differs"] is None, (C, what)
        own, later = creates(f)
        assert r["families"][0] == own and all(x in later for x in r["families"][1:]), (C, what)
        assert all(x in r["families"][1:] for x in later), (C, what)  # ... and each of them did run
        assert r["classes"] == [C], (C, what)  # every `launch C` line of the leg, those of the batches for its spans included
        assert r["n_waves"] == sw.waves(f, r["n_pairs"], G) and r["n_launches"] == 1 and r["padded_cells"] % (64 * C) == 0, (C, what)
        if f.family in (1, 2, 3):  # a packed plan: the odd pair leaves the last group a vacant half
            assert r["n_pairs"] % 2 == 1 and r["groups"][0] == [(r["n_pairs"] + 1) // 2, 1], (C, what)
        if f.family == 2 and f.rising == 4:
            wide = C // 2 if C >= 14 else 4
            assert r["period"] == [[4 if name == "pk2 period 4" else wide, wide]], (C, what)
    # the score-only legs of different kernels on the same batch: implied by the oracle, but this names the odd one out
    for G in sw.gs(C):
        same = [(name, tuple(by[(name, G)]["scores"])) for name in sw.families(C)
                if sw.FAMILIES[name].kind == "score" and sw.FAMILIES[name].scorer == "plain" and not sw.FAMILIES[name].twin]
        if same:
            most = collections.Counter(s for _, s in same).most_common(1)[0][0]
            assert [name for name, s in same if s != most] == [], (C, G)
            assert len(same) == (1 if C in sw.WIDE_CLASSES else 7 + (C >= 14))


@pytest.mark.parametrize("C", sw.WIDTHS)
def test_width(C):
    if _DIED:
        pytest.skip("the child of width %d died: no more GPU work" % _DIED[0])
    try:
        recs = sw.run_child("gpu", C)
    except sw.ChildDied as e:
        _DIED.append(C)
        pytest.fail(str(e))
    check(C, recs)


@pytest.fixture(scope="module")
def ctxs(oracle):
    sw.load_checkers()
    with agx.Context(0) as ctx, agx.Context(0) as own:
        yield ctx, own  # own: the context whose kernel option is changed


@pytest.mark.parametrize("C", [4, 22, 38])
def test_shipped_planner_on_the_same_shapes(ctxs, oracle, C):
    """Without a knob, in this process (libagx.so): the batches of the narrowest class, of one that no other batch of the suite
    reaches and of a wide one, for every family that needs no knob and every G, through the planner's own tiling."""
    if _DIED:
        pytest.skip("the child of width %d died: no more GPU work" % _DIED[0])
    assert agx.LIB_PATH.endswith("libagx.so"), agx.LIB_PATH
    done, want = 0, sum(1 for G in sw.GS for f in sw.FAMILIES.values() if not f.env and sw.shapes(f.kind, C, G))
    for G in sw.GS:
        for name, f in sw.FAMILIES.items():
            if not f.env and sw.shapes(f.kind, C, G):
                r = sw.run_leg(ctxs[0], ctxs[1], oracle, name, C, G)
                assert r["differs"] is None and r["relaunch_differs"] is None, (C, {k: v for k, v in r.items() if k != "scores"})
                done += 1
    # every G: seven score-only fills, thirty align fills, and the stats and cigar fills whose shapes are within their limits
    assert done == want == 7 * (7 + 60) - (30 if C == 38 else 0)


@pytest.mark.parametrize("name", list(sw.REGRESSIONS))
def test_named_regression_case(ctxs, oracle, name):
    """the shapes that found something (sw_widths.REGRESSIONS says what), on the shipped library"""
    if _DIED:
        pytest.skip("the child of width %d died: no more GPU work" % _DIED[0])
    fill, C, G = sw.REGRESSIONS[name]
    r = sw.run_leg(ctxs[0], ctxs[1], oracle, fill, C, G)
    assert r["differs"] is None and r["relaunch_differs"] is None, r
