"""Banded plans and their images stay what tests/golden/sw_band_plan_digests.json says, record for record and byte for byte.

agx_sw_host::create_band (csrc/agx_sw_band.cpp over the stages of csrc/agx_sw_band_plan.cpp) plans every banded batch: plain,
around a diagonal, z-drop and matrix, each with and without CIGARs.  Under the tuning build's AGX_TRACE_CREATE it prints the kind
of batch, "plan digest %016llx" (FNV-1a over the kind, the kernel constants, the launches, every wave and group record, the first
rows, the diagonals and a cigar batch's tables), what the plan is made of, and "image digest %016llx" over the bytes the fills
read.  The cases of tests/sw_band_plan_cases.py -- one per branch of the planner -- are created plan-only in child processes and
every line and the agx_sw_info fields must equal the fixture, which tools/record_sw_band_plan_digests.py wrote from the build
BEFORE create_band was split into stages (the one function it was, with only the trace lines added).  A change that is meant to
alter banded plans records the fixture again with that tool.  tests/test_sw_band_gpu.py holds three of the cases, created on a
device, to the same fixture: what is uploaded is what is hashed here."""
import json
import os

import pytest

from tests import sw_band_plan_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "sw_band_plan_digests.json")) as _f:
    GOLDEN = json.load(_f)

_got = {}


def _group(group):
    """Every group's child process runs once, whichever test asks first."""
    if group not in _got:
        _got[group] = bc.run_group(group)[0]
    return _got[group]


def _fpad(name):
    return [int(v) for v in GOLDEN[name]["fpad"].split("/")]


def test_fixture_names_the_cases():
    assert sorted(GOLDEN) == sorted(c[0] for c in bc.CASES)


@pytest.mark.parametrize("name,group", [(c[0], c[1]) for c in bc.CASES], ids=[c[0] for c in bc.CASES])
def test_plan_and_image_equal_the_recorded_ones(name, group):
    assert _group(group)[name] == GOLDEN[name]


def test_threads_do_not_change_the_plan_or_the_image():
    """The plan is made by one thread; the image by all of them, a range of groups each, into disjoint bytes."""
    assert GOLDEN["global_w12_5000_threads1"] == GOLDEN["global_w12_5000"] == GOLDEN["global_w12_5000_threads3"]


def test_the_cases_reach_their_branches():
    """What the recorded lines themselves show of the names in sw_band_plan_cases.CASES."""
    kind = {n: GOLDEN[n]["kind"] for n in GOLDEN}
    assert all(_fpad("global_w8")) and len(GOLDEN["global_w8"]["launch_k"].split()) > 1  # every fpad, several K
    assert GOLDEN["extend_w0_one_diagonal"]["launch_k"] == "4" and GOLDEN["extend_w0_one_diagonal"]["info"]["n_waves"] == (300 + 63) // 64  # G = 1
    wide = GOLDEN["global_2048_diagonals"]
    assert wide["launch_k"] == "32" and sum(_fpad("global_2048_diagonals")) == 1 == wide["info"]["n_waves"]  # one group, its own wave
    assert wide["info"]["padded_cells"] == (2999 + 64) * 64 * 32  # G = 64: lb + G steps of 64 lanes of 32 diagonals
    for name in ("empty_0_pairs", "empty_sides_only"):
        assert GOLDEN[name]["info"]["n_waves"] == 0 and GOLDEN[name]["launch_k"] == "none"
    assert sum(_fpad("empty_side_and_1x1")) == 1
    for what, wname in ((1, "ends"), (2, "spans")):
        for mode, mname in ((1, "global"), (3, "extend"), (4, "extend_query")):
            assert kind["diag_%s_%s" % (mname, wname)] == "mode %d band 16 align %d at 1 zdrop -1 cigar 0 matrix 0" % (mode, what)
        assert int(GOLDEN["diag_fit_windows_" + wname]["trimmed_rows"]) > 0  # row0 > 0, rows behind the band
        spread = GOLDEN["diag_local_spread_" + wname]
        assert 0 < sum(_fpad("diag_local_spread_" + wname)) < spread["info"]["n_pairs"]  # some bands miss the matrix: no group
        assert int(spread["trimmed_rows"]) > 0
    assert kind["zdrop_diag_none"] == kind["zdrop_diags"] == "mode 3 band 16 align 2 at 1 zdrop 50 cigar 0 matrix 0"
    assert GOLDEN["zdrop_diag_none"]["digest"] != GOLDEN["zdrop_diags"]["digest"]
    for mname in ("local", "fit"):  # the same bytes, the same layout: codes + 1 under the matrix
        with_m, without = GOLDEN["matrix_" + mname], GOLDEN["protein_%s_no_matrix" % mname]
        assert with_m["kind"].endswith("matrix 1") and without["kind"].endswith("matrix 0")
        assert with_m["info"] == without["info"] and with_m["fpad"] == without["fpad"] and with_m["image"] != without["image"]
    # a cigar batch: the same records and image as the batch without, another digest (the flag and the tables)
    for cig, plain in (("cigar_global_w8", "global_w8"), ("cigar_diag_fit_windows", "diag_fit_windows_spans"),
                       ("cigar_matrix_local", "matrix_local"), ("cigar_zdrop", "zdrop_diags")):
        assert kind[cig] == kind[plain].replace("cigar 0", "cigar 1")
        assert GOLDEN[cig]["image"] == GOLDEN[plain]["image"] and GOLDEN[cig]["digest"] != GOLDEN[plain]["digest"]
