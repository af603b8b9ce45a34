"""PairHMM plans and packed images stay what tests/golden/phmm_plan_digests.json says, record for record and byte for byte.

create_batch (csrc/agx_phmm.cpp) and make_plan (csrc/agx_phmm_plan.cpp) are the one place every PairHMM batch is laid out and
planned.  Under the tuning build's AGX_TRACE_CREATE a create prints "plan digest main %016llx" -- FNV-1a over kind, slots, the
trains and file_order flags, the padded cells, the launches and every wave, table and group record -- "plan digest stripe" for
the striped plan (with stripe_rows, stripe_grid, stripe_mis_div), "image digest" (img_dw, the image bytes, read_dw, hap_dw) and
the batch's flags.  The cases of tests/phmm_plan_cases.py -- one per branch -- are created plan-only in child processes (the
knobs are read once per process) and all of it, with the agx_phmm_info fields, must equal the fixture, which
tools/record_phmm_plan_digests.py wrote from the build BEFORE the two functions were split into stages.  A change that is
meant to alter plans records the fixture again with that tool.

Not pinned here: forced read trains (trains == 2, AGX_PHMM_TRAINS_ON) are an option of a context, so no plan-only route
reaches them -- the GPU tests of tests/test_phmm_range_gpu.py and tests/test_phmm_gpu.py that force trains are their check.  A
packed batch's rescue plan is made on a device at the first underflow; make_plan gets exactly the arguments of an F64 batch
under AGX_PHMM_NO_LUT, which the no_lut cases pin, and tests/test_phmm_gpu.py compares the two digests on a device.

Thread counts: up to 16 383 pairs with work the plan does not depend on the host threads (corpus_x4_pk: 1, 3 and the default).
From 16 384 on the waves are filled on one piece of the pair list per thread, and a wave, or a read train, never spans a
piece's end: such a plan differs by thread count, so the large cases are recorded at a pinned count (1, some also at 3)."""
import json
import os

import pytest

from tests import phmm_plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "phmm_plan_digests.json")) as _f:
    GOLDEN = json.load(_f)

_got = {}


def _group(group):
    """Every group's child process runs once, whichever test asks first."""
    if group not in _got:
        _got[group] = pc.run_group(group)[0]
    return _got[group]


def _flags(name):
    words = GOLDEN[name]["flags"].split()
    return dict(zip(words[0::2], (int(v) for v in words[1::2])))


def test_fixture_names_the_cases():
    assert sorted(GOLDEN) == sorted(c[0] for c in pc.CASES)


@pytest.mark.parametrize("name,group", [(c[0], c[1]) for c in pc.CASES], ids=[c[0] for c in pc.CASES])
def test_plan_equals_the_recorded_one(name, group):
    assert _group(group)[name] == GOLDEN[name]


def test_threads_do_not_change_a_plan_of_one_piece():
    """Stable sorts, integer reductions and per-class sums that are only compared: 1, 3 and all threads give one plan while the
    waves are filled in one piece.  (The pinned large cases differ by thread count, as the module's docstring says.)"""
    for k in ("main", "image", "flags", "compared", "info"):
        assert GOLDEN["corpus_x4_pk_threads1"].get(k) == GOLDEN["corpus_x4_pk"].get(k) == GOLDEN["corpus_x4_pk_threads3"].get(k)
    assert GOLDEN["corpus_x_pk"]["image"] == GOLDEN["corpus_x_pk_threads3"]["image"]
    assert GOLDEN["corpus_x_pk"]["flags"] == GOLDEN["corpus_x_pk_threads3"]["flags"]


def test_the_cases_reach_their_branches():
    """What the recorded lines themselves show of the comments in phmm_plan_cases.CASES."""
    main = {n: GOLDEN[n]["main"] for n in GOLDEN}
    info = {n: GOLDEN[n]["info"] for n in GOLDEN}
    # read trains: by themselves (one shape, no comparison), compared and kept, compared and dropped, switched off, refused
    assert _flags("one_shape_pk")["trains"] == 1 and "compared" not in GOLDEN["one_shape_pk"]
    assert _flags("two_shapes_pk")["trains"] == 1 and GOLDEN["two_shapes_pk"]["compared"] == "with"
    assert _flags("corpus_x_pk")["trains"] == 0 and GOLDEN["corpus_x_pk"]["compared"] == "without"
    assert _flags("one_shape_pk_no_trains")["trains"] == 0 and main["one_shape_pk_no_trains"] != main["one_shape_pk"]
    assert _flags("wild_pk") == dict(fast=1, trains=0, lut_prior=0, lut_ring=0, file_order=1) and "compared" not in GOLDEN["wild_pk"]
    assert all("compared" not in GOLDEN[n] for n in ("corpus_pk", "jitter_pk", "corpus_x4_pk"))  # below the threshold
    # file order: one shape and every pair with work
    assert _flags("one_shape_pk")["file_order"] == 1 and _flags("whole_pk")["file_order"] == 1
    assert _flags("empty_reads_pk")["file_order"] == 0 and info["empty_reads_pk"]["n_pairs"] == 22 and info["whole_pk"]["n_pairs"] == 16
    assert info["empty_reads_pk"]["n_waves"] == info["whole_pk"]["n_waves"] == 1  # the empty reads' pairs: output slots, no work
    # the striped plan
    for n in GOLDEN:
        assert ("stripe" in GOLDEN[n]) == n.startswith("long_"), n
    assert info["long_f64"]["n_launches"] == 2 and info["long_f32"]["n_launches"] == 3 and info["long_pk"]["n_launches"] == 2
    assert GOLDEN["long_gatk_f64"]["stripe"] != GOLDEN["long_gatk_f64_short_read"]["stripe"]
    # the scans
    assert _flags("plain_f64")["lut_prior"] == 1 and _flags("not_dna_f64")["lut_prior"] == 0
    assert _flags("plain_pk")["fast"] == 1 and _flags("not_dna_pk")["fast"] == 0 and _flags("gcp0_pk")["fast"] == 0
    assert _flags("ring_no_f64")["lut_ring"] == 0 and _flags("ring_yes_f64")["lut_ring"] == 1
    assert _flags("corpus_f64")["lut_prior"] == 1 and _flags("corpus_f64_no_lut")["lut_prior"] == 0
    # the shard view: the image and the plan of the same regions on their own
    for p in ("f64", "pk"):
        assert GOLDEN["shard_view_" + p] == GOLDEN["shard_alone_" + p]
    # knobs
    assert main["jitter_pk_beta0"] != main["jitter_pk"] and info["jitter_pk_beta0"]["n_waves"] < info["jitter_pk"]["n_waves"]
    assert main["corpus_f64_beta0"] == main["corpus_f64"]
    assert main["corpus_f64_c16"] != main["corpus_f64"]
    assert info["jitter_big_f64"]["n_launches"] == 3 and info["jitter_big_f64_2_classes"]["n_launches"] == 2
    assert GOLDEN["jitter_f64_gatk"]["image"] == GOLDEN["jitter_f64"]["image"]  # the prior is no part of the image
    # empty inputs
    assert info["empty_no_regions"]["n_waves"] == 0 == info["empty_only"]["n_waves"] and info["empty_only"]["n_pairs"] == 2
    assert info["one_by_one_f64"]["n_waves"] == 1 and info["one_by_one_f64"]["cells"] == 1
    # the rescue route: the ladder's double plan is an ordinary one
    assert info["ladder_f64_no_lut"]["n_pairs"] == info["ladder_pk"]["n_pairs"] == 480
