"""Host-made Smith-Waterman plans stay what tests/golden/sw_plan_digests.json says, record for record.

agx_sw_host::create_batch (csrc/agx_sw.cpp) is the one place every Smith-Waterman batch is planned.  Under the tuning build's
AGX_TRACE_CREATE a host-made plan prints "plan digest %016llx": FNV-1a over family, rising, wide, stage, the launches, the wave
records and the group records.  The cases of tests/sw_plan_cases.py -- one per branch of the planner -- are created plan-only
in child processes (the knobs are read once per process) and the digest, the kernel-choice lines and the agx_sw_info fields
must equal the fixture, which tools/record_sw_plan_digests.py wrote from the build BEFORE create_batch was split into stages.
A change that is meant to alter plans records the fixture again with that tool.

Not pinned here: cigar == 2 batches (the traced fill's chunk batches, whose walk records the digest also covers) are made by
agx_sw_batch_cigars on a device only -- no plan-only route reaches them, the GPU CIGAR tests are their check -- and
device-planned batches, which need a device: under the trace their records are copied back and hashed the same way ("device
plan digest"), and tests/test_sw_devplan_gpu.py holds that digest equal to the host-made plan's of the same batch."""
import json
import os

import pytest

from tests import sw_plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "sw_plan_digests.json")) as _f:
    GOLDEN = json.load(_f)

_got = {}


def _group(group):
    """Every group's child process runs once, whichever test asks first."""
    if group not in _got:
        _got[group] = pc.run_group(group)[0]
    return _got[group]


def test_fixture_names_the_cases():
    assert sorted(GOLDEN) == sorted(c[0] for c in pc.CASES)


@pytest.mark.parametrize("name,group", [(c[0], c[1]) for c in pc.CASES], ids=[c[0] for c in pc.CASES])
def test_plan_equals_the_recorded_one(name, group):
    assert _group(group)[name] == GOLDEN[name]


def test_threads_do_not_change_the_plan():
    """Stable sorts, integer reductions and per-class sums that are only compared: 1, 3 and all threads give one plan."""
    for k in ("digest", "family", "period", "staged", "info"):
        assert GOLDEN["mixed_20000_threads1"][k] == GOLDEN["mixed_20000"][k] == GOLDEN["mixed_20000_threads3"][k]


def test_the_cases_reach_their_branches():
    """What the recorded lines themselves show of the comments in sw_plan_cases.CASES."""
    fam = {n: GOLDEN[n]["family"] for n in GOLDEN}
    assert fam["short_2560"] == "family 2 rising 4" and fam["short_2561"] == "family 0 rising 0"
    assert fam["i32_coded"] == "family 3 rising 0" and fam["i32_delta_128"] == "family 0 rising 0"
    assert fam["signed_2558"] == "family 1 rising 0"
    assert [fam["rising_%d" % r] for r in (0, 1, 4)] == ["family 2 rising %d" % r for r in (0, 1, 4)]
    assert GOLDEN["period_19"]["period"] == "class period 19 of 19"
    assert fam["matrix_500"] == "family 0 rising 0" and fam["align_ends_local"] == "family 4 rising 0"
    assert all(fam["align_%s_%s" % (w, m)] == "family 5 rising 0" for w in ("ends", "spans") for m in ("global", "fit", "extend"))
    assert GOLDEN["align_ends_local_20000"]["info"]["n_launches"] == 2  # classes kept: more than one, each its own launch
    assert GOLDEN["uniform_1024"]["digest"] != GOLDEN["uniform_1023"]["digest"]
    assert GOLDEN["mixed_300"]["digest"] != GOLDEN["mixed_300_beta0"]["digest"]  # the tail term re-tiled the batch
    assert GOLDEN["empty_0_pairs"]["info"]["n_waves"] == 0 == GOLDEN["empty_sides_only"]["info"]["n_waves"]
