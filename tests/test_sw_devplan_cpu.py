"""The cases of tests/sw_devplan_cases.py are what tests/test_sw_devplan_gpu.py assumes of them, checked without a device.

The GPU test compares a device-made plan with the host-made plan of the same batch.  That says something only where the device
planner takes the batch: the packed biased fill (family 2), one launch, enough waves for the verdict on 256 CUs (estimated waves
>= 0.48 x 20 x 256 = 2458), not uniform, no dominant shape, and none of the host's rules that tile again.  A plan-only create is
tiled for 256 CUs by the host planner; it is made twice per case, as the library ships and under AGX_SW_TAIL_BETA=0 (no tail
term).  Equal digests say the tail term did not fire, so the plan is the one the full tiling table gives -- the device
planner's -- and the wave count of the beta-0 run is then the verdict's: at least 2816 waves is fill >= 0.55."""
import re

import numpy as np
import pytest

from tests import sw_devplan_cases as dc

NAMES = list(dc.CASES)
_got = {}


def _plans(name):
    """(as shipped, under AGX_SW_TAIL_BETA=0) of the named case: one child process each, once per module."""
    if name not in _got:
        _got[name] = (dc.run("plan", [name])[0][name], dc.run("plan", [name], extra_env={"AGX_SW_TAIL_BETA": "0"})[0][name])
    return _got[name]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_one_the_device_planner_takes(name):
    default, beta0 = _plans(name)
    print(name, default, beta0)
    want_family = "family 2 rising 0" if name == "tail_65535" else "family 2 rising 4"
    assert default["family"] == want_family and beta0["family"] == want_family
    assert default["digest"] == beta0["digest"], "the tail term re-tiled the batch"
    assert default["parts"] == beta0["parts"] and default["info"] == beta0["info"]
    assert beta0["info"]["n_waves"] >= 2816
    assert default["info"]["n_launches"] == 1 and default["info"]["planned_on_device"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_case_is_neither_uniform_nor_dominated_by_a_shape(name):
    la, lb, _ = dc.lens(name)
    shapes, counts = np.unique(np.minimum(la, lb).astype(np.uint64) << 16 | np.maximum(la, lb), return_counts=True)
    assert shapes.size > 1
    assert counts.max() * 2 < la.size, (shapes[counts.argmax()], counts.max())


@pytest.mark.parametrize("name", NAMES)
def test_case_lengths_are_deterministic_and_as_described(name):
    assert dc.lens_sha256(name) == dc.lens_sha256(name)
    la, lb, special = dc.lens(name)
    n = la.size
    sub = dc.subset(name)
    assert len(sub) <= 64 and set(special) <= set(sub) and all(0 <= p < n for p in sub)
    assert int(np.minimum(la, lb).max()) <= 2560 and int(np.maximum(la, lb).max()) <= 65535
    empty = np.nonzero((la == 0) | (lb == 0))[0]
    if name == "mixed":
        assert list(empty) == [0, 20000, 40001, n - 1] and n == 64001
        a, b = dc.TIE_SHAPE
        fwd, rev = np.nonzero((la == a) & (lb == b))[0], np.nonzero((la == b) & (lb == a))[0]
        assert fwd.size >= 200 and rev.size >= 200 and (fwd.size + rev.size) * 100 < n  # several hundred ties, under 1 %
        assert fwd.max() - fwd.min() > n // 2 and rev.max() - rev.min() > n // 2       # scattered through the file
    else:
        assert empty.size == 0
    if name == "one_class":
        assert n == 96000 and np.all(la == 150) and lb.min() == 150 and lb.max() == 399
    if name == "long":
        assert n == 6000 and (la[77], lb[77]) == (2560, 2700) and (la[78], lb[78]) == (2700, 2560)
        assert la.min() >= 1200 and lb.min() >= 1200
    if name == "tail_65535":
        assert n == 60000 and (la[30000], lb[30000]) == (65535, 40) and (la[n - 1], lb[n - 1]) == (1, 1)
        assert np.count_nonzero(np.maximum(la, lb) > 600) == 1
    if name == "stride":
        assert n == 1100000 and n > 16 * 256 * 256 and la.min() == 8 and la.max() == 48


def test_one_class_batch_is_one_launch_of_that_class():
    """The plan parts line names the columns per lane of every launch: one launch, and not the any-class kernel's 0."""
    m = re.search(r"; launch C((?: \d+)+)$", _plans("one_class")[0]["parts"])
    assert m and len(m.group(1).split()) == 1 and int(m.group(1)) != 0, _plans("one_class")[0]["parts"]


def test_digest_sees_the_dispatch_order_and_the_parts_line_says_where():
    """The same records in another wave order are another plan: under AGX_SW_SORT_WAVES=0 (tuning build) the host leaves the
    waves of `mixed` in bucket order.  Nothing an agx_sw_info field counts changes, the digest does, and of the three parts
    only the wave records'."""
    sorted_, _ = _plans("mixed")
    unsorted = dc.run("plan", ["mixed"], extra_env={"AGX_SW_SORT_WAVES": "0"})[0]["mixed"]
    assert unsorted["info"] == sorted_["info"] and unsorted["family"] == sorted_["family"]
    assert unsorted["digest"] != sorted_["digest"]
    part = {k: [re.search(k + r" ([0-9a-f]{16})", e["parts"]).group(1) for e in (sorted_, unsorted)] for k in ("head", "waves", "groups")}
    assert part["head"][0] == part["head"][1] and part["groups"][0] == part["groups"][1] and part["waves"][0] != part["waves"][1], part


def test_mixed_batch_has_vacant_halves():
    m = re.search(r"; (\d+) groups, (\d+) vacant halves; launch C 0$", _plans("mixed")[0]["parts"])
    assert m and int(m.group(2)) > 0, _plans("mixed")[0]["parts"]
