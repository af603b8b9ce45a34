"""The device planner (csrc/agx_sw_plan_kernel.hip) writes the records the host planner writes, byte for byte.

Every case of tests/sw_devplan_cases.py is created twice on device 0 in a fresh child process under the tuning build's
AGX_TRACE_CREATE: with the host planner, whose "plan digest" line hashes the records it uploads, and with the device planner,
whose "device plan digest" line hashes the records copied back from the device.  The two digests must be equal -- kernel choice,
launches, every wave record in dispatch order, every group record -- and where they are not, the "plan parts" lines of both
creates (head, waves and groups hashed apart, the groups, the vacant halves, the launches' columns per lane) go into the
message.  Beyond that: the six agx_sw_info fields, the scores of all pairs (by hash) and, for at most 64 pairs per case (the
empty sides, the 65 535 x 40 and the 1 x 1 pair among them), the scores against the oracle.

The cases are sized for 256 CUs (the verdict and the tiling depend on the count; tests/test_sw_devplan_cpu.py checks the sizes
for that count), so the tests skip on a device with another count.  One child per case, each under its own time limit; a child
that fails, is killed or runs out of time fails its test, and nothing is started again."""
import ctypes as C
import re

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
from tests import oracle_api
from tests import sw_devplan_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu():
    """The device's CU count, asked of the HIP runtime the library itself runs on (hipDeviceAttributeMultiprocessorCount = 63)."""
    agx.lib()
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0, v.value
    return v.value


def _parts(line):
    m = re.search(r"; (\d+) groups, (\d+) vacant halves; launch C((?: \d+)+)$", line)
    assert m, line
    return int(m.group(1)), int(m.group(2)), [int(c) for c in m.group(3).split()]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_device_made_plan_is_the_host_made_plan(oracle, n_cu, name):
    if n_cu != 256:
        pytest.skip("the device has %d CUs: the cases are sized for the device planner's verdict and tiling on 256" % n_cu)
    got, err = dc.run("device", [name], timeout=120)
    host, dev = got[name]["host"], got[name]["device"]
    print(name, "\n host  ", host, "\n device", dev)
    assert host["info"]["planned_on_device"] == 0 and "verdict" not in host and "digest" in host and "device_digest" not in host, err[-3000:]
    assert dev.get("verdict", "").startswith("device planner verdict 1:") and dev["info"]["planned_on_device"] == 1, err[-3000:]
    assert dev.get("on_device") == "on device" and "digest" not in dev and "device_digest" in dev, err[-3000:]
    assert dev["device_digest"] == host["digest"], "the plans differ\n  host:   %s\n  device: %s" % (host["parts"], dev["parts"])
    assert dev["parts"] == host["parts"]
    for f in dc.INFO_FIELDS:
        assert dev["info"][f] == host["info"][f], f
    assert dev["scores_sha256"] == host["scores_sha256"]

    sub = dc.subset(name)
    la, lb, _ = dc.lens(name)
    want = oracle_api.sw_batch_mt(oracle, dc.batch(name).subset(sub))
    assert dev["subset"] == [int(v) for v in want] and host["subset"] == dev["subset"]
    empty = [k for k, p in enumerate(sub) if la[p] == 0 or lb[p] == 0]
    assert all(dev["subset"][k] == 0 for k in empty)
    assert any(v > 0 for v in dev["subset"])

    want_rising = "family 2 rising 0" if name == "tail_65535" else "family 2 rising 4"
    assert host["family"] == want_rising and dev["family"] == want_rising
    groups, vacant, launch_c = _parts(dev["parts"])
    assert dev["info"]["n_launches"] == 1 == len(launch_c)
    if name == "mixed":
        assert vacant > 0 and len(empty) == 4
    if name == "one_class":
        assert launch_c[0] != 0
    else:
        assert launch_c == [0]
    if name == "tail_65535":
        assert 30000 in sub and 59999 in sub  # the 65 535 x 40 pair and the 1 x 1 pair went through the oracle
    if name == "stride":
        assert dev["info"]["n_pairs"] > 16 * 256 * n_cu
