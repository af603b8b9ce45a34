"""The staged wave priority of the packed SW fill (SwParams::stage; agx_sw_pk2_kernel.inc, "Staged priority") and the wave counts
at which a launch's shape can go wrong: scores against the oracle, bit-exact, and staging on against staging off, byte for byte.

The batches are those of tests/sw_launch_shape_cases.py: 150 x 150 DNA pairs in 1, 2, 3, 5 and 9 waves of 38 columns per lane
(a lone wave, a partly filled last workgroup, a vacant half), a mixed batch of 7 waves in the one-launch kernel, and uniform
batches of exactly 8 x CUs waves -- the last that is resident at once, which the host stages -- and of one wave more, which it
must not.  Child processes on the tuning build score every group four ways: as planned and under AGX_SW_STAGE=0, each at the
class period the host chose and under AGX_SW_PERIOD=4 (the limit group runs 4 columns per lane, which has one period: two ways).
Every child runs under AGX_TRACE_CREATE, so each create says whether it staged; the test holds that too.  All children run side
by side, once for the module; the oracle scores each batch once."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
from tests import sw_launch_shape_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"staged": {}, "unstaged": {"AGX_SW_STAGE": "0"}, "staged_p4": {"AGX_SW_PERIOD": "4"},
         "unstaged_p4": {"AGX_SW_PERIOD": "4", "AGX_SW_STAGE": "0"}}


def _forms(group):
    return ("staged", "unstaged") if group == "limit" else tuple(FORMS)


@pytest.fixture(scope="module")
def n_cu():
    """The device's CU count, asked of the HIP runtime the library itself runs on (hipDeviceAttributeMultiprocessorCount = 63)."""
    import ctypes as C

    agx.lib()
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0, v.value
    return v.value


@pytest.fixture(scope="module")
def children(n_cu):
    """{(group, form): {case: (scores, (pairs, waves, launches), staged, waves traced, resident traced, period run or None)}}"""
    with tempfile.TemporaryDirectory() as d:
        procs = {}
        for g in cases.GROUPS:
            for form in _forms(g):
                env = dict(os.environ, AGX_TRACE_CREATE="1", **cases.KNOBS[g], **FORMS[form])
                env.pop("AGX_LIB_PATH", None)
                out = os.path.join(d, "%s_%s.npz" % (g, form))
                procs[(g, form)] = (out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "sw_launch_shape_cases.py"), g, out, str(n_cu)],
                                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env))
        got = {}
        for key, (out, p) in procs.items():
            _, err = p.communicate(timeout=300)
            err = err.decode()
            assert p.returncode == 0, (key, err[-2000:])
            res = {}
            with np.load(out) as z:
                for part in re.split(r"^CASE ", err, flags=re.M)[1:]:
                    name = part.split("\n", 1)[0]
                    m = re.findall(r"staged priority (\d): (\d+) waves, (\d+) resident at once\n", part)
                    assert len(m) == 1, (key, part)
                    per = re.findall(r"class period (\d+) of \d+\n", part)
                    res[name] = (z[name], tuple(int(v) for v in z["pairs_" + name]), int(m[0][0]), int(m[0][1]), int(m[0][2]),
                                 int(per[0]) if per else None)
            got[key] = res
        return got


_want = {}


def _batch(group, name, pairs):
    if group == "c38":
        return cases.c38_batch(int(name[len("waves"):]))
    return cases.mixed_batch(pairs) if group == "mixed" else cases.tiny_batch(pairs)


def _oracle(oracle, group, name, pairs):
    if (group, name) not in _want:
        _want[(group, name)] = oracle.sw_batch(_batch(group, name, pairs))
    return _want[(group, name)]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d pairs differ, first pair %d: got %d, want %d" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("group", cases.GROUPS)
def test_scores_against_the_oracle_staged_and_not(oracle, children, group):
    base = children[(group, "staged")]
    assert base, group
    for name, (scores, (pairs, waves, launches), *_rest) in base.items():
        want = _oracle(oracle, group, name, pairs)
        for form in _forms(group):
            got, plan, *_ = children[(group, form)][name]
            assert plan == (pairs, waves, launches), (group, form, name, plan)
            _same(got, want, "%s %s %s against the oracle" % (group, name, form))
            assert got.tobytes() == scores.tobytes(), "%s %s: %s differs from the staged run" % (group, name, form)


def test_wave_counts_and_kernels(children):
    """The shapes the cases are named for: 1, 2, 3, 5, 9 waves at period 19 (and at 4 under the knob), 7 waves in one launch."""
    for form in FORMS:
        c38 = children[("c38", form)]
        assert [c38["waves%d" % w][1][1:] for w in cases.WAVES_C38] == [(w, 1) for w in cases.WAVES_C38], (form, c38.keys())
        assert {v[5] for v in c38.values()} == {4 if form.endswith("p4") else 19}, form
        (name, v), = children[("mixed", form)].items()
        assert v[1][1:] == (cases.MIXED_WAVES, 1), (form, v[1])
        assert (v[5] == 4) == form.endswith("p4"), (form, v[5])


def test_staging_follows_the_resident_at_once_rule(children, n_cu):
    """Staged exactly when every wave is resident at once -- two on each of a CU's four SIMDs -- and never under AGX_SW_STAGE=0."""
    limit = 8 * n_cu
    for (group, form), res in children.items():
        for name, (_, (pairs, waves, launches), staged, traced_waves, resident, _period) in res.items():
            assert traced_waves == waves and resident == limit, (group, form, name, traced_waves, waves, resident, limit)
            assert staged == (1 if form.startswith("staged") and waves <= limit else 0), (group, form, name, staged, waves, limit)
    at, above = children[("limit", "staged")]["at_limit"], children[("limit", "staged")]["above_limit"]
    assert at[1][1] == limit and at[2] == 1, at[1:]
    assert above[1][1] == limit + 1 and above[2] == 0, above[1:]
