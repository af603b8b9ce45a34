"""The packed SW fill with column classes of period C / 2 (agx_sw_pk2w_kernel.hip) against the oracle, bit-exact, and against the
same batches forced to the period of four.

The batches are those of tests/sw_period_cases.py.  This process scores the "natural" group on the shipped library; child
processes on the tuning build score every group once as planned and once under AGX_SW_PERIOD=4, the groups c14 / c38 / c40 with
the columns per lane pinned (AGX_SW_FORCE_C): the smallest and the largest wide class at one, two and 64 lanes a group, and 38
columns for the tail steps and the edge of the host's rule.  Every child runs under AGX_TRACE_CREATE, so each create says which
period it ran: the test holds that too.  All children run side by side, once for the module."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
from tests import oracle_api
from tests import sw_period_cases as cases
from tests import sw_period_ref as pref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = cases.GROUPS


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def batches():
    return {g: cases.cases(g) for g in GROUPS}


@pytest.fixture(scope="module")
def children():
    """{(group, 'wide' | 'narrow'): ({case: scores}, {case: (period run, widest period launched, launches)})}"""
    with tempfile.TemporaryDirectory() as d:
        procs = {}
        for g in GROUPS:
            for form in ("wide", "narrow"):
                env = dict(os.environ, AGX_TRACE_CREATE="1", **cases.KNOBS[g])
                env.pop("AGX_LIB_PATH", None)
                if form == "narrow":
                    env["AGX_SW_PERIOD"] = "4"
                out = os.path.join(d, "%s_%s.npz" % (g, form))
                procs[(g, form)] = (out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "sw_period_cases.py"), g, out],
                                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env))
        got = {}
        for key, (out, p) in procs.items():
            _, err = p.communicate(timeout=300)
            err = err.decode()
            assert p.returncode == 0, (key, err[-2000:])
            periods = {}
            for part in re.split(r"^CASE ", err, flags=re.M)[1:]:
                m = re.findall(r"class period (\d+) of (\d+)\n", part)
                assert len(m) == 1, (key, part)
                periods[part.split("\n", 1)[0]] = (int(m[0][0]), int(m[0][1]), int(re.findall(r"^LAUNCHES (\d+)$", part, flags=re.M)[0]))
            with np.load(out) as z:
                got[key] = ({k: z[k] for k in z.files}, periods)
        return got


_want = {}


def _oracle(oracle, group, name, scoring, b):
    """The oracle's scores of a case, worked out once: slices of the batch on the host's cores."""
    if (group, name) not in _want:
        n = b.n_pairs
        cells = b.len[0::2].astype(np.int64) * b.len[1::2].astype(np.int64)
        order = np.argsort(-cells, kind="stable")
        t = max(1, min(oracle_api._threads(), n))
        parts = [order[k::t] for k in range(t)]  # long pairs spread over the threads
        with ThreadPoolExecutor(t) as ex:
            res = list(ex.map(lambda idx: oracle.sw_batch_scored(b.subset(idx), scoring), parts))
        want = np.empty(n, np.int32)
        for idx, r in zip(parts, res):
            want[idx] = r
        _want[(group, name)] = want
    return _want[(group, name)]


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d pairs differ, first pair %d: got %d, want %d" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def test_shipped_library_on_the_natural_group(ctx, oracle, batches, children):
    """32 768 pairs of 150 x 150 with sentinels on the default library, no knob: 4 lanes of 38 columns by the planner's own choice,
    at period 19 (the children's traces of the same batch say so), against the oracle and against the tuning build's narrow run."""
    narrow, periods = children[("natural", "narrow")]
    for name, scoring, b in batches["natural"]:
        dev = ctx.sw_batch(b, scoring)
        try:
            dev.launch()
            got = dev.scores()
        finally:
            dev.close()
        _same(got, _oracle(oracle, "natural", name, scoring, b), "natural " + name)
        _same(got, narrow[name], "natural %s against the period of four" % name)
        assert periods[name][:2] == (pref.NARROW, pref.period(38)), (name, periods[name])  # (the knob held a wide batch back)
        assert children[("natural", "wide")][1][name][:2] == (pref.period(38), pref.period(38))


@pytest.mark.parametrize("group", GROUPS)
def test_wide_and_narrow_runs_against_the_oracle(oracle, batches, children, group):
    wide, wp = children[(group, "wide")]
    narrow, np_ = children[(group, "narrow")]
    top = pref.period(cases.FORCED[group]) if group in cases.FORCED else None
    for name, scoring, b in batches[group]:
        want = _oracle(oracle, group, name, scoring, b)
        _same(wide[name], want, "%s %s as planned" % (group, name))
        _same(narrow[name], want, "%s %s at the period of four" % (group, name))
        outside = name == "edge_outside"
        W = wp[name][1]
        assert W > pref.NARROW and (top is None or W == top), (group, name, wp[name])
        assert wp[name][0] == (pref.NARROW if outside else W), (group, name, wp[name])
        assert np_[name][:2] == (pref.NARROW, W), (group, name, np_[name])
        if group == "mixed":  # several classes in ONE launch: sw_fill_pk2w_any
            assert wp[name][2] == 1 and len(np.unique(b.len.reshape(-1, 2).min(axis=1))) > 100, wp[name]


def test_edge_batches_stand_on_the_rule_s_edge(batches):
    """edge_inside has its longest longer side on the last ll the restated rule calls wide at period 19, edge_outside one beyond."""
    by = {name: (scoring, b) for name, scoring, b in batches["c38"]}
    P = pref.period(38)
    L = pref.last_wide_ll(cases.EDGE, 150, P)
    for name, longest, want in (("edge_inside", L, True), ("edge_outside", L + 1, False)):
        scoring, b = by[name]
        l = b.len.reshape(-1, 2)
        assert (int(l.min(axis=1).max()), int(l.max(axis=1).max())) == (150, longest), name
        assert pref.wide(scoring, 150, longest, P) == want
