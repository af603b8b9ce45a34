"""Completion on the dispatch (agx_sw.cpp): a one-launch batch of the packed biased fill launches with an event of its own as
the kernel's stop event, and a fetch from its bound array waits for that event while the launch is the stream's last enqueue.
Also the rule for a fetch after agx_sw_batch_bind_scores changed the binding.  Scores against the oracle, bit-exact, and byte for
byte against the same calls with the event taken off.

The batches and call sequences are those of tests/sw_done_event_cases.py.  Child processes on the tuning build run each group
twice -- as shipped, and under AGX_SW_DONE_EVENT=0 -- always under AGX_TRACE_CREATE and AGX_TRACE_FETCH, so that every create says whether the batch
owns a done event and every fetch from a bound array what it waited for; the tests hold those lines too.  All children run side
by side, once for the module; the oracle scores each batch once."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
from tests import sw_done_event_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"on": {}, "off": {"AGX_SW_DONE_EVENT": "0"}}


@pytest.fixture(scope="module")
def children():
    """{(group, form): ({array name: array}, {case: its trace lines})}"""
    with tempfile.TemporaryDirectory() as d:
        procs = {}
        for g in cases.GROUPS:
            for form in FORMS:
                env = dict(os.environ, AGX_TRACE_CREATE="1", AGX_TRACE_FETCH="1", **cases.KNOBS[g], **FORMS[form])
                env.pop("AGX_LIB_PATH", None)
                out = os.path.join(d, "%s_%s.npz" % (g, form))
                procs[(g, form)] = (out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "sw_done_event_cases.py"), g, out],
                                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env))
        got = {}
        for key, (out, p) in procs.items():
            _, err = p.communicate(timeout=300)
            err = err.decode()
            assert p.returncode == 0, (key, err[-2000:])
            with np.load(out) as z:
                arrays = {k: z[k] for k in z.files}
            traces = {}
            for part in re.split(r"^CASE ", err, flags=re.M)[1:]:
                name, _, rest = part.partition("\n")
                traces[name] = rest
            got[key] = (arrays, traces)
        return got


_want = {}


def _oracle(oracle, name, make):
    if name not in _want:
        _want[name] = oracle.sw_batch(make())
    return _want[name]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d pairs differ, first pair %d: got %d, want %d" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def _events(trace):
    return [int(v) for v in re.findall(r"^\[agx_sw_batch_create\] done event (\d)$", trace, flags=re.M)]


def _waits(trace):
    return re.findall(r"^\[agx_sw_batch_scores\] wait: (\w+)$", trace, flags=re.M)


def _bounds(trace):
    return [int(v) for v in re.findall(r"^\[agx_sw_batch_bind_scores\] bound (\d)$", trace, flags=re.M)]


def _against_off(children, group, names):
    on, off = children[(group, "on")][0], children[(group, "off")][0]
    for k in names:
        assert on[k].tobytes() == off[k].tobytes(), "%s %s: differs from the run without the done event" % (group, k)


@pytest.mark.parametrize("n", cases.C38_PAIRS)
def test_c38_unbound_bound_and_rebound(oracle, children, n):
    """One, two and three waves of 38 columns, and the smallest batch that takes the binding: every launch's scores."""
    name = "pairs%d" % n
    want = _oracle(oracle, name, lambda: cases.c38_batch(n))
    on, traces = children[("c38", "on")]
    waves = {32: 1, 64: 2, 80: 3, 1043: 33}[n]
    assert tuple(on["plan_" + name]) == (n, waves, 1), on["plan_" + name]
    keys = ["%s_u%d" % (name, k) for k in range(3)] + ["%s_b%d" % (name, k) for k in range(3)] + [name + "_r"]
    for k in keys:
        _same(on[k], want, k)
    _same(on[name + "_first_after"], want, name + " first array after the rebound launch")
    _against_off(children, "c38", keys)
    # one launch: the batch owns the event; the binding is taken from 1024 pairs in file order on, and only a bound fetch waits for it
    taken = 1 if n >= 1024 else 0
    assert _events(traces[name]) == [1], traces[name]
    assert _bounds(traces[name]) == [taken, taken], traces[name]
    assert _waits(traces[name]) == ["event"] * (4 * taken), traces[name]
    off_trace = children[("c38", "off")][1][name]
    assert _events(off_trace) == [0] and _waits(off_trace) == ["stream"] * (4 * taken), off_trace


def test_mixed_batch_has_the_event_and_the_other_kernels_do_not(oracle, children):
    on, traces = children[("other", "on")]
    assert on["plan_mixed"][2] == 1 and on["plan_mixed"][1] > 1, on["plan_mixed"]
    want = _oracle(oracle, "mixed", cases.mixed_batch)
    for k in range(3):
        _same(on["mixed_%d" % k], want, "mixed launch %d" % k)
    _same(on["i32"], _oracle(oracle, "i32", cases.i32_batch), "int32 kernel")
    _same(on["align"], _oracle(oracle, "align", cases.align_batch), "align batch")
    _against_off(children, "other", ["mixed_0", "mixed_1", "mixed_2", "i32", "align"])
    assert _events(traces["mixed"]) == [1], traces["mixed"]
    assert _events(traces["i32"]) == [0], traces["i32"]
    assert _events(traces["align"]) == [0], traces["align"]
    off_traces = children[("other", "off")][1]
    assert [_events(off_traces[c]) for c in ("mixed", "i32", "align")] == [[0]] * 3


def test_two_batches_interleaved_on_one_context(oracle, children):
    """Launch A, launch B, fetch A: A's event is not the stream's last enqueue, so the fetch waits for the stream.  B's is; and so
    is A's when it is launched alone, also for a second fetch with no launch between."""
    on, traces = children[("other", "on")]
    want_a, want_b = _oracle(oracle, "a", cases.batch_a), _oracle(oracle, "b", cases.batch_b)
    _same(on["a_behind_b"], want_a, "A fetched behind B's launch")
    _same(on["b_last"], want_b, "B")
    _same(on["a_alone"], want_a, "A alone")
    _same(on["a_again"], want_a, "A fetched again")
    _against_off(children, "other", ["a_behind_b", "b_last", "a_alone", "a_again"])
    assert _bounds(traces["interleave"]) == [1, 1], traces["interleave"]
    assert _waits(traces["interleave"]) == ["stream", "event", "event", "event"], traces["interleave"]
    assert _waits(children[("other", "off")][1]["interleave"]) == ["stream"] * 4


def test_fetch_after_the_bound_array_changed(oracle, children):
    """Bind, launch, unbind, fetch: E_ARG until the next launch, whichever array is asked for; the same after a rebind."""
    want = _oracle(oracle, "a", cases.batch_a)
    for form in FORMS:
        got = children[("other", form)][0]
        assert list(got["code_after_unbind"]) == [agx.E_ARG, agx.E_ARG], (form, got["code_after_unbind"])
        _same(got["after_unbind_launch"], want, form + ": launched after the unbind")
        assert list(got["code_after_rebind"]) == [agx.E_ARG, agx.E_ARG], (form, got["code_after_rebind"])
        _same(got["after_rebind_launch"], want, form + ": launched after the rebind")
        assert list(got["code_same_array"]) == [agx.OK], (form, got["code_same_array"])
