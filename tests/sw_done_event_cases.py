"""The batches and call sequences of tests/test_sw_done_event_gpu.py, the same in every process that runs them.

The done event of a one-launch packed batch (agx_sw.cpp, "Completion on the dispatch") is taken off by a knob of the tuning build
(AGX_SW_DONE_EVENT=0), so the test runs this file as a program in child processes (tests/sw_launch_shape_cases.py is the model),
always under AGX_TRACE_CREATE and AGX_TRACE_FETCH: every create then says whether the batch owns a done event, every bind_scores whether the array
was taken, and every fetch from a bound array what it waited for.
    usage: python tests/sw_done_event_cases.py GROUP OUT.npz      (stderr: "CASE name" ahead of each case's trace lines)

  c38    (AGX_SW_FORCE_C=38) 150 x 150 DNA pairs in one, two and three waves of 38 columns per lane -- 32, 64 and 80 pairs, the
         last wave half vacant; bind_scores is a hint for them (no file order below 1024 pairs) -- and 1043 pairs, 33 waves with a
         vacant half, which is the smallest batch that does take the binding.  Each: three launches unbound, three bound to one
         array, one more bound to a second array.
  other  a mixed batch of 300 pairs of 32 .. 512 (the one-launch kernel, with the event), a uniform batch through the int32
         kernel and a small align batch (neither has one); two bound batches interleaved on one context; fetches after unbind
         and rebind"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import accelerating_genomics_amd.synth as synth  # noqa: E402

KNOBS = {"c38": {"AGX_SW_FORCE_C": "38"}, "other": {}}
GROUPS = tuple(KNOBS)
C38_PAIRS = (32, 64, 80, 1043)


def c38_batch(n):
    return synth.sw_pairs(n, 150, 150, seed=700 + n, related_frac=0.4)


def mixed_batch():
    return synth.sw_pairs(300, 32, 512, seed=77, related_frac=0.5)


def i32_batch():
    return synth.sw_pairs(100, 150, 150, seed=9, related_frac=0.4)


def align_batch():
    return synth.sw_pairs(60, 40, 200, seed=10, related_frac=0.5)


def batch_a():
    return synth.sw_pairs(1043, 150, 150, seed=21, related_frac=0.4)


def batch_b():
    return synth.sw_pairs(1030, 100, 100, seed=22, related_frac=0.4)


def _case(name):
    sys.stderr.write("CASE %s\n" % name)
    sys.stderr.flush()


def _plan(dev, b):
    i = dev.info()
    return np.array([b.n_pairs, i.n_waves, i.n_launches], np.int64)


def run_c38(agx, ctx, got):
    for n in C38_PAIRS:
        name = "pairs%d" % n
        _case(name)
        b = c38_batch(n)
        dev = ctx.sw_batch(b)
        try:
            got["plan_" + name] = _plan(dev, b)
            for k in range(3):
                dev.launch()
                got["%s_u%d" % (name, k)] = dev.scores()
            first, second = agx.host_array(n, np.int32), agx.host_array(n, np.int32)
            first[:] = -5
            second[:] = -6
            dev.bind_scores(first)
            for k in range(3):
                dev.launch()
                dev.scores(first)
                got["%s_b%d" % (name, k)] = first.copy()
            dev.bind_scores(second)
            dev.launch()
            dev.scores(second)
            got[name + "_r"] = second.copy()
            got[name + "_first_after"] = first.copy()  # the second array's launch leaves the first alone
        finally:
            dev.close()


def _code(agx, call):
    try:
        call()
    except agx.AgxError as e:
        return e.code
    return agx.OK


def run_other(agx, ctx, got):
    _case("mixed")
    b = mixed_batch()
    dev = ctx.sw_batch(b)
    got["plan_mixed"] = _plan(dev, b)
    for k in range(3):
        dev.launch()
        got["mixed_%d" % k] = dev.scores()
    dev.close()

    _case("i32")
    b = i32_batch()
    ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_INT32)
    try:
        dev = ctx.sw_batch(b)
    finally:
        ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
    dev.launch()
    got["i32"] = dev.scores()
    dev.close()

    _case("align")
    b = align_batch()
    dev = ctx.sw_batch(b, align=agx.SW_ALIGN_ENDS)
    dev.launch()
    got["align"] = dev.scores()
    dev.close()

    _case("interleave")
    a, b = batch_a(), batch_b()
    out_a, out_b = agx.host_array(a.n_pairs, np.int32), agx.host_array(b.n_pairs, np.int32)
    dev_a, dev_b = ctx.sw_batch(a), ctx.sw_batch(b)
    dev_a.bind_scores(out_a)
    dev_b.bind_scores(out_b)
    out_a[:] = -1
    out_b[:] = -1
    dev_a.launch()
    dev_b.launch()
    dev_a.scores(out_a)  # B's launch is behind A's on the stream: the stream wait
    got["a_behind_b"] = out_a.copy()
    dev_b.scores(out_b)  # the stream's last enqueue is B's launch
    got["b_last"] = out_b.copy()
    out_a[:] = -1
    dev_a.launch()
    dev_a.scores(out_a)
    got["a_alone"] = out_a.copy()
    dev_a.scores(out_a)  # no launch between
    got["a_again"] = out_a.copy()
    dev_b.close()

    _case("stale")
    dev_a.launch()
    dev_a.bind_scores(None)
    got["code_after_unbind"] = np.array([_code(agx, dev_a.scores), _code(agx, lambda: dev_a.scores(out_a))])
    dev_a.launch()
    got["after_unbind_launch"] = dev_a.scores()
    dev_a.bind_scores(out_a)
    got["code_after_rebind"] = np.array([_code(agx, lambda: dev_a.scores(out_a)), _code(agx, dev_a.scores)])
    out_a[:] = -1
    dev_a.launch()
    dev_a.scores(out_a)
    got["after_rebind_launch"] = out_a.copy()
    dev_a.bind_scores(out_a)  # the same array again: nothing changed, the fetch stands
    got["code_same_array"] = np.array([_code(agx, lambda: dev_a.scores(out_a))])
    dev_a.close()


def main(group, path):
    import accelerating_genomics_amd.api as agx

    assert agx.LIB_PATH.endswith("libagx_tuning.so"), agx.LIB_PATH
    got = {}
    with agx.Context(0) as ctx:
        (run_c38 if group == "c38" else run_other)(agx, ctx, got)
    np.savez(path, **got)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
