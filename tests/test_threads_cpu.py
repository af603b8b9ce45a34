"""Plan-only creates from several host threads at once (no device: ctx = NULL).

Every create runs its planner stages on the one process-wide worker pool, in which a caller waiting for its parts runs whatever
is queued -- another caller's parts included (run_on, csrc/agx_runtime.cpp).  Four Python threads, released by one barrier,
create the cases of tests/threads_cases.py for several rounds, each in another rotation, from inputs they share and only read
(ctypes drops the GIL for every call).  The info() of every create must equal, field by field, the info() of the same create
made alone before the threads started: a plan does not depend on who ran a pool part."""
import ctypes as C

import accelerating_genomics_amd.api as agx
from tests import threads_cases as tc

THREADS, ROUNDS = 4, 3


def test_plan_only_creates_from_four_threads_give_the_plans_made_alone():
    lib = agx.lib()
    lib.agx_host_threads_c.restype = C.c_int
    assert lib.agx_host_threads_c() >= 2, "one pool thread: no stage splits, nothing is shared between the callers"
    batches = tc.plan_batches()
    cases = tc.plan_cases(agx)
    families = {c[1].split("_")[0] for c in cases}
    assert families == {"sw", "align", "stats", "cigar", "band", "phmm"}
    alone = {c[1]: tc.plan_info(agx, batches, c) for c in cases}
    for name, info in alone.items():
        assert info["n_pairs"] >= 16384 and info["n_waves"] > 0 and info["cells"] > 0 and info["padded_cells"] > 0, (name, info)
    differing = []

    def body(t):
        def f(timed):
            k = t * len(cases) // THREADS
            for case in (cases[k:] + cases[:k]) * ROUNDS:
                got = timed(tc.plan_info, agx, batches, case)
                if got != alone[case[1]]:
                    differing.append((t, case[1], got, alone[case[1]]))
        return f

    spans = tc.run_callers([body(t) for t in range(THREADS)], join_timeout=300.0)
    assert all(len(s) == ROUNDS * len(cases) for s in spans)
    assert not differing, "%d creates differ from the same create made alone, first: %s" % (len(differing), differing[0])
    n = tc.overlaps(spans)
    print("creates %d, overlapping pairs of calls %d" % (sum(len(s) for s in spans), n))
    assert n >= 1, "no two creates of different threads overlapped: the test did not test what it is for"
