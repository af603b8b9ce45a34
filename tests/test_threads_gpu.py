"""The threading contract of include/agx.h on a real device, with several host threads inside the library at once:

  a. a context and everything created from it belong to one host thread at a time; distinct contexts may be used from distinct
     threads -- four threads, four contexts, every kernel family;
  b. the first device-planned create of two fresh contexts at the same time (the two once_per_context mutexes of csrc/agx_sw.cpp);
  c. agx_sw_score_devices and agx_phmm_forward_devices are callable from several host threads at once, and agx_warmup_devices runs
     beside them: calls take turns on each (device, shard slot) context;
  d. agx_pairHMM beside them: it uses the process-wide context (device 0, slot 0) under that context's busy mutex, as the first
     shard of a device list does;
  e. agx_last_error() is per thread.

Each test runs its body (tests/threads_cases.py, CHILDREN) in one fresh child process with at most four caller threads and one
time limit.  In the child every thread is released by one barrier, every join has a time limit, and a thread that does not come
back makes the child print every thread's stack and exit: a deadlock is reported with its place; nothing is run a second time.
What a child expects is computed before its threads start, from tests/oracle_api.py and the by-definition checkers (sw_align_ref
and sw_modes_ref through sw_stats_ref.hits, sw_stats_ref, sw_cigar_ref, sw_band_diag_ref, sw_band_zdrop_ref), never from the
library; in (a) every result is also compared, bit for bit, with the same call made alone before the barrier.  Every child
asserts that calls of different threads were inside the library at the same time.

Time limits: ten times the child's wall time measured once on an MI355X, and at least 60 s, so that only a deadlock reaches the
limit, not a busy machine.  Measured -- the whole child process (interpreter start, inputs and reference values included), its
threaded part, library calls made by the threads, pairs of calls of different threads that overlapped:
    contexts  1.80 s   0.10 s   126 calls   111 overlaps
    devplan   0.61 s   0.21 s     8 calls     7 overlaps
    devices   1.16 s   0.24 s    21 calls    40 overlaps
    seam      0.54 s   0.13 s    92 calls   128 overlaps
    errors    0.62 s   0.04 s    40 calls    27 overlaps
Ten times each is below 60 s, so every child gets 60 s; a caller that has not come back after threads_cases.JOIN_S = 40 s is
reported by the child itself."""
import pytest

from tests import threads_cases as tc

pytestmark = pytest.mark.gpu

MEASURED_S = {"contexts": 1.80, "devplan": 0.61, "devices": 1.16, "seam": 0.54, "errors": 0.62}  # whole child, on an MI355X


def _limit(name):
    limit = max(60.0, 10.0 * MEASURED_S[name])
    assert limit > tc.JOIN_S  # the child reports a stuck caller before its own time runs out
    return limit


def test_distinct_contexts_on_distinct_threads():
    print(tc.run("contexts", _limit("contexts")))


def test_first_device_planned_create_on_two_fresh_contexts_at_once():
    print(tc.run("devplan", _limit("devplan")))


def test_device_lists_from_three_threads_beside_a_warmup():
    print(tc.run("devices", _limit("devices")))


def test_function_seam_beside_the_device_lists():
    print(tc.run("seam", _limit("seam")))


def test_error_text_is_per_thread():
    print(tc.run("errors", _limit("errors")))
