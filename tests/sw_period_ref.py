"""The class period of the biased packed Smith-Waterman fill's column classes (agx_sw.cpp, "class period"), restated in plain
Python next to tests/sw_range_ref.py.

A batch on the rising cell with column classes (kc == 4 in sw_range_ref.variant) runs them with period C / 2 in every class of
C >= 14 columns per lane that is built that way ("wide"), and with period 4 everywhere ("narrow") otherwise.  Column j of a lane
carries (j mod P) |ge|, so the wide kernel's values stand up to (P - 1) |ge| higher where the narrow one's stood 3 |ge| higher.
With P the largest period among the classes the batch launches, the batch is wide when

    B + (ls + 1) match + |gf| + (ll + 65 + P) |ge| < 0x7c00

-- the rising cell's own rule (sw_range_ref: + (ll + 69) |ge|) with P in the place of 4.  The sum bounds, with steps <= ll + 63,
    the diagonal sum          B + (ls + 1) match        + (steps + P - 1) |ge|
    z, f ahead of its wrap    B + ls match - |gf|       + (steps + P) |ge|
    the running maxima        B + ls match - |gf|       + (steps + P + 4) |ge|     (|gf| >= |ge|, match >= 1)
and from below every half is a true value of at least B - max(|gf|, -mismatch) >= 0x0400 plus an offset that is never negative.

This file only FINDS the edge; scores are always compared with the oracle's."""
from tests import sw_range_ref as ref

NARROW = 4
WIDE_FROM = 14          # columns per lane from which the column classes are used at all
KEEP_NARROW = ()        # classes whose wide build does not fit two waves per SIMD: none
PACKED_CLASSES = tuple(range(4, 41, 2))


def period(C):
    """The period class C runs in a wide batch."""
    return C // 2 if C >= WIDE_FROM and C not in KEEP_NARROW else NARROW


def wide(scoring, ls, ll, P):
    """Whether a batch with these longest sides, whose widest launched period is P, runs the wide kernels."""
    if ref.variant(scoring, ls, ll) != ("biased", 4) or P <= NARROW:
        return False
    _, _, _, ge, _ = ref._terms(scoring)
    return ref._top(scoring, ls) + (ll + 65 + P) * ge < ref.TOP


def last_wide_ll(scoring, ls, P):
    """The largest ll in ls .. 65535 that is still wide beside ls columns at period P; None when none is."""
    if not wide(scoring, ls, ls, P):
        return None
    lo, hi = ls, ref.MAX_LONG
    while lo < hi:  # monotonic in ll
        mid = (lo + hi + 1) // 2
        if wide(scoring, ls, mid, P):
            lo = mid
        else:
            hi = mid - 1
    return lo
