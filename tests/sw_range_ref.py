"""The host's choice of the score-only Smith-Waterman kernel (agx_sw.cpp, "kernel family"), restated in plain Python.

The biased packed fill (agx_sw_pk2_kernel.hip) is exact only while every stored 16-bit half is the pattern of a positive
normal half-precision number, [0x0400, 0x7c00).  Three inequalities over the scoring, the batch's longest shorter side
ls and its longest longer side ll decide whether a batch stays inside:

    biased (else the signed packed kernel):     B + (ls + 1) match + |gf| < 0x7c00
    rising-offset cell (else the plain cell):   the same sum + (ll + 69) |ge| < 0x7c00
    column classes (KC = 4, else KC = 1):       mismatch + |gf| - 3 |ge| >= 0

with gf = gap_open + gap_extend, ge = gap_extend and B = 0x0400 + max(|gf| + |ge|, match - mismatch).

This file only FINDS the edges of those rules for tests/test_sw_range_cpu.py and tests/test_sw_range_gpu.py; the value a
score is compared with is always the oracle's."""

TOP = 0x7C00            # first pattern that is no finite half-precision number
BOTTOM = 0x0400         # first normal one
MAX_SHORT = 2560        # columns of the packed kernels: 64 lanes x 40
MAX_LONG = 65535
RISING_SLACK = 69       # steps <= ll + 63, z carries (t + 2 + class) |ge|, class <= 3, one more for u = z_diag + hd


def _terms(scoring):
    match, mismatch, gap_open, gap_extend = scoring
    gf, ge = -(gap_open + gap_extend), -gap_extend
    bias = BOTTOM + max(gf + ge, match - mismatch)
    return match, mismatch, gf, ge, bias


def _top(scoring, ls):
    match, _, gf, _, bias = _terms(scoring)
    return bias + (ls + 1) * match + gf


def variant(scoring, ls, ll):
    """-> (family, kc): family "biased" / "signed"; kc 0 (plain cell, and every signed batch), 1 (rising), 4 (rising with column classes)."""
    assert 1 <= ls <= MAX_SHORT and ls <= ll <= MAX_LONG
    _, mismatch, gf, ge, _ = _terms(scoring)
    if not _top(scoring, ls) < TOP:
        return "signed", 0
    if not _top(scoring, ls) + (ll + RISING_SLACK) * ge < TOP:
        return "biased", 0
    return "biased", 4 if mismatch + gf - 3 * ge >= 0 else 1


def last_biased_ls(scoring):
    """The largest ls <= 2560 the biased kernel still takes; None when that is no ls at all."""
    ok = [ls for ls in range(1, MAX_SHORT + 1) if variant(scoring, ls, ls)[0] == "biased"]
    return max(ok) if ok else None


def last_rising_ll(scoring, ls):
    """The largest ll in ls .. 65535 that still runs the rising cell beside a longest shorter side of ls; None when none does."""
    lo, hi = ls, MAX_LONG
    if variant(scoring, ls, lo)[1] == 0:
        return None
    while lo < hi:  # the rule is monotonic in ll
        mid = (lo + hi + 1) // 2
        if variant(scoring, ls, mid)[1]:
            lo = mid
        else:
            hi = mid - 1
    return lo


# The scorings both test files walk: scoring -> (ls values whose ll edge is tested, whether the ls edge is).
# Chosen for the cell they select and for how little slack they leave: constant 0 / -1 of the third rule (either side of the
# KC edge), a large |ge| (small edges), gap_open = 0 (|gf| = |ge|, the least slack), the largest B (plain biased only), and
# match - mismatch = 128 (no coded match).
CASES = {
    (1, -1, -3, -1): ((2560, 150, 4), False),      # the reference's scoring: KC = 4, constant exactly 0
    (3, -1, -3, -1): ((2560,), False),             # KC = 4, constant 0
    (1, -2, -3, -1): ((2560, 150, 4), False),      # KC = 1, constant -1
    (4, -1, -30, -5): ((40, 2560), False),         # KC = 4, larger |ge|
    (1, -3, 0, -2): ((40, 2560), False),           # KC = 1, |gf| = |ge|
    (8, -2, -20, -16): ((40, 2560), False),        # KC = 1, the smallest edges; no rising cell at all beside 2560 columns
    (12, -100, -50, -7): ((40,), True),            # KC = 1
    (12, -4, -10, -3): ((), True),                 # KC = 4
    (12, -1, -1000, -1000): ((), True),            # plain biased only, the largest B
    (12, -116, -1000, -1000): ((), True),          # ... and delta = 128
    (12, 0, 0, -1): ((), True),                    # KC = 1, free mismatch and free gap open
}
