"""The biased packed Smith-Waterman fill (agx_sw_pk2_kernel.hip) at the edges of its value range.

Its packed maxima (v_pk_maximum3_f16) are exact integer maxima only while every stored 16-bit half lies in
[0x0400, 0x7c00); agx_sw.cpp keeps a batch inside by three inequalities over the scoring and the batch's longest sides
(restated in tests/sw_range_ref.py, held against the library in tests/test_sw_range_cpu.py).  The batches here stand on
the LAST length each inequality still accepts and one beyond it, with the best alignment ending in the last rows, where
score and rising offset are both at their largest.  Every score is compared bit-exactly with the oracle's Gotoh; the
restated rule only finds the lengths."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import oracle_api
from tests import sw_range_ref as ref

pytestmark = pytest.mark.gpu

NL = b"\n"
FORMS = ((True, True), (True, False), (False, True), (False, False))  # final newline on (x, y)
AMINO_X, AMINO_Y = b"ARNDCQEGHI", b"LKMFPSTWYV"                        # two disjoint halves of the protein alphabet
KINDS = ("end", "start", "homo")


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def own():
    """The context the forced kernels run on: the default one never has its kernel option changed."""
    with agx.Context(0) as c:
        yield c


def _rand(rng, alphabet, n):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def _pair(rng, kind, ls, rows, form, general, swap):
    """One pair whose shorter side x has ls symbols and whose longer side y has `rows`, final newlines included.
    end:   y = unrelated symbols, then a copy of x -- the maximum is reached in the last rows;
    start: y = the copy of x, then unrelated symbols -- an early maximum that has to survive `rows` steps;
    homo:  one symbol throughout -- every cell ties and the whole last row stands at the top value.
    general: more than four symbols in x, or a newline inside it, so that the wave runs the general cell, not the DNA-coded one.
    -> (x, y in batch order, the score an alignment of the whole copy gives in matches: the pair's score is match times that)."""
    nlx, nly = form
    cx, cy = ls - nlx, rows - nly  # symbols before the final newline
    if kind == "homo":
        x, y = b"A" * cx, b"A" * cy
        if general and cx >= 2:  # a newline that is not the last symbol: no sentinel to strip
            x, y = NL + x[1:], NL + y[1:]
    else:
        ax, ay = (AMINO_X, AMINO_Y) if general else (b"AC", b"GT")
        x = _rand(rng, ax, cx)
        if general and cx >= 8:
            x = ax[:8] + x[8:]  # at least eight distinct symbols
        elif general and cx >= 3:
            x = x[:1] + NL + x[2:]
        other = _rand(rng, ay, cy - cx)
        y = other + x if kind == "end" else x + other
    top = cx + (1 if nlx and nly and (kind != "start" or cy == cx) else 0)  # (start: y's final newline is far from the copy's end)
    x, y = x + NL * nlx, y + NL * nly
    assert len(x) == ls and len(y) == rows
    return ((y, x) if swap else (x, y)), top


def _filler(rng, ls, n=30):
    """Short random pairs, half of them related: the wave of the long pair also holds vacant halves and idle lanes."""
    seqs = []
    for k in range(n):
        lx = int(rng.integers(1, max(2, min(ls, 60))))  # with its newline no longer than ls
        a = _rand(rng, b"ACGT", lx)
        y = _rand(rng, b"ACGT", int(rng.integers(0, 60)))
        y = y + a + _rand(rng, b"ACGT", int(rng.integers(0, 9))) if k % 2 else y + _rand(rng, b"ACGT", lx)
        if k % 5 == 3 and lx > 2:
            a = a[:1] + b"N" + a[2:]
        seqs += [a + NL, y + NL] if k % 3 else [y, a]
    return seqs


def ll_edge_batch(scoring, ls, L, longest):
    """The batch of an ll edge: longest shorter side exactly ls, longest longer side exactly `longest` (L, or L + 1 in the worst pair
    alone).  -> (SWBatch, [(pair number, expected matches)] of the pairs whose score is known by construction)."""
    rng = np.random.default_rng(1000 * ls + L)  # the L and the L + 1 batch draw the same symbols
    seqs, known = [], []

    def add(pair, top):
        known.append((len(seqs) // 2, top))
        seqs.extend(pair)

    for ki, kind in enumerate(KINDS):
        for ri in range(4):  # rows L .. L - 3: every tail length of the quad loop, both parities of the quad count
            rows = L - ri if L - ri >= ls else L
            if ki == 0 and ri == 0:
                rows = longest
            pair, top = _pair(rng, kind, ls, rows, FORMS[(ki + ri) % 4], False, ri % 2 == 1)
            add(pair, top)
        pair, top = _pair(rng, kind, ls, L, FORMS[(0, 3, 2)[ki]], True, ki % 2 == 1)
        add(pair, top)
    for lx in (1, 4):  # single-lane groups: the fewest skew steps
        if lx < ls:
            pair, top = _pair(rng, "end", lx, L, FORMS[3], False, False)
            add(pair, top)
    seqs += _filler(rng, ls)
    return synth.sw_from_seqs(seqs), known


def ls_edge_batch(scoring, ls):
    rng = np.random.default_rng(7000 + ls)
    x = _rand(rng, b"ACGT", ls - 1) + NL
    cut = ls // 2
    seqs = [x, x,                                                             # identical: match * ls
            x, x[:cut] + x[cut + 100:-1] + _rand(rng, b"ACGT", 150) + NL,     # a 100-symbol deletion and a tail
            x, x[-2::-1] + NL]                                                # reversed
    seqs += _filler(rng, ls)
    return synth.sw_from_seqs(seqs), [(0, ls)]


def _sides(b):
    l = b.len.reshape(-1, 2)
    return int(l.min(axis=1).max()), int(l.max(axis=1).max())


_want = {}


def _oracle_scores(oracle, b, scoring):
    """The oracle's score of every pair, one pair per task on the host's cores, remembered by content: the L + 1 batch
    differs from the L batch in one pair, and the forced kernels score the batch the default one did."""
    keys = [(scoring, hashlib.sha1(b.seq(2 * p)).digest(), hashlib.sha1(b.seq(2 * p + 1)).digest()) for p in range(b.n_pairs)]
    todo = sorted({k: p for p, k in enumerate(keys) if k not in _want}.items(), key=lambda kp: -int(b.len[2 * kp[1]]) * int(b.len[2 * kp[1] + 1]))
    if todo:
        with ThreadPoolExecutor(oracle_api._threads()) as ex:
            got = list(ex.map(lambda kp: int(oracle.sw_batch_scored(b.subset(np.array([kp[1]])), scoring)[0]), todo))
        for (k, _), s in zip(todo, got):
            _want[k] = s
    return np.array([_want[k] for k in keys], np.int32)


def _scores(ctx, b, scoring, kernel=agx.SW_KERNEL_AUTO):
    ctx.set_option(agx.OPT_SW_KERNEL, kernel)
    try:
        dev = ctx.sw_batch(b, scoring)
    finally:
        ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
    try:
        dev.launch()
        return dev.scores()
    finally:
        dev.close()


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d pairs differ, first pair %d: got %d, want %d" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def _check(ctx, own, oracle, b, known, scoring, what, every_kernel):
    want = _oracle_scores(oracle, b, scoring)
    for p, top in known:  # the top of the range is provably reached
        assert want[p] == scoring[0] * top, (what, p, want[p], top)
    _same(_scores(ctx, b, scoring), want, what + " auto")
    if every_kernel:  # the same scores from three more representations: unsigned biased halves, signed halves, 32-bit state
        for name in ("SW_KERNEL_PACKED_BIASED", "SW_KERNEL_PACKED_SIGNED", "SW_KERNEL_INT32"):
            _same(_scores(own, b, scoring, getattr(agx, name)), want, what + " " + name)


LL_EDGES = [(s, ls) for s, (ll_at, _) in ref.CASES.items() for ls in ll_at]
LS_EDGES = [s for s, (_, ls_edge) in ref.CASES.items() if ls_edge]
_ids = lambda v: "_".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("scoring,ls", LL_EDGES, ids=_ids)
def test_last_rows_the_rising_cell_takes_and_the_first_it_does_not(ctx, own, oracle, scoring, ls):
    """L = the largest longest-longer-side the rising cell still runs beside ls columns.  The batch at L runs the rising cell
    (KC = 1 or 4 by the scoring), the same batch with ONE more row in its worst pair the plain cell.  The worst pair's copy of
    x ends in y's last rows: score match * ls at offset (L + 63 + 2 + class) |ge|, the largest halves the rule admits."""
    L = ref.last_rising_ll(scoring, ls)
    if L is None:  # (8, -2, -20, -16) beside 2560 columns: the plain cell even at 2560 rows, so that is what runs here
        assert ref.variant(scoring, ls, ls) == ("biased", 0)
        b, known = ll_edge_batch(scoring, ls, ls + 3, ls + 3)
        assert _sides(b) == (ls, ls + 3)
        _check(ctx, own, oracle, b, known, scoring, "%s ls %d, no rising cell" % (scoring, ls), True)
        return
    assert ref.variant(scoring, ls, L)[1] in (1, 4) and ref.variant(scoring, ls, L + 1) == ("biased", 0)
    for longest in (L, L + 1):
        b, known = ll_edge_batch(scoring, ls, L, longest)
        assert _sides(b) == (ls, longest)
        assert known[0] == (0, ls)  # the worst pair: both final newlines, the whole of x matched
        _check(ctx, own, oracle, b, known, scoring, "%s ls %d ll %d (edge %d)" % (scoring, ls, longest, L), longest == L)


@pytest.mark.parametrize("scoring", LS_EDGES, ids=_ids)
def test_last_columns_the_biased_kernel_takes_and_the_first_it_does_not(ctx, own, oracle, scoring):
    """L = the largest longest-shorter-side the biased kernel still takes under this scoring; at L + 1 the signed kernel runs.
    An identical pair L x L reaches match * L, the largest score the rule admits."""
    L = ref.last_biased_ls(scoring)
    assert ref.variant(scoring, L, L)[0] == "biased" and ref.variant(scoring, L + 1, L + 1) == ("signed", 0)
    for ls in (L, L + 1):
        b, known = ls_edge_batch(scoring, ls)
        assert _sides(b) == (ls, ls + 50)
        _check(ctx, own, oracle, b, known, scoring, "%s ls %d (edge %d)" % (scoring, ls, L), ls == L)


@pytest.mark.parametrize("scoring", [(12, -116, -1000, -1000), (12, 0, 0, 0)], ids=_ids)
def test_signed_packed_kernel_at_its_own_extremes(ctx, oracle, scoring):
    """agx_sw_pk_kernel.hip keeps signed 16-bit state: identical 2560-symbol pairs give its largest positive values
    (12 * 2560 = 30 720), the costliest gaps and mismatches its most negative ones."""
    rng = np.random.default_rng(99)
    x = _rand(rng, b"ACGT", 2559) + NL
    seqs = [x, x,
            x, x[:1200] + x[1300:-1] + _rand(rng, b"ACGT", 150) + NL,  # one long deletion
            x[:-1], x[-2::-1],                                          # reversed, no newline
            b"A" * 2560, b"A" * 2560]
    seqs += _filler(rng, 2560)
    b = synth.sw_from_seqs(seqs)
    want = _oracle_scores(oracle, b, scoring)
    assert want[0] == 12 * 2560 and want[3] == 12 * 2560
    _same(_scores(ctx, b, scoring, agx.SW_KERNEL_PACKED_SIGNED), want, "%s signed" % (scoring,))
    _same(_scores(ctx, b, scoring), want, "%s auto" % (scoring,))
