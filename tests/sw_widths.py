"""Shared by tests/test_sw_widths_cpu.py and tests/test_sw_widths_gpu.py: the batches that place a Smith-Waterman pair on a chosen
number of lanes per group, the table of which fill is built for which columns-per-lane class, and the child process that runs
every fill of one class with the class pinned.  No tests here, and no device at import.

Every column-owning fill is a template family with one build per class C (agx_sw.h: AGX_SW_FOR_EACH_CLASS, _WIDE_CLASS,
_STATS_CLASS, _TRACE_CLASS, and the zeros of the cost tables).  AGX_SW_FORCE_C pins C; it exists in the tuning build only and is
read once per process, as AGX_SW_KERNEL is, so every width runs in a child of its own (run_child).  A class that a family does not
have is refused (AGX_E_LIMIT, "no lane tiling fits"), never swapped for another: FAMILIES says which create must succeed.  The
banded fills are not here: their classes follow from the band width, which WIDTHS of tests/sw_fuzz_cases.py walks.

For a class C a pair lands on G = ceil(lx / C) lanes, lx = the side across the lanes (the shorter side of a score batch, the
query of an align batch).  GS = 1, 2, 3, 16, 17, 33, 64: one lane (no arrival), two, three and seventeen (21 and 3 groups to a wave,
idle lanes behind the last), sixteen and sixty-four (the full powers of two), thirty-three (one group and 31 idle lanes).  The
wide classes (80, 120, 160: the byte-compare int32 fill only) run on 1, 2, 3, 17 and 64 lanes, and at 64 lanes on two pairs only:
10 240 x 10 243 cells take the oracle about a second, and no other pair of the sweep is larger.

How a batch reaches a fill: the packed biased fill is the default kernel under the reference's scoring, with column classes
(rising 4) at the wide period C / 2 from 14 columns on and at period four under AGX_SW_PERIOD=4; AGX_SW_RISE=1 / =0 give the
rising cell without column classes and the plain cell, AGX_SW_DNA=0 the general cell in every wave, one N in one pair the general
cell in that pair's wave, of the packed biased fill and of the int32 fill with the coded match alike (the pack kernel decides
that per wave on the device and AGX_SW_DNA is read during the upload: neither prints a trace line and no plan shows it, only the
scores of the wave do);
AGX_OPT_SW_KERNEL picks the packed signed fill and the int32 fill with the coded match, AGX_SW_I32_CLASSIC the int32 fill that
compares bytes, matrix= the int32 fill with the table lookup.  align= / mode= reach the locating and the anchored fill, stats=True
the builds that count (the batch's own fill in GLOBAL, EXTEND and EXTEND_QUERY; the begin pass of LOCAL and FIT, which exists
with a device only -- so a plan made without one cannot show that class, and the GPU test reads it from the begin pass's own trace
lines), cigar=True the traced fill of the spans and the walk (also a batch of its own, made when the CIGARs are fetched).  The
knobs named AGX_SW_RISE, _PERIOD, _DNA and _I32_CLASSIC are read at every create, so a child changes them between batches.

Which classes the rest of the suite reaches: probe() makes plan-only creates on the tuning build under AGX_TRACE_CREATE (tiled
for 256 CUs, one `launch C` line per batch, no AGX_SW_FORCE_C) of batches like those of the family files and of the joint sweep --
up_to_40 (the 0..40 x 0..40 grid), tie_heavy (600 pairs of 1..199) and lane_edges of tests/sw_cigar_cases.py, 2048 pairs of
140..150 x 150..600, 4096 pairs of 32..512, the corpus of tests/sw_fuzz_cases.py for the five unbanded families, single pairs of
1792, 2048 and 2560 columns, 65 536 pairs of 150 x 150; some are those files' own generators, the others are made alike here.
What it found when this file was written (a record, not a contract: it moves with the planner's cost tables and with those
generators): score-only batches launch 4, 6, 10, 28, 32, 38 and 40, under a matrix the same without 38; align batches 4, 6,
10 .. 20, 28, 32, 38, 40; stats batches 4, 6, 10, 14 .. 20, 28, 38; cigar batches 4, 6, 10, 14, 16, 18, 28, 32, 38 -- each the class of
the batch's own fill (the begin pass and the traced fill of the spans are batches made on the device, and smaller ones).  Classes
8, 22, 24, 26, 30, 34 and 36 are launched by none of them in any align, statistics or traced build, twelve of the nineteen classes
by no score-only batch, and the wide classes run at 64 lanes only: before this sweep most of the roughly 250 builds had never
produced a number that was compared with anything.  tests/test_sw_widths_cpu.py repeats the probe and holds only that the
planner alone leaves built classes unreached.

Batches: width_batch(kind, C, G, alphabet) is seeded by (kind, C, G, alphabet) and holds, for every shape of shapes(kind, C, G),
five pairs, and a score batch one pair more, so that its count is odd: under AGX_SW_FORCE_C all pairs of a batch share one
(class, G) bucket, which a packed plan fills two pairs to a group, and the last group then has a vacant half (the all-padding half
and the single-score store of the packed kernels).  The five: one whose only long diagonal ends in the last column of the last lane in the
last row, one ending in the first column of a lane other than the first, a related pair with a two-symbol indel across a lane
boundary, a homopolymer pair (every cell ties: what "smallest row, then smallest column" and the walk's tie order are decided on)
and an unrelated pair; under the plain scoring with final newlines on both sides, one side or none (FORMS of
tests/test_sw_range_gpu.py).  Alphabets: "dna" for the plain scoring (the coded cells run), "acgt" (no newline: the matrix maps
four symbols) under the four-symbol matrix with a zero and a positive off-diagonal entry, "amino" under BLOSUM62 with gaps
-11 / -1.  Every align kind runs all five modes, so GLOBAL, whose span is the whole pair, puts the traced and the counting fill
themselves on the G lanes asked for."""
import collections
import contextlib
import json
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import sw_fuzz_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = b"\n"
FORMS = ((True, True), (True, False), (False, True), (False, False))  # final newline on (x, y), as tests/test_sw_range_gpu.py
GS = (1, 2, 3, 16, 17, 33, 64)
WIDE_GS = (1, 2, 3, 17, 64)
CLASSES = tuple(range(4, 41, 2))         # AGX_SW_FOR_EACH_CLASS
WIDE_CLASSES = (80, 120, 160)            # AGX_SW_FOR_EACH_WIDE_CLASS
STATS_CLASSES = tuple(range(4, 29, 2))   # AGX_SW_FOR_EACH_STATS_CLASS
TRACE_CLASSES = tuple(range(4, 33, 2))   # AGX_SW_FOR_EACH_TRACE_CLASS
WIDTHS = CLASSES + WIDE_CLASSES
CHILD_TIMEOUT = 300  # seconds, as the other child processes of the suite
MODES = fc.MODES
KINDS = ("score", "align", "stats", "cigar")
LIMIT = {"score": 10240, "align": agx.SW_ALIGN_MAX_QUERY_LEN, "stats": agx.SW_STATS_MAX_QUERY_LEN, "cigar": agx.SW_CIGAR_MAX_QUERY_LEN}
PAIR_KINDS = ("end", "lane", "indel", "homo", "unrelated")
ALPHABETS = {"dna": (b"AC", b"GT", b"ACGT"), "acgt": (b"AC", b"GT", b"ACGT"), "amino": (b"ARNDCQEGHI", b"LKMFPSTWYV", synth.AMINO)}
SCORERS = {"plain": "dna", "four": "acgt", "blosum62": "amino"}  # scorer -> the alphabet of its batches
KERNELS = {"auto": agx.SW_KERNEL_AUTO, "i32": agx.SW_KERNEL_INT32, "pk1": agx.SW_KERNEL_PACKED_SIGNED, "pk2": agx.SW_KERNEL_PACKED_BIASED}

# Shapes that found something, kept by name: name -> (fill, C, G).  Both test files run them beside the sweep.
#   lone_newline_coded_i32: a shorter side that is one newline against a longer side that ends with one.  The pack kernel strips
#   both sentinels and marks the pair (bit 13 of its record); the two newlines still align, one match.  agx_sw_i32d_kernel.hip
#   dropped that match whenever a stripped side was empty and answered 0 -- since the kernel was added; the packed biased fill,
#   which reads the same records, always had it.  Every class, one lane: the pairs of shape 1 x 1 .. 1 x 4 with both newlines.
REGRESSIONS = {"lone_newline_coded_i32": ("i32 coded", 4, 1)}

# kind: which batches; classes: the builds that exist; family, rising: what AGX_TRACE_CREATE prints for the create; kernel: the
# option (a context) or AGX_SW_KERNEL (no device); env: knobs read at every create; scorer: plain, four or blosum62; twin: the
# batch with one N; mode, what: of an align batch
Fill = collections.namedtuple("Fill", "kind classes family rising kernel env scorer twin mode what")


def _fills():
    out = collections.OrderedDict()

    def score(name, classes, family, rising, kernel="auto", env=None, scorer="plain", twin=False):
        out[name] = Fill("score", classes, family, rising, kernel, env or {}, scorer, twin, fc.LOCAL, 0)

    score("pk2 period 4", CLASSES, 2, 4, env={"AGX_SW_PERIOD": "4"})
    score("pk2 wide period", tuple(c for c in CLASSES if c >= 14), 2, 4)
    score("pk2 rising 1", CLASSES, 2, 1, env={"AGX_SW_RISE": "1"})
    score("pk2 rising 0", CLASSES, 2, 0, env={"AGX_SW_RISE": "0"})
    score("pk2 general cell", CLASSES, 2, 4, env={"AGX_SW_DNA": "0"})
    score("pk2 one N", CLASSES, 2, 4, twin=True)
    score("pk1", CLASSES, 1, 0, kernel="pk1")
    score("i32 coded", CLASSES, 3, 0, kernel="i32")
    score("i32 coded one N", CLASSES, 3, 0, kernel="i32", twin=True)
    score("i32 bytes", CLASSES + WIDE_CLASSES, 0, 0, kernel="i32", env={"AGX_SW_I32_CLASSIC": "1"})
    score("i32 four", CLASSES, 0, 0, scorer="four")
    score("i32 blosum62", CLASSES, 0, 0, scorer="blosum62")
    for mode in MODES:
        for scorer in SCORERS:
            fam = 4 if mode == fc.LOCAL else 5
            for what, name in ((fc.ENDS, "ends"), (fc.SPANS, "spans")):
                out["align %s %s %s" % (fc.MODE_NAMES[mode], scorer, name)] = Fill("align", CLASSES, fam, 0, "auto", {}, scorer, False, mode, what)
            out["stats %s %s" % (fc.MODE_NAMES[mode], scorer)] = Fill("stats", STATS_CLASSES, fam, 0, "auto", {}, scorer, False, mode, fc.SPANS)
            out["cigar %s %s" % (fc.MODE_NAMES[mode], scorer)] = Fill("cigar", TRACE_CLASSES, fam, 0, "auto", {}, scorer, False, mode, fc.SPANS)
    return out


FAMILIES = _fills()

def families(C):
    return [name for name, f in FAMILIES.items() if C in f.classes]


def gs(C):
    return WIDE_GS if C in WIDE_CLASSES else GS


def legs(C):
    """the (fill, G) legs of class C: what the child runs and the parent expects back, nothing left out"""
    return [(name, G) for G in gs(C) for name in families(C) if shapes(FAMILIES[name].kind, C, G)]


def shapes(kind, C, G):
    """(lx, ly) -- across the lanes, rows -- of the pairs that sit on G lanes of C columns, the smallest at which a fill can go
    wrong: the last lane full or holding one column; rows fewer than, equal to and beyond the skew of G - 1 steps, the four tail
    lengths of the quad loop (steps = rows + G - 1); a score batch's longer side cannot be shorter than its columns."""
    across = [lx for lx in sorted({(G - 1) * C + 1, G * C}) if lx <= LIMIT[kind]]
    if kind == "score":
        if C in WIDE_CLASSES and G == 64:
            return [(G * C, G * C + 3), ((G - 1) * C + 1, (G - 1) * C + 2)]
        return [(lx, lx + d) for lx in across for d in sorted({0, 1, 2, 3, G})]
    rows = sorted({r for r in (1, 2, G - 1, G, 2 * G + 3, 2 * G + 4, 2 * G + 5, 2 * G + 6) if r >= 1})
    return [(lx, r) for lx in across for r in rows]


def _rand(rng, alphabet, n):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def _pair(rng, which, L, R, C, G, alphabet):
    """-> (a of L symbols across the lanes, t of R rows).  a is drawn from one half of the alphabet and what is unrelated in t from
    the other, so that the copy of a is the only long diagonal."""
    ax, ay, full = ALPHABETS[alphabet]
    if which == "homo":
        return full[:1] * L, full[:1] * R
    if which == "unrelated":
        return _rand(rng, full, L), _rand(rng, full, R)
    a = _rand(rng, ax, L)
    lane = max(1, G // 2)
    edge = lane * C if G > 1 else max(L // 2, 1)  # the first column of a lane other than the first (one lane: its middle)
    if which == "end":  # ... ends in a's last column and t's last row
        m = min(L, R)
        return a, _rand(rng, ay, R - m) + a[L - m:]
    if which == "lane":  # ... ends in column `edge`, one row above the last where there is one
        k = min(edge, L - 1)
        m = min(k + 1, max(R - 1, 1))
        post = 1 if R - m >= 1 else 0
        return a, _rand(rng, ay, R - m - post) + a[k + 1 - m:k + 1] + _rand(rng, ay, post)
    p = min(edge, L - 1)  # "indel": two symbols either side of the boundary dropped, or two foreign ones put in there
    mut = a[:max(p - 1, 0)] + a[p + 1:] if (L + R) % 2 else a[:p] + _rand(rng, ay, 2) + a[p:]
    q = max(p - 1, 0)
    if len(mut) >= R:  # the window of R rows around the boundary
        start = min(max(q - R // 2, 0), len(mut) - R)
        return a, mut[start:start + R]
    return a, _rand(rng, ay, R - len(mut)) + mut


def width_seqs(kind, C, G, alphabet="dna"):
    rng = np.random.default_rng([KINDS.index(kind), C, G, list(ALPHABETS).index(alphabet)])
    seqs = []
    few = kind == "score" and C in WIDE_CLASSES and G == 64
    for si, (L, R) in enumerate(shapes(kind, C, G)):
        for ki, which in enumerate(PAIR_KINDS[si:si + 1] if few else PAIR_KINDS):
            a, t = _pair(rng, which, L, R, C, G, alphabet)
            if alphabet == "dna":  # (a newline is no symbol of a matrix)
                nla, nlt = FORMS[(si % 2) * 3] if which == "end" else FORMS[(si + ki) % 4]
                a, t = (a[:-1] + NL if nla else a), (t[:-1] + NL if nlt else t)
            assert len(a) == L and len(t) == R
            seqs += [t, a] if kind == "score" and (si + ki) % 2 else [a, t]
    if kind == "score" and not few:
        # one pair more, so that the batch's count is odd: under AGX_SW_FORCE_C all its pairs share one (class, G) bucket, which the
        # packed plans fill two pairs to a group -- the last group then has a vacant half (all padding, a single-score store)
        a, t = _pair(rng, "end", L, R, C, G, alphabet)
        seqs += [a[:-1] + NL, t[:-1] + NL] if alphabet == "dna" else [a, t]
    return seqs


_batches = {}


def width_batch(kind, C, G, alphabet="dna", twin=False):
    """The batch of (kind, C, G): made once per process, shared and left unchanged.  twin: one N in the middle of the first pair's
    first sequence -- a fifth symbol, which takes that pair's wave of the packed biased fill off the coded cell."""
    kind = "align" if kind in ("stats", "cigar") and shapes(kind, C, G) == shapes("align", C, G) else kind  # (the same pairs)
    key = (kind, C, G, alphabet, twin)
    if key not in _batches:
        seqs = width_seqs(kind, C, G, alphabet)
        if twin:
            seqs[0] = seqs[0][:len(seqs[0]) // 2] + b"N" + seqs[0][len(seqs[0]) // 2 + 1:]
        _batches[key] = synth.sw_from_seqs(seqs)
    return _batches[key]


_matrices = {}


def matrix(scorer):
    """blosum62: synth.BLOSUM62 over synth.AMINO, gaps -11 / -1; four: the table of tests/sw_cigar_cases.py's four_symbols
    (a zero and a positive entry off the diagonal: a mismatch can tie with or beat a match elsewhere)"""
    if scorer == "plain":
        return None
    if scorer not in _matrices:
        _matrices[scorer] = (agx.SwMatrix.build(synth.AMINO, synth.BLOSUM62, -11, -1) if scorer == "blosum62" else
                             agx.SwMatrix.build(b"ACGT", [[2, 1, 0, -3], [1, 2, -3, 0], [0, -3, 2, 1], [-3, 0, 1, 2]], -2, -1))
    return _matrices[scorer]


def kw_of(fill):
    """the keyword arguments of Context.sw_batch / api.SwBatch for a fill"""
    kw = {}
    if fill.scorer != "plain":
        kw["matrix"] = matrix(fill.scorer)
    if fill.kind == "score":
        return kw
    kw["mode"] = fill.mode
    if fill.kind == "align":
        kw["align"] = fill.what
    else:
        kw[fill.kind] = True
    return kw


def batch_of(name, C, G):
    f = FAMILIES[name]
    return width_batch(f.kind, C, G, SCORERS[f.scorer], f.twin)


# ---- the yardsticks: the oracle for scores, the by-definition checkers for everything else, over the host's cores


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


_scores = {}


def oracle_scores(orc, b, scorer):
    """The oracle's score of every pair (sw_batch, row-major Gotoh under the reference's scoring; sw_batch_matrix), one pair per
    task, remembered by content: a twin differs from its batch in one pair."""
    m = matrix(scorer)
    keys = [(scorer, b.seq(2 * p), b.seq(2 * p + 1)) for p in range(b.n_pairs)]
    todo = sorted({k: p for p, k in enumerate(keys) if k not in _scores}.items(), key=lambda kp: -len(kp[0][1]) * len(kp[0][2]))

    def one(kp):
        sub = b.subset(np.array([kp[1]]))
        return int((orc.sw_batch(sub, 1) if m is None else orc.sw_batch_matrix(sub, m))[0])

    if todo:
        with ThreadPoolExecutor(_threads()) as ex:
            for (k, _), s in zip(todo, list(ex.map(one, todo))):
                _scores[k] = s
    return np.array([_scores[k] for k in keys], np.int32)


_refs = {}


def load_checkers():
    """compile and load the five by-definition checkers of the unbanded families now, before any thread uses one"""
    from tests import sw_align_ref, sw_cigar_ref, sw_matrix_align_ref, sw_modes_ref, sw_stats_ref

    for m in (sw_align_ref, sw_cigar_ref, sw_matrix_align_ref, sw_modes_ref, sw_stats_ref):
        m.load()


def reference(name, C, G):
    """sw_fuzz_cases.reference of an align, stats or cigar fill's batch, once per process.  A large batch goes through it in
    slices over the host's cores.  A stats or cigar fill's answer is what sw_stats_ref.expected / sw_cigar_ref.expected make it
    of, step by step -- the SPANS hits of the align checkers, then the counts or the CIGARs of those hits -- with the hits taken
    from the align fill's reference where that was computed over the same batch."""
    from tests import sw_cigar_ref, sw_stats_ref

    f = FAMILIES[name]
    key = (f.kind, f.scorer, f.mode, f.what, C, G)
    if key in _refs:
        return _refs[key]
    b, kw = batch_of(name, C, G), kw_of(f)
    if "matrix" not in kw:
        kw["scoring"] = None
    if f.kind in ("stats", "cigar"):
        spans = "align %s %s spans" % (fc.MODE_NAMES[f.mode], f.scorer)
        h = reference(spans, C, G)["hits"] if batch_of(spans, C, G) is b else sw_stats_ref.hits(b, f.mode, None, kw.get("matrix"))
        if f.kind == "stats":
            out = {"hits": h, "stats": sw_stats_ref.stats(b, h, None, kw.get("matrix"))[0]}
        else:
            out = dict(zip(("op_off", "ops"), sw_cigar_ref.cigars(b, h, None, kw.get("matrix"))), hits=h)
    else:
        cells = int((b.len[0::2].astype(np.int64) * b.len[1::2]).sum())
        t = max(1, min(_threads(), b.n_pairs // 4)) if cells > 4000000 else 1
        if t == 1:
            out = fc.reference(b, kw)
        else:
            cuts = np.linspace(0, b.n_pairs, t + 1).astype(np.int64)
            with ThreadPoolExecutor(t) as ex:
                parts = list(ex.map(lambda k: fc.reference(b.subset(np.arange(cuts[k], cuts[k + 1])), kw), range(t)))
            out = {"hits": np.concatenate([p["hits"] for p in parts])}
    _refs[key] = out
    return out


# ---- the child's own trace lines


_case = [0]


def mark(name):
    """"CASE n name" on the process's own stderr, ahead of a leg's creates, as tests/sw_period_cases.py does: the library prints
    its AGX_TRACE_CREATE lines there, unbuffered, and the parent cuts what it captured at these markers (run_child) -- so the
    message of a child that died ends with the leg it was running and the library's last lines.  -> n"""
    _case[0] += 1
    sys.stderr.flush()
    os.write(2, ("CASE %d %s\n" % (_case[0], name)).encode())
    return _case[0]


def parse(text):
    """-> what the creates of one leg said: {"families": [[F, R], ...], "classes": the C of every `launch C` line, "period":
    [[run, of], ...], "groups": [[groups, vacant halves], ...] per create}; the first family is the leg's own create, the others
    the batches it made for its spans"""
    classes = set()
    for m in re.finditer(r"launch C((?: \d+)+| none)", text):
        classes |= {int(c) for c in m.group(1).split() if c != "none"}
    return {"families": [[int(f), int(r)] for f, r in re.findall(r"family (\d+) rising (\d+)", text)], "classes": sorted(classes),
            "period": [[int(p), int(q)] for p, q in re.findall(r"class period (\d+) of (\d+)", text)],
            "groups": [[int(g), int(v)] for g, v in re.findall(r"(\d+) groups, (\d+) vacant halves", text)]}


def cut(stderr):
    """-> {n: the text between the marker CASE n and the next marker}"""
    parts = re.split(r"^CASE (\d+) [^\n]*\n", stderr, flags=re.M)
    return {int(parts[k]): parts[k + 1] for k in range(1, len(parts) - 1, 2)}


@contextlib.contextmanager
def _env(knobs):
    for k, v in knobs.items():
        os.environ[k] = v
    try:
        yield
    finally:
        for k in knobs:
            del os.environ[k]


def _info(dev):
    i = dev.info()
    return {"n_waves": i.n_waves, "n_launches": i.n_launches, "padded_cells": i.padded_cells}


def _where(d):
    return None if d is None else "%s of pair %d: got %s, want %s" % d


def run_leg(ctx, own, orc, name, C, G, trace=False):
    """One fill on one batch: created, launched twice, fetched twice, compared exactly -> a record.  own: the context whose kernel
    option is changed (the default one never has it changed).  trace: a marker goes ahead of the leg ("case" in the record)."""
    f = FAMILIES[name]
    b, kw = batch_of(name, C, G), kw_of(f)
    rec = {"where": "G%d" % G, "leg": name, "n_pairs": b.n_pairs}
    if trace:
        rec["case"] = mark("%s G%d" % (name, G))
    t0 = time.perf_counter()
    with _env(f.env):
        if f.kind == "score":
            c = own if f.kernel != "auto" else ctx
            c.set_option(agx.OPT_SW_KERNEL, KERNELS[f.kernel])
            try:
                dev = c.sw_batch(b, **kw)
            finally:
                c.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
            try:
                rec.update(_info(dev))
                dev.launch()
                got = dev.scores()
                dev.launch()
                again = dev.scores()
            finally:
                dev.close()
            want = oracle_scores(orc, b, f.scorer)
            bad = np.nonzero(got != want)[0]
            rec["differs"] = None if not bad.size else "score of pair %d (%d x %d): got %d, want %d; %d pairs differ" % (
                bad[0], b.len[2 * bad[0]], b.len[2 * bad[0] + 1], got[bad[0]], want[bad[0]], bad.size)
            rec["relaunch_differs"] = None if np.array_equal(got, again) else "scores"
            rec["scores"] = got.tolist()
        else:
            dev = ctx.sw_batch(b, **kw)
            try:
                rec.update(_info(dev))
                dev.launch()
                got = fc._collect(dev, kw)
                dev.launch()
                again = fc._collect(dev, kw)
            finally:
                dev.close()
            rec["differs"] = _where(fc.differ(got, reference(name, C, G)))
            rec["relaunch_differs"] = _where(fc.differ(again, got))
            if f.kind == "cigar" and rec["differs"] is None:
                p = fc.path_check(b, dict(kw, scoring=None), got)
                rec["differs"] = None if p < 0 else "the CIGAR of pair %d fails the path checks" % p
    rec["seconds"] = round(time.perf_counter() - t0, 4)
    return rec


def gpu_width(C):
    """every built fill of class C on every G, on the device -> records"""
    from tests import oracle_api

    orc = oracle_api.load()
    load_checkers()
    with agx.Context(0) as ctx, agx.Context(0) as own:
        return [run_leg(ctx, own, orc, name, C, G, True) for name, G in legs(C)]


def plan_leg(name, C, G):
    """the plan-only create of one fill on one batch -> a record; "error": the AgxError code where the create is refused"""
    f = FAMILIES[name]
    b, kw = batch_of(name, C, G), kw_of(f)
    rec = {"where": "G%d" % G, "leg": name, "n_pairs": b.n_pairs, "error": None, "case": mark("%s G%d" % (name, G))}
    with _env(f.env):
        try:
            dev = agx.SwBatch(None, b, **kw)
            rec.update(_info(dev))
            dev.close()
        except agx.AgxError as e:
            rec["error"] = e.code
    return rec


def plan_width(C, kernel="auto"):
    """Plans only (no device): every fill that the kernel choice `kernel` (this process's AGX_SW_KERNEL) can reach, built for
    class C or not, on every G of GS -> records"""
    return [plan_leg(name, C, G) for G in (GS if kernel != "i32" else sorted(set(GS) | set(WIDE_GS)))
            for name, f in FAMILIES.items() if f.kernel == kernel and shapes(f.kind, C, G)]


PROBE_KINDS = ("score", "matrix", "align", "stats", "cigar")


def probe():
    """Which classes the planner gives batches like those of the rest of the suite (the module docstring lists them), by kind of
    create: plan-only creates without AGX_SW_FORCE_C -> records {"kind", "case"}; reached() sums them up.  A create that a limit
    or a planted byte refuses is skipped: it launches nothing."""
    from tests import sw_cigar_cases as cc

    rng = np.random.default_rng(7)
    mid = []
    for _ in range(2048):
        mid += [_rand(rng, b"ACGT", int(rng.integers(140, 151))), _rand(rng, b"ACGT", int(rng.integers(150, 601)))]
    batches = [(cc.up_to_40(), None), (cc.tie_heavy(), None), (cc.lane_edges(), None), (synth.sw_from_seqs(mid), None),
               (synth.sw_pairs(4096, 32, 512, seed=85, related_frac=0.5), None), (synth.sw_pairs(65536, 150, 150, seed=86, related_frac=0.25), None)]
    batches += [(synth.sw_from_seqs([_rand(rng, b"ACGT", n), _rand(rng, b"ACGT", n + 7)]), None) for n in (1792, 2048, 2560)]
    for fam in fc.FAMILIES[:5]:
        batches += [(c.batch, c.kw) for c in fc.corpus(fam)]
    four = matrix("four")
    out = []
    for b, own in batches:
        if own is not None:
            kws = [("cigar" if own.get("cigar") else "stats" if own.get("stats") else "align", own)]
        else:
            kws = [("score", {}), ("matrix", {"matrix": four})]
            for mode in (fc.LOCAL, fc.GLOBAL):
                for m in ({}, {"matrix": four}):
                    kws += [("align", dict(m, align=fc.SPANS, mode=mode)), ("stats", dict(m, stats=True, mode=mode)), ("cigar", dict(m, cigar=True, mode=mode))]
        for kind, kw in kws:
            n = mark(kind)
            try:
                agx.SwBatch(None, b, **kw).close()
            except agx.AgxError as e:
                assert e.code in (agx.E_LIMIT, agx.E_SYMBOL), e
                continue
            out.append({"kind": kind, "case": n})
    return out


def reached(recs):
    """-> {kind: sorted classes} of probe()'s records as run_child returns them"""
    return {k: sorted({c for r in recs if r["kind"] == k for c in r["classes"]}) for k in PROBE_KINDS}


CHILD = """
import json, sys
sys.path.insert(0, %r)
import accelerating_genomics_amd.api as agx
from tests import sw_widths as sw
assert agx.LIB_PATH.endswith("libagx_tuning.so"), agx.LIB_PATH
mode, C = sys.argv[1], int(sys.argv[2])
print("RESULT " + json.dumps(sw.gpu_width(C) if mode == "gpu" else sw.probe() if mode == "probe" else sw.plan_width(C, mode)))
""" % ROOT


class ChildDied(Exception):
    pass


def run_child(mode, C):
    """One fresh process with AGX_SW_FORCE_C = C and AGX_TRACE_CREATE; mode "gpu", or the AGX_SW_KERNEL of a plan-only child
    ("auto": none), or "probe" (no AGX_SW_FORCE_C: probe()) -> its records, each with what parse() reads from the child's trace
    lines between the record's marker and the next.  ChildDied: it ended by a signal, at its time limit or without a result (the
    message carries its last output: the marker of the leg it was in and the library's last lines)."""
    env = dict(os.environ, AGX_TRACE_CREATE="1")
    env.pop("AGX_LIB_PATH", None)
    if mode != "probe":
        env["AGX_SW_FORCE_C"] = str(C)
    for k in ("AGX_SW_KERNEL", "AGX_SW_RISE", "AGX_SW_PERIOD", "AGX_SW_DNA", "AGX_SW_I32_CLASSIC"):
        env.pop(k, None)
    if mode not in ("gpu", "auto", "probe"):
        env["AGX_SW_KERNEL"] = mode
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, mode, str(C)], capture_output=True, timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired as e:
        raise ChildDied("width %d: no result within %d s\n%s" % (C, CHILD_TIMEOUT, ((e.stdout or b"") + (e.stderr or b"")).decode(errors="replace")[-2000:]))
    lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or len(lines) != 1:
        raise ChildDied("width %d: exit status %d\n%s" % (C, r.returncode, (r.stdout + r.stderr).decode(errors="replace")[-3000:]))
    recs, said = json.loads(lines[0][len("RESULT "):]), cut(r.stderr.decode(errors="replace"))
    for rec in recs:
        rec.update(parse(said[rec.pop("case")]))
    return recs


def waves(fill, n_pairs, G):
    """Waves of n_pairs pairs that all sit on G lanes: 64 // G groups to a wave, two pairs to a group in the packed plans
    (families 1, 2, 3)."""
    groups = -(-n_pairs // 2) if fill.family in (1, 2, 3) else n_pairs
    return -(-groups // (64 // G))
