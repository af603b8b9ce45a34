"""The batches whose PairHMM plans tests/golden/phmm_plan_digests.json pins, built the same way in every process.

Each case is small and reaches another branch of create_batch (csrc/agx_phmm.cpp) or of make_plan (csrc/agx_phmm_plan.cpp); the
comment beside it says which, as the trace lines of the recording run showed it.  A case is created plan-only (no device) under
the tuning build's AGX_TRACE_CREATE, which prints a "plan digest main" line (kind, slots, flags, padded cells, the launches and
every wave, table and group record), a "plan digest stripe" line when the batch has a striped plan, an "image digest" line and
a "batch flags" line.  The knobs of the tuning build are read once per process, so the cases are grouped by the environment
they need and every group runs in a child process of its own:     python tests/phmm_plan_cases.py GROUP      (stderr: "CASE
name" ahead of each create's trace lines; stdout: one JSON object, name -> the seven agx_phmm_info fields)

record() runs every group and returns what the fixture holds; tools/record_phmm_plan_digests.py writes it to the JSON."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import accelerating_genomics_amd.synth as synth  # noqa: E402

F64, F64_FMA, F32, PK, GATK = 0, 1, 2, 3, 0x100  # agx.PHMM_*; PK = AGX_PHMM_F32_FMA, the packed float fill
INFO_FIELDS = ("n_pairs", "cells", "padded_cells", "input_bytes", "n_launches", "n_waves", "n_rescued")
# group -> the knobs its child process runs under (AGX_TRACE_CREATE is added to each)
GROUPS = {
    "default": {},
    # From 16 384 pairs with work on, the planner fills waves on one piece of the pair list per host thread (at most one per 8192
    # pairs) and a wave never spans a piece's end: such a batch's plan depends on the thread count, and the default count on the
    # machine.  Every case of that size runs in a group that pins the count.
    "threads_1": {"AGX_HOST_THREADS": "1"},
    "threads_3": {"AGX_HOST_THREADS": "3"},
    "no_trains": {"AGX_PHMM_NO_TRAINS": "1", "AGX_HOST_THREADS": "1"},
    "no_lut": {"AGX_PHMM_NO_LUT": "1"},
    "tail_beta_0": {"AGX_PHMM_TAIL_BETA": "0"},
    "force_c16": {"AGX_PHMM_FORCE_C": "16"},
    "max_classes_2": {"AGX_PHMM_MAX_CLASSES": "2", "AGX_HOST_THREADS": "1"},
}
CORPUS_TIMES = 24  # repeats of the corpus at which its packed plan passes the trains threshold (16 waves per CU of 256)


def _regions_of(b):
    """synth.PhmmBatch -> the list synth.phmm_from_regions takes."""
    tracks = (b.read_bases, b.q_base, b.q_ins, b.q_del, b.q_gcp)
    out = []
    for g in range(b.n_regions):
        reads = [tuple(t[int(b.roff[r]):int(b.roff[r + 1])].tobytes() for t in tracks) for r in range(int(b.rreg[g]), int(b.rreg[g + 1]))]
        haps = [b.hap_bases[int(b.hoff[h]):int(b.hoff[h + 1])].tobytes() for h in range(int(b.hreg[g]), int(b.hreg[g + 1]))]
        out.append((reads, haps))
    return out


def _one_shape():
    return synth.phmm_regions(64, 64, 16, 100, 300, seed=3)


def _corpus(times=1):
    """tests/golden/phmm_10s.in, read as bench.py reads it."""
    with open(os.path.join(ROOT, "tests", "golden", "phmm_10s.in"), "rb") as f:
        b = synth.parse_phmm_text(f.read())
    return synth.phmm_repeat(b, times) if times > 1 else b


def _jitter():
    return synth.phmm_regions(16, 32, 8, 150, 380, seed=83, jitter=100)


def _jitter_big():
    """262 144 pairs from 2048 reads and 4096 haplotypes: enough estimated waves for three kept classes."""
    return synth.phmm_regions(32, 64, 128, 150, 380, seed=85, jitter=100)


def _read(rng, R, qual=b"I"):
    return (synth._ACGT[rng.integers(0, 4, size=R)].tobytes(), qual * R, b"K" * R, b"K" * R, b"+" * R)


def _hap(rng, H):
    return synth._ACGT[rng.integers(0, 4, size=H)].tobytes()


def _sparse():
    """23 pairs whose lengths span a window of 3991 x 1991 cells: the shapes are counted through the hash map."""
    rng = np.random.default_rng(61)
    return synth.phmm_from_regions([([_read(rng, 10), _read(rng, 4000)], [_hap(rng, 10), _hap(rng, 2000), _hap(rng, 300)]),
                                    ([_read(rng, 150)] * 1 + [_read(rng, 90), _read(rng, 151)], [_hap(rng, 280), _hap(rng, 40), _hap(rng, 333)]),
                                    ([_read(rng, 700), _read(rng, 33)], [_hap(rng, 1200), _hap(rng, 64), _hap(rng, 65), _hap(rng, 1999)])])


def _dominant():
    """1280 pairs in regions of 8 reads x 8 haplotypes: three regions of 120 x 260 for every two of 50..150 x 160..260."""
    one = _regions_of(synth.phmm_regions(12, 8, 8, 120, 260, seed=71))
    other = _regions_of(synth.phmm_regions(8, 8, 8, 150, 260, seed=72, jitter=100))
    regions = []
    for k in range(4):
        regions += one[3 * k:3 * k + 3] + other[2 * k:2 * k + 2]
    return synth.phmm_from_regions(regions)


def _long(read_len=0):
    """Ordinary pairs and one region with a haplotype of 2600 bases, beyond 64 lanes x the widest class of every arithmetic
    (2048 double and packed, 2560 float); read_len: a read of that length in the long region."""
    rng = np.random.default_rng(73)
    regions = _regions_of(synth.phmm_regions(2, 6, 4, 100, 300, seed=74))
    reads = [_read(rng, 120), _read(rng, 80)] + ([_read(rng, read_len)] if read_len else [])
    return synth.phmm_from_regions(regions + [(reads, [_hap(rng, 2600), _hap(rng, 250)])])


def _small(R=100):
    return synth.phmm_regions(3, 4, 4, R, R + 100, seed=75)


def _two_shapes():
    """The one-shape batch and one region of another shape behind it: every run but the last pairs."""
    return synth.phmm_from_regions(_regions_of(_one_shape()) + _regions_of(synth.phmm_regions(1, 4, 4, 50, 80, seed=77)))


def _edit(make, track, at, byte):
    def f():
        b = make()
        for t in track:
            getattr(b, t)[at] = byte
        return b
    return f


def _with_empty(what):
    """A region of one shape (4 reads x 4 haplotypes of 50 x 80) and a region whose reads (or haplotypes) are all empty: its pairs
    have output slots and no work."""
    def f():
        rng = np.random.default_rng(76)
        full = _regions_of(synth.phmm_regions(1, 4, 4, 50, 80, seed=77))
        if what == "reads":
            hollow = ([(b"",) * 5, (b"",) * 5], [_hap(rng, 80), _hap(rng, 70), _hap(rng, 60)])
        else:
            hollow = ([_read(rng, 50), _read(rng, 40)], [b"", b"", b""])
        return synth.phmm_from_regions(full + [hollow])
    return f


def _only_empty():
    return synth.phmm_from_regions([([(b"",) * 5], [b"", b""])])


def _shard_whole():
    return synth.phmm_regions(6, 5, 3, 120, 260, seed=78, jitter=40)


def _shard_view():
    """Regions 2..3 of six as agx_phmm_forward_devices hands a shard on: the whole batch's tracks and offsets, region tables that
    start at the shard's first region and keep the caller's absolute read and haplotype numbers."""
    b = _shard_whole()
    return synth.PhmmBatch(b.read_bases, b.q_base, b.q_ins, b.q_del, b.q_gcp, b.roff, b.hap_bases, b.hoff, b.rreg[2:5].copy(), b.hreg[2:5].copy())


def _ladder():
    from tests import phmm_range_cases as rc

    return rc.rescue_ladder("usual")


# (name, group, batch maker, precision)
CASES = [
    # one (R, H) shape: one_shape, file order, no sorts, the dominant-shape rule tiles it (16 lanes x 19 columns packed)
    ("one_shape_f64", "threads_1", _one_shape, F64),
    ("one_shape_f64fma", "threads_1", _one_shape, F64_FMA),
    ("one_shape_f32", "threads_1", _one_shape, F32),
    # ... packed: 8192 estimated waves >= 16 x 256, read trains on the `sure` branch (one plan made)
    ("one_shape_pk", "threads_1", _one_shape, PK),
    ("one_shape_pk_no_trains", "no_trains", _one_shape, PK),
    # not one shape, nearly: both plans are built, the one with trains has fewer padded cells and stays
    ("two_shapes_pk", "threads_1", _two_shapes, PK),
    # the reference's corpus, 7 regions: tail regime (beta 2), consolidation (used > k_max = 1)
    ("corpus_f64", "default", _corpus, F64),
    ("corpus_f32", "default", _corpus, F32),
    ("corpus_pk", "default", _corpus, PK),
    # the same without the tail term: consolidated to the one class it has with the term, the same plan
    ("corpus_f64_beta0", "tail_beta_0", _corpus, F64),
    # 16 columns per lane pinned
    ("corpus_f64_c16", "force_c16", _corpus, F64),
    # no looked-up priors: make_plan is called with exactly the arguments of a packed batch's rescue plan
    ("corpus_f64_no_lut", "no_lut", _corpus, F64),
    # the corpus repeated: beyond the trains threshold, both plans are built and compared by padded cells
    ("corpus_x_pk", "threads_1", lambda: _corpus(CORPUS_TIMES), PK),
    # ... on three pieces: other waves where a piece ends; the one-shape batch loses the trains of the reads a cut parts
    ("corpus_x_pk_threads3", "threads_3", lambda: _corpus(CORPUS_TIMES), PK),
    ("one_shape_pk_threads3", "threads_3", _one_shape, PK),
    # below 16 384 pairs one piece: 1, 3 and all threads give one plan
    ("corpus_x4_pk", "default", lambda: _corpus(4), PK),
    ("corpus_x4_pk_threads1", "threads_1", lambda: _corpus(4), PK),
    ("corpus_x4_pk_threads3", "threads_3", lambda: _corpus(4), PK),
    ("corpus_x_f64", "threads_1", lambda: _corpus(CORPUS_TIMES), F64),
    # reads of 50..150 against haplotypes of 280..380: the dense shape table
    ("jitter_f64", "default", _jitter, F64),
    ("jitter_pk", "default", _jitter, PK),
    # ... without the tail term (the batch is in the tail regime: 587 waves): another class, fewer and longer waves
    ("jitter_pk_beta0", "tail_beta_0", _jitter, PK),
    ("jitter_f64_gatk", "default", _jitter, F64 | GATK),
    ("jitter_pk_gatk", "default", _jitter, PK | GATK),
    # 262 144 pairs: more than 32 768 estimated waves, three classes kept; two under AGX_PHMM_MAX_CLASSES=2
    ("jitter_big_f64", "threads_1", _jitter_big, F64),
    ("jitter_big_f64_2_classes", "max_classes_2", _jitter_big, F64),
    # a window of lengths too wide for the dense table: the hash map
    ("sparse_f64", "default", _sparse, F64),
    ("sparse_pk", "default", _sparse, PK),
    # 60 % of the pairs have one shape: the dominant-shape rule re-tiles them among jittered ones
    ("dominant_f64", "default", _dominant, F64),
    ("dominant_pk", "default", _dominant, PK),
    # a haplotype no class spans: the striped plan beside the main one
    ("long_f64", "default", _long, F64),
    ("long_f32", "default", _long, F32),
    ("long_pk", "default", _long, PK),
    # ... with the GATK prior and a read of 3900 bases: the striped launch divides the prior itself (stripe_mis_div)
    ("long_gatk_f64", "default", lambda: _long(3900), F64 | GATK),
    ("long_gatk_f64_short_read", "default", _long, F64 | GATK),
    # a read base outside ACGTN: no looked-up priors (lut_prior 0), the plain packed cell (fast 0)
    ("not_dna_f64", "default", _edit(_small, ("read_bases",), 5, ord("R")), F64),
    ("not_dna_pk", "default", _edit(_small, ("read_bases",), 5, ord("R")), PK),
    ("plain_f64", "default", _small, F64),
    ("plain_pk", "default", _small, PK),
    # both gap qualities of one row at Phred 0 (`wild`): a batch that would form trains plans without them
    ("wild_pk", "threads_1", _edit(_one_shape, ("q_ins", "q_del"), 17, ord("!")), PK),
    # a gap-continuation quality of Phred 0: the plain packed cell
    ("gcp0_pk", "default", _edit(_small, ("q_gcp",), 5, ord("!")), PK),
    # the longest read on either side of ph_lut_is_ring (R + 2 > 365)
    ("ring_no_f64", "default", lambda: _small(363), F64),
    ("ring_yes_f64", "default", lambda: _small(364), F64),
    # nothing to plan; pairs without work (n_work < n_pairs: not in file order); one cell
    ("empty_no_regions", "default", lambda: synth.phmm_from_regions([]), F64),
    ("empty_only", "default", _only_empty, PK),
    ("empty_reads_pk", "default", _with_empty("reads"), PK),
    ("empty_haps_f64", "default", _with_empty("haps"), F64),
    ("whole_pk", "default", lambda: _regions_batch(_with_empty("reads")(), 0, 1), PK),
    ("one_by_one_f64", "default", lambda: synth.phmm_regions(1, 1, 1, 1, 1, seed=79), F64),
    ("one_by_one_pk", "default", lambda: synth.phmm_regions(1, 1, 1, 1, 1, seed=79), PK),
    # a descriptor narrowed to r_base / h_base: the image and the plan of the same regions passed on their own
    ("shard_view_f64", "default", _shard_view, F64),
    ("shard_alone_f64", "default", lambda: _regions_batch(_shard_whole(), 2, 4), F64),
    ("shard_view_pk", "default", _shard_view, PK),
    ("shard_alone_pk", "default", lambda: _regions_batch(_shard_whole(), 2, 4), PK),
    # tests/phmm_range_cases.py's mismatch ladder across the rescue threshold: packed, and the double plan its rescue pass gets
    ("ladder_pk", "default", _ladder, PK),
    ("ladder_f64_no_lut", "no_lut", _ladder, F64),
]
assert len({c[0] for c in CASES}) == len(CASES) and all(c[1] in GROUPS for c in CASES)


def _regions_batch(b, lo, hi):
    return b.regions(lo, hi)


def child(group, names=None, device=False, run=()):
    """Creates the group's cases (all, or `names`) in this process; device=True: on device 0 instead of plan-only, and the cases
    named in `run` are launched and their results fetched (a packed batch plans its rescue pass at the first underflow)."""
    import accelerating_genomics_amd.api as agx

    infos = {}
    ctx = agx.Context(0) if device else None
    try:
        for name, g, make, prec in CASES:
            if g != group or (names and name not in names):
                continue
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            dev = agx.PhmmBatchDev(ctx, make(), prec)
            try:
                if device and name in run:
                    dev.launch()
                    dev.results()
                info = dev.info()
                infos[name] = {f: int(getattr(info, f)) for f in INFO_FIELDS}
            finally:
                dev.close()
        sys.stderr.write("CASE end\n")
    finally:
        if ctx is not None:
            ctx.close()
    print(json.dumps(infos))


_LINES = {
    "main": r"\[agx_phmm_batch_create\] plan digest main ([0-9a-f]{16})$",
    "stripe": r"\[agx_phmm_batch_create\] plan digest stripe ([0-9a-f]{16})$",
    "rescue": r"\[agx_phmm_batch_create\] plan digest rescue ([0-9a-f]{16})$",
    "image": r"\[agx_phmm_batch_create\] image digest ([0-9a-f]{16})$",
    "flags": r"\[agx_phmm_batch_create\] batch flags (fast \d trains \d lut_prior \d lut_ring \d file_order \d)$",
    "compared": r"\[phmm make_plan kind 3\] read trains: .* -> (with|without)$",
}


def parse(stderr, infos):
    """The trace of one child -> name -> fixture entry."""
    parts = re.split(r"^CASE (\w+)\n", stderr, flags=re.M)[1:]
    out = {}
    for name, text in zip(parts[0::2], parts[1::2]):
        if name == "end":
            continue
        e = {}
        for key, pat in _LINES.items():
            m = re.findall("^" + pat, text, flags=re.M)
            assert len(m) <= 1 and (m or key not in ("main", "image", "flags")), (name, key, text)
            if m:
                e[key] = m[0]
        e["info"] = infos[name]
        out[name] = e
    return out


def run_group(group, lib_path=None, names=None, device=False, run=(), extra_env=None, timeout=600):
    """One child process -> (name -> fixture entry, its whole stderr)."""
    env = dict(os.environ, AGX_TRACE_CREATE="1", **GROUPS[group])
    env.update(extra_env or {})
    env.pop("AGX_LIB_PATH", None)
    if lib_path:
        env["AGX_LIB_PATH"] = os.path.abspath(lib_path)
    argv = [sys.executable, os.path.abspath(__file__), group, "device" if device else "plan", ",".join(names or []), ",".join(run)]
    r = subprocess.run(argv, capture_output=True, timeout=timeout, env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-3000:]
    return parse(err, json.loads(r.stdout.decode())), err


def record(lib_path=None):
    """Every case, plan-only -> what tests/golden/phmm_plan_digests.json holds."""
    out = {}
    for group in GROUPS:
        out.update(run_group(group, lib_path)[0])
    return {c[0]: out[c[0]] for c in CASES}


if __name__ == "__main__":
    _a = sys.argv[1:] + [""] * 4
    child(_a[0], [n for n in _a[2].split(",") if n] or None, _a[1] == "device", tuple(n for n in _a[3].split(",") if n))
