"""The batches whose host-made plans tests/golden/sw_plan_digests.json pins, built the same way in every process.

Each case is small and reaches another branch of agx_sw_host::create_batch (csrc/agx_sw.cpp); the comment beside it says which, as
the trace lines of the recording run showed it.  A case is created plan-only (no device) under the tuning build's
AGX_TRACE_CREATE, whose "plan digest" line is a hash of the kernel choice, the launches and every wave and group record.  The
knobs of the tuning build are read once per process, so the cases are grouped by the environment they need and every group
runs in a child process of its own:     python tests/sw_plan_cases.py GROUP      (stderr: "CASE name" ahead of each create's
trace lines; stdout: one JSON object, name -> the six agx_sw_info fields)

record() runs every group and returns what the fixture holds; tools/record_sw_plan_digests.py writes it to the JSON."""
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

REF = (1, -1, -3, -1)  # the reference's scoring
INFO_FIELDS = ("n_pairs", "cells", "padded_cells", "input_bytes", "n_launches", "n_waves")
# group -> the knobs its child process runs under (AGX_TRACE_CREATE is added to each)
GROUPS = {
    "default": {},
    "tail_beta_0": {"AGX_SW_TAIL_BETA": "0"},  # tail_beta_override() reads this one
    "kernel_i32": {"AGX_SW_KERNEL": "i32"},
    "force_c38": {"AGX_SW_FORCE_C": "38"},
    "threads_1": {"AGX_HOST_THREADS": "1"},
    "threads_3": {"AGX_HOST_THREADS": "3"},
}


def _from_lens(la, lb, seed):
    """Pairs of the given lengths over ACGT, no newline."""
    lens = np.empty(2 * len(la), np.uint32)
    lens[0::2], lens[1::2] = la, lb
    off = np.zeros(lens.size, np.uint64)
    if lens.size > 1:
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(lens.sum()))]
    return synth.SWBatch(bases, off, lens)


def _dominant():
    """4096 pairs, about 60 % of them 100 x 200, the rest 32..512, interleaved at random: the stride sample meets the shape."""
    rng = np.random.default_rng(41)
    la, lb = rng.integers(32, 513, size=4096), rng.integers(32, 513, size=4096)
    dom = rng.random(4096) < 0.6
    la[dom], lb[dom] = 100, 200
    return _from_lens(la, lb, 42)


def _with_filler(extra, seed):
    """64 filler pairs of 32..64 and the sequences of `extra` behind them."""
    f = synth.sw_pairs(64, 32, 64, seed=seed, newline=False)
    return synth.sw_from_seqs([f.seq(k) for k in range(128)] + list(extra))


def _period_wave150():
    from tests import sw_period_cases as pc

    return synth.sw_from_seqs(pc._wave150(np.random.default_rng(83), 32, False))


def _mixed(n, seed=11):
    return lambda: synth.sw_pairs(n, 32, 512, seed=seed)


def _blosum():
    import accelerating_genomics_amd.api as agx

    return agx.SwMatrix.build(synth.AMINO, synth.BLOSUM62, -11, -1)


def _align_cases():
    out = []
    for what, wname in ((1, "ends"), (2, "spans")):
        for mode, mname in ((0, "local"), (1, "global"), (2, "fit"), (3, "extend")):
            # family 4 (LOCAL: the locating fill) or 5 (the anchored fill), the first sequence across the lanes; tail regime
            out.append(("align_%s_%s" % (wname, mname), "default", lambda: synth.sw_pairs(200, 32, 300, seed=21), dict(align=what, mode=mode)))
    return out


# (name, group, batch maker, keyword arguments of agx.SwBatch beyond the batch) -- "matrix": True stands for BLOSUM62 -11/-1
CASES = [
    # family 2 rising 4, uniform rule: file order, one launch, no tiling pass; 256 waves, staged priority off (plan only)
    ("uniform_1024", "default", lambda: synth.sw_pairs(1024, 150, 150, seed=1, newline=False), {}),
    # one pair short of the uniform rule: host planner, tail regime (beta 10), one class already
    ("uniform_1023", "default", lambda: synth.sw_pairs(1023, 150, 150, seed=1, newline=False), {}),
    # host planner, tail regime (beta 10) and consolidation to one class
    ("mixed_300", "default", _mixed(300), {}),
    # the same under AGX_SW_TAIL_BETA=0: no tail term, consolidation only
    ("mixed_300_beta0", "tail_beta_0", _mixed(300), {}),
    # 16 000 pairs: tail regime and consolidation (used > k_max)
    ("mixed_16000", "default", _mixed(16000, 12), {}),
    # 20 000 pairs: tail regime (beta 6), then 2052 estimated waves: the one-launch kernel keeps every class (k_max = all of them)
    ("mixed_20000", "default", _mixed(20000), {}),
    ("mixed_20000_threads1", "threads_1", _mixed(20000), {}),
    ("mixed_20000_threads3", "threads_3", _mixed(20000), {}),
    # the dominant-shape rule re-tiles the 100 x 200 pairs (sample votes > 0, count * 2 >= n_pairs)
    ("dominant_4096", "default", _dominant, {}),
    # nothing to plan: no waves, no launch
    ("empty_0_pairs", "default", lambda: synth.sw_from_seqs([]), {}),
    ("empty_sides_only", "default", lambda: synth.sw_from_seqs([b"", b"ACGT", b"ACGT", b"", b"", b""] * 3), {}),
    ("empty_side_and_1x1", "default", lambda: synth.sw_from_seqs([b"", b"ACGT", b"A", b"C"]), {}),
    # shorter side 2560: still the packed biased fill (family 2); 2561: classic int32 (family 0) and a wide class
    ("short_2560", "default", lambda: _with_filler([b"A" * 2560, b"C" * 2600], 31), {}),
    ("short_2561", "default", lambda: _with_filler([b"A" * 2561, b"C" * 2600], 31), {}),
    # int32 asked for: family 3 (the packed plan in 32-bit state) while delta < 128, classic family 0 from delta = 128
    ("i32_coded", "kernel_i32", lambda: _with_filler([], 32), {}),
    ("i32_delta_128", "kernel_i32", lambda: _with_filler([], 32), dict(scoring=(12, -116, -10, -3))),
    # the biased range rule fails beyond 2556 columns under this scoring: family 1
    ("signed_2558", "default", lambda: _with_filler([b"A" * 2558, b"C" * 2558], 33), dict(scoring=(12, -4, -10, -3))),
    # rising 4 (column classes), 1 (mismatch + |gf| - 3 |ge| < 0) and 0 (a longer side beyond the rising rule's edge, 1824)
    ("rising_4", "default", lambda: _with_filler([], 34), {}),
    ("rising_1", "default", lambda: _with_filler([], 34), dict(scoring=(1, -2, -3, -1))),
    ("rising_0", "default", lambda: _with_filler([b"A" * 40, b"C" * 1825], 34), dict(scoring=(8, -2, -20, -16))),
    # 38 columns per lane pinned: class period 19 of 19, the wide kernel
    ("period_19", "force_c38", _period_wave150, {}),
    # substitution matrix: family 0 without wide classes, tail regime, consolidation to one class
    ("matrix_500", "default", lambda: synth.protein_pairs(500, 20, 400, seed=51, related_frac=0.0), dict(matrix=True)),
] + _align_cases() + [
    # 20 000 pairs, one to a lane group: enough waves for more than one kept class, every class its own launch
    ("align_ends_local_20000", "default", _mixed(20000), dict(align=1)),
    # stats == 2 (GLOBAL: the batch's own fill is the stats build): the stats cost table, fewer classes
    ("stats_global", "default", lambda: synth.sw_pairs(200, 32, 300, seed=22), dict(mode=1, stats=True)),
    # cigar == 1: a SPANS batch with the cigar builds' query limit (cigar == 2 is made per chunk on a device only)
    ("cigar_fit", "default", lambda: synth.sw_pairs(200, 32, 300, seed=23), dict(mode=2, cigar=True)),
    ("align_matrix_ends_local", "default", lambda: synth.protein_pairs(200, 20, 300, seed=52, related_frac=0.0), dict(matrix=True, align=1)),
]
assert len({c[0] for c in CASES}) == len(CASES) and all(c[1] in GROUPS for c in CASES)


def create(agx, ctx, name):
    """The named case as an agx.SwBatch on ctx (None: plan only)."""
    _, _, make, kw = next(c for c in CASES if c[0] == name)
    kw = dict(kw)
    if kw.pop("matrix", False):
        kw["matrix"] = _blosum()
    return agx.SwBatch(ctx, make(), **kw)


def child(group, names=None, device=False, cases=None, create=None):
    """Creates the group's cases (all, or `names`) in this process; device=True: on device 0 instead of plan-only.
    cases, create: another module's list of cases (name and group first) and its create, for CASES and create() here."""
    import accelerating_genomics_amd.api as agx

    cases, create = cases or CASES, create or globals()["create"]

    infos = {}
    ctx = agx.Context(0) if device else None
    try:
        for name, g in (c[:2] for c in cases):
            if g != group or (names and name not in names):
                continue
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            dev = create(agx, ctx, name)
            try:
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
    "digest": r"plan digest(?: ([0-9a-f]{16})|: (on device))$",
    "family": r"(family \d+ rising \d+): longest",
    "period": r"(class period \d+ of \d+)$",
    "staged": r"(staged priority \d+): ",
}


def parse(stderr, infos, lines=None, prefix="agx_sw_batch_create", required=("digest", "family")):
    """The trace of one child -> name -> fixture entry.  lines, prefix, required: another create's trace lines for the ones here."""
    parts = re.split(r"^CASE (\w+)\n", stderr, flags=re.M)[1:]
    out = {}
    for name, text in zip(parts[0::2], parts[1::2]):
        if name == "end":
            continue
        e = {}
        for key, pat in (lines or _LINES).items():
            m = re.findall(r"^\[%s\] " % prefix + pat, text, flags=re.M)
            if key in required:
                assert len(m) == 1, (name, key, text)
            if m:
                assert len(m) == 1, (name, key, text)
                e[key] = (m[0][0] or m[0][1]) if isinstance(m[0], tuple) else m[0]
        e["info"] = infos[name]
        out[name] = e
    return out


def run_group(group, lib_path=None, names=None, device=False, extra_env=None, script=None, parse=parse):
    """One child process -> (name -> fixture entry, its whole stderr).  script, parse: another module of cases run as this one is."""
    env = dict(os.environ, AGX_TRACE_CREATE="1", **GROUPS[group])
    env.update(extra_env or {})
    env.pop("AGX_LIB_PATH", None)
    if lib_path:
        env["AGX_LIB_PATH"] = os.path.abspath(lib_path)
    argv = [sys.executable, os.path.abspath(script or __file__), group, "device" if device else "plan", ",".join(names or [])]
    r = subprocess.run(argv, capture_output=True, timeout=600, env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-3000:]
    return parse(err, json.loads(r.stdout.decode())), err


def record(lib_path=None):
    """Every case, plan-only -> what tests/golden/sw_plan_digests.json holds."""
    out = {}
    for group in GROUPS:
        out.update(run_group(group, lib_path)[0])
    return {name: out[name] for name, _, _, _ in CASES}


def main(argv, **kw):
    """GROUP [plan|device [name,name...]] -> child()"""
    child(argv[1], [n for n in argv[3].split(",") if n] if len(argv) > 3 else None, len(argv) > 2 and argv[2] == "device", **kw)


if __name__ == "__main__":
    main(sys.argv)
