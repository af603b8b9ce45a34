"""The batches on which the device planner's records are compared with the host planner's, built the same way in every process.

agx_sw_plan_kernel.hip plans a large mixed batch of the packed biased fill on the device and promises the records the host
planner writes, byte for byte.  Under the tuning build's AGX_TRACE_CREATE a create prints its plan's digest -- "plan digest"
for a host-made plan, "device plan digest" for a device-made one, whose records the trace copies back -- and a "plan parts"
line that hashes head, wave records and group records apart.  Each case below is large enough for the device planner's verdict
on 256 CUs (at least 0.48 x 20 x 256 = 2458 estimated waves; the cases have 2816 and more, fill 0.55) and outside the rules that
need another tiling (tail regime, consolidation, dominant shape); tests/test_sw_devplan_cpu.py holds that of every case.

    python tests/sw_devplan_cases.py plan|device [name,name...]
stderr: "CASE name" ahead of each case's trace lines ("CREATE host" / "CREATE device" ahead of each create in device mode);
stdout: one JSON object, name -> what the mode records.  No knob but AGX_TRACE_CREATE may be set in device mode: any planner
knob sends the batch to the host planner (device_plan_candidate, csrc/agx_sw.cpp)."""
import hashlib
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

INFO_FIELDS = ("n_pairs", "cells", "padded_cells", "input_bytes", "n_launches", "n_waves")
TIE_SHAPE = (137, 301)  # the lengths the ties of `mixed` share, in both orientations


def _lens_mixed():
    """64 001 pairs of 32..512 x 32..512: many (class, G) buckets, odd counts among them (vacant halves).  Pairs 0, 20 000, 40 001
    and 64 000 have an empty side (they sort behind every bucket and score 0).  400 pairs scattered through the file (0.6 %, no
    dominant shape) share the lengths 137 and 301, every other one of them as 301 x 137: a stable sort keeps them in file order,
    each with its own second_short bit."""
    rng = np.random.default_rng(101)
    n = 64001
    la, lb = rng.integers(32, 513, size=n), rng.integers(32, 513, size=n)
    ties = np.sort(rng.choice(np.arange(1, n - 1), size=400, replace=False))
    la[ties], lb[ties] = TIE_SHAPE
    la[ties[1::2]], lb[ties[1::2]] = TIE_SHAPE[::-1]
    special = [0, 20000, 40001, n - 1]
    la[0], lb[20000], la[40001], lb[n - 1] = 0, 0, 0, 0
    return la, lb, special + [int(t) for t in ties[:6]]


def _lens_one_class():
    """96 000 pairs of 150 x 150..399: every pair tiles into one class, so the launch carries that class's C instead of 0 and
    the host orders the waves by steps alone."""
    rng = np.random.default_rng(102)
    n = 96000
    return np.full(n, 150), rng.integers(150, 400, size=n), [0, n - 1]


def _lens_long():
    """6 000 pairs of 1200..2560 x 1200..2700: 64 lanes per group, one pair per half-wave; pair 77 is 2560 x 2700, the packed
    fill's limit on the shorter side, and pair 78 the same the other way round."""
    rng = np.random.default_rng(103)
    n = 6000
    la, lb = rng.integers(1200, 2561, size=n), rng.integers(1200, 2701, size=n)
    la[77], lb[77] = 2560, 2700
    la[78], lb[78] = 2700, 2560
    return la, lb, [77, 78]


def _lens_tail_65535():
    """60 000 pairs of 1..600 x 1..600, pair 30 000 of 65 535 x 40 and pair 59 999 of 1 x 1: beyond the rising cell's range
    (rising 0); the sort key's low field is 0 for the long pair and 65 534 for the shortest, the long pair's wave has the
    largest dispatch key (65 535 + G - 1 steps)."""
    rng = np.random.default_rng(104)
    n = 60000
    la, lb = rng.integers(1, 601, size=n), rng.integers(1, 601, size=n)
    la[30000], lb[30000] = 65535, 40
    la[n - 1], lb[n - 1] = 1, 1
    return la, lb, [30000, n - 1]


def _lens_stride():
    """1 100 000 pairs of 8..48 x 8..48: more pairs than the 16 x 256 x 256 = 1 048 576 threads the planning kernels launch at
    most on 256 CUs, so every grid-stride loop runs a second iteration; radix sort and scan beyond 2^20 entries."""
    rng = np.random.default_rng(105)
    n = 1100000
    return rng.integers(8, 49, size=n), rng.integers(8, 49, size=n), [0, 1048575, 1048576, n - 1]


CASES = {"mixed": _lens_mixed, "one_class": _lens_one_class, "long": _lens_long, "tail_65535": _lens_tail_65535, "stride": _lens_stride}


def lens(name):
    """-> (la, lb, the pairs the oracle subset must hold) of the named case."""
    la, lb, special = CASES[name]()
    return la.astype(np.uint32), lb.astype(np.uint32), special


def lens_sha256(name):
    la, lb, _ = lens(name)
    return hashlib.sha256(la.tobytes() + lb.tobytes()).hexdigest()


def subset(name):
    """At most 64 pairs whose scores go through the oracle: the case's special pairs and others spread evenly."""
    la, _, special = lens(name)
    n = la.size
    spread = [int(p) for p in np.linspace(0, n - 1, 64 - len(special)).astype(np.int64)]
    out = sorted(set(special + spread))
    assert len(out) <= 64
    return out


def batch(name):
    """The named case as a synth.SWBatch: ACGT from a seeded generator, no newline.  In every pair of the oracle subset and in
    every 97th pair the second sequence is a copy of the start of the first (as far as both reach) with a base in 16 redrawn,
    so that scores are not those of unrelated sequences alone."""
    la, lb, _ = lens(name)
    n = la.size
    ln = np.empty(2 * n, np.uint32)
    ln[0::2], ln[1::2] = la, lb
    off = np.zeros(2 * n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    bases = acgt[rng.integers(0, 4, size=int(ln.sum(dtype=np.uint64)), dtype=np.uint8)]
    for p in sorted(set(subset(name)) | set(range(0, n, 97))):
        k = int(min(la[p], lb[p]))
        if k == 0:
            continue
        a, b = int(off[2 * p]), int(off[2 * p + 1])
        copy = bases[a:a + k].copy()
        hit = rng.random(k) < 1.0 / 16
        copy[hit] = acgt[rng.integers(0, 4, size=int(hit.sum()))]
        bases[b:b + k] = copy
    return synth.SWBatch(bases, off, ln)


def _info(dev):
    i = dev.info()
    d = {f: int(getattr(i, f)) for f in INFO_FIELDS}
    d["planned_on_device"] = int(i.planned_on_device)
    return d


def child(mode, names):
    """Creates the cases (all, or `names`) in this process.  plan: plan-only, the info fields.  device: on device 0, first with
    the host planner, then with the device planner; each is launched and its scores hashed."""
    import accelerating_genomics_amd.api as agx

    out = {}
    ctx = agx.Context(0) if mode == "device" else None
    try:
        for name in CASES:
            if names and name not in names:
                continue
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            b = batch(name)
            if ctx is None:
                dev = agx.SwBatch(None, b)
                try:
                    out[name] = {"info": _info(dev)}
                finally:
                    dev.close()
                continue
            sub = subset(name)
            out[name] = {}
            for label, planner in (("host", agx.SW_PLANNER_HOST), ("device", agx.SW_PLANNER_DEVICE)):
                sys.stderr.write("CREATE %s\n" % label)
                sys.stderr.flush()
                ctx.set_option(agx.OPT_SW_PLANNER, planner)
                try:
                    dev = ctx.sw_batch(b)
                finally:
                    ctx.set_option(agx.OPT_SW_PLANNER, agx.SW_PLANNER_AUTO)
                try:
                    dev.launch()
                    s = dev.scores()
                    out[name][label] = {"info": _info(dev), "scores_sha256": hashlib.sha256(s.tobytes()).hexdigest(),
                                        "subset": [int(v) for v in s[sub]]}
                finally:
                    dev.close()
        sys.stderr.write("CASE end\n")
    finally:
        if ctx is not None:
            ctx.close()
    print(json.dumps(out))


_LINES = {
    "digest": r"plan digest ([0-9a-f]{16})$",
    "on_device": r"plan digest: (on device)$",
    "device_digest": r"device plan digest ([0-9a-f]{16})$",
    "parts": r"(plan parts: .*)$",
    "family": r"(family \d+ rising \d+): longest",
    "verdict": r"(device planner verdict \d+: .*)$",
}


def _lines(text):
    e = {}
    for key, pat in _LINES.items():
        m = re.findall(r"^\[agx_sw_batch_create\] " + pat, text, flags=re.M)
        assert len(m) <= 1, (key, text)
        if m:
            e[key] = m[0]
    return e


def parse(stderr, results, mode):
    """The trace of one child and its JSON -> name -> entry (device mode: name -> "host" / "device" -> entry)."""
    parts = re.split(r"^CASE (\w+)\n", stderr, flags=re.M)[1:]
    out = {}
    for name, text in zip(parts[0::2], parts[1::2]):
        if name == "end":
            continue
        if mode == "plan":
            out[name] = dict(_lines(text), **results[name])
            continue
        creates = re.split(r"^CREATE (\w+)\n", text, flags=re.M)[1:]
        out[name] = {label: dict(_lines(t), **results[name][label]) for label, t in zip(creates[0::2], creates[1::2])}
    return out


def run(mode, names=None, extra_env=None, timeout=120):
    """One fresh child process -> (name -> entry, its whole stderr).  A child that fails, is killed by a signal or runs out of
    time raises (AssertionError / TimeoutExpired); nothing is tried again."""
    env = dict(os.environ, AGX_TRACE_CREATE="1")
    env.update(extra_env or {})
    env.pop("AGX_LIB_PATH", None)
    argv = [sys.executable, os.path.abspath(__file__), mode, ",".join(names or [])]
    r = subprocess.run(argv, capture_output=True, timeout=timeout, env=env)
    err = r.stderr.decode()
    assert r.returncode == 0, "child %s %s ended with status %d:\n%s" % (mode, names, r.returncode, err[-3000:])
    return parse(err, json.loads(r.stdout.decode()), mode), err


if __name__ == "__main__":
    child(sys.argv[1], [n for n in sys.argv[2].split(",") if n] if len(sys.argv) > 2 else None)
