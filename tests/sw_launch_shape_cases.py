"""The batches of tests/test_sw_launch_shape_gpu.py, built the same way in every process that scores them.

Each group needs knobs of the tuning build, so it runs this file as a program in child processes (tests/sw_period_cases.py
is the model): AGX_SW_FORCE_C pins the columns per lane, AGX_SW_PERIOD=4 forces the period of four, AGX_SW_STAGE=0 takes the
staged wave priority off, AGX_TRACE_CREATE makes every create say what it chose.
    usage: python tests/sw_launch_shape_cases.py GROUP OUT.npz N_CU    (stderr: "CASE name" ahead of each create's trace lines)

  c38    packed DNA batches of 150 x 150 pairs in 1, 2, 3, 5 and 9 waves of 4 lanes x 38 columns (sw_fill_pk2w<38>, or
         sw_fill_pk2<38, 4> under AGX_SW_PERIOD=4): a lone wave, a partly filled last workgroup, a last wave with a vacant half
  mixed  one batch of lengths 32 .. 512 that plans into 7 waves of one launch (sw_fill_pk2w_any / sw_fill_pk2_any<4>)
  limit  uniform pairs of 4 x 4 symbols in exactly 8 N_CU waves -- all resident at once: the last batch that is staged -- and in
         one wave more, which is not"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import accelerating_genomics_amd.synth as synth  # noqa: E402

WAVES_C38 = (1, 2, 3, 5, 9)
MIXED_WAVES = 7
KNOBS = {"c38": {"AGX_SW_FORCE_C": "38"}, "mixed": {"AGX_SW_TAIL_BETA": "0"}, "limit": {"AGX_SW_FORCE_C": "4"}}
GROUPS = tuple(KNOBS)


def c38_batch(waves):
    """32 pairs fill a wave (16 groups of 4 lanes, two pairs each): waves - 1 full ones and 19 pairs more."""
    return synth.sw_pairs(32 * (waves - 1) + 19, 150, 150, seed=600 + waves, related_frac=0.4)


def mixed_batch(n_pairs):
    return synth.sw_pairs(n_pairs, 32, 512, seed=77, related_frac=0.5)


def tiny_batch(n_pairs):
    """n_pairs pairs of 4 x 4 symbols over ACGT, no newline."""
    rng = np.random.default_rng(78)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=8 * n_pairs)].copy()
    return synth.SWBatch(bases, np.arange(2 * n_pairs, dtype=np.uint64) * 4, np.full(2 * n_pairs, 4, np.uint32))


def _waves(ctx, b):
    """the waves and launches the planner gives b on this device"""
    plan = ctx.sw_batch(b)
    try:
        return plan.info().n_waves, plan.info().n_launches
    finally:
        plan.close()


def cases(group, ctx, n_cu):
    """-> [(name, SWBatch)]; sizes that depend on the plan are found by planning"""
    if group == "c38":
        return [("waves%d" % w, c38_batch(w)) for w in WAVES_C38]
    if group == "mixed":
        for n in range(4, 400, 4):
            if _waves(ctx, mixed_batch(n)) == (MIXED_WAVES, 1):
                return [("mixed%d" % MIXED_WAVES, mixed_batch(n))]
        raise SystemExit("no mixed batch of %d waves in one launch found" % MIXED_WAVES)
    limit = 8 * n_cu
    w, _ = _waves(ctx, tiny_batch(128 * limit))
    per_wave = -(-128 * limit // w)  # pairs in a full wave
    return [("at_limit", tiny_batch(per_wave * limit)), ("above_limit", tiny_batch(per_wave * limit + 1))]


def main(group, path, n_cu):
    import accelerating_genomics_amd.api as agx

    assert agx.LIB_PATH.endswith("libagx_tuning.so"), agx.LIB_PATH
    got = {}
    with agx.Context(0) as ctx:
        trace = os.environ.pop("AGX_TRACE_CREATE", None)  # (the probes stay quiet: the library asks for it in every create)
        todo = cases(group, ctx, n_cu)
        if trace is not None:
            os.environ["AGX_TRACE_CREATE"] = trace
        for name, b in todo:
            sys.stderr.write("CASE %s\n" % name)
            sys.stderr.flush()
            dev = ctx.sw_batch(b)
            i = dev.info()
            sys.stderr.write("PLAN %d waves %d launches %d pairs\n" % (i.n_waves, i.n_launches, b.n_pairs))
            try:
                dev.launch()
                got[name] = dev.scores()
                got["pairs_" + name] = np.array([b.n_pairs, i.n_waves, i.n_launches], np.int64)  # (the test rebuilds the batch from this)
            finally:
                dev.close()
    np.savez(path, **got)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]))
