"""The packed SW fill looks for the corner cell (the stripped final newlines, agx_sw_pk2_kernel.hip) only from the
quad of steps that holds its wave's first corner step on, and keeps its running maxima per offset within a quad.
These batches put the corner steps of one wave in many quads: the first quad, the last one, the tail steps behind
the quads, and waves where only some lanes have a corner.  Pairs that are copies of each other make the corner
decide the score.  Bar: bit-exact against the oracle, through the one-class launch and the one-launch kernel of
mixed batches."""
import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


def _pairs(rng, n, lx_lo, lx_hi, ly_choices):
    seqs = []
    for k in range(n):
        lx = int(rng.integers(lx_lo, lx_hi + 1))
        ly = int(rng.choice(ly_choices))
        a = ACGT[rng.integers(0, 4, size=lx)].tobytes()
        if k % 3 == 0:  # a copy, cut or extended to ly: the best local alignment ends in the corner
            b = (a * (ly // max(lx, 1) + 1))[:ly]
        elif k % 3 == 1:  # a's tail at the end of y: the corner again, after a run of unrelated rows
            b = (ACGT[rng.integers(0, 4, size=ly)].tobytes() + a)[-ly:]
        else:
            b = ACGT[rng.integers(0, 4, size=ly)].tobytes()
        nl = (k // 3) % 4  # both final newlines, x only, y only, none
        a += b"\n" if nl in (0, 1) else b""
        b += b"\n" if nl in (0, 2) else b""
        seqs += [a, b] if k % 2 else [b, a]  # either side the shorter one
    return synth.sw_from_seqs(seqs)


def _launch(ctx, b):
    dev = ctx.sw_batch(b)
    try:
        dev.launch()
        return dev.scores(), dev.info()
    finally:
        dev.close()


# ly choices: first-quad corners (1..4 rows) next to long rows in one wave; every residue mod 4 around the quad
# boundaries; rows that end exactly at a quad and rows that leave 1..3 tail steps
LY_MIXED = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 34, 35, 60, 61, 62, 63, 64, 149, 150, 151, 152, 153, 300, 301, 302, 303]


@pytest.mark.parametrize("seed", [1, 2])
def test_corner_steps_in_every_quad_one_class(ctx, oracle, seed):
    """Shorter sides of 140 to 150 symbols: one lane-tiling class (the headline's), one launch of sw_fill_pk2."""
    rng = np.random.default_rng(100 + seed)
    b = _pairs(rng, 4096, 140, 150, LY_MIXED)
    s, _ = _launch(ctx, b)
    assert np.array_equal(s, oracle.sw_batch(b))


@pytest.mark.parametrize("seed", [1, 2])
def test_corner_steps_in_every_quad_mixed_classes(ctx, oracle, seed):
    """Shorter sides of 1 to 300 symbols: many classes, the one-launch kernel sw_fill_pk2_any."""
    rng = np.random.default_rng(200 + seed)
    b = _pairs(rng, 4096, 1, 300, LY_MIXED)
    s, _ = _launch(ctx, b)
    assert np.array_equal(s, oracle.sw_batch(b))


def test_one_corner_per_wave(ctx, oracle):
    """Every pair but one per 128 without final newlines: in most waves a single lane looks for a corner, at a step
    that differs from wave to wave."""
    rng = np.random.default_rng(7)
    seqs = []
    for k in range(8192):
        lx, ly = int(rng.integers(100, 151)), int(rng.integers(1, 400))
        a = ACGT[rng.integers(0, 4, size=lx)].tobytes()
        b = (a * (ly // lx + 1))[:ly]
        if k % 128 == int(rng.integers(0, 128)):
            a, b = a + b"\n", b + b"\n"
        seqs += [a, b]
    b = synth.sw_from_seqs(seqs)
    s, _ = _launch(ctx, b)
    assert np.array_equal(s, oracle.sw_batch(b))
