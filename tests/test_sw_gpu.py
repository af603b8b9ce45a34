"""GPU parity of the Smith-Waterman fill (through the C-ABI) against the oracle and the
reference's golden outputs.  Bar: bit-exact int32 scores."""
import glob
import os

import numpy as np
import pytest

import accelerating_genomics_amd.api as agx
import accelerating_genomics_amd.synth as synth
from tests import oracle_api
from tests.test_oracle_sw import expect_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with agx.Context(0) as c:
        yield c


GOLD = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "sw_*.in")))


@pytest.mark.parametrize("name", GOLD)
def test_golden_files_bit_exact(ctx, golden_dir, name):
    """text reader + kernel vs stdout of the unmodified reference program."""
    n_ref, s_ref = expect_scores(os.path.join(golden_dir, name + ".expect"))
    line_num, b, _ = agx.read_sw_text(os.path.join(golden_dir, name + ".in"))
    assert line_num == n_ref
    assert np.array_equal(ctx.sw_score(b), s_ref)


@pytest.mark.parametrize("lo,hi,n,seed", [(1, 8, 500, 1), (1, 70, 2000, 2), (150, 150, 1024, 3), (32, 512, 1500, 4),
                                          (500, 999, 64, 5), (1000, 2500, 6, 6)])
def test_random_and_related_pairs_vs_oracle(ctx, oracle, lo, hi, n, seed):
    b = synth.sw_pairs(n, lo, hi, seed=seed, related_frac=0.5)
    assert np.array_equal(ctx.sw_score(b), oracle.sw_batch(b))


def test_every_short_length_and_tiling_boundary(ctx, oracle):
    """lx = 1..170 against ly in {lx, lx+1, 3*lx}: walks every (C, G) choice incl. non-power-of-two G."""
    rng = np.random.default_rng(7)
    seqs = []
    for lx in range(1, 171):
        for ly in (lx, lx + 1, 3 * lx):
            a = b"ACGT"[0:0] + bytes(rng.choice(list(b"ACGT"), size=lx).tolist())
            y = bytearray(rng.choice(list(b"ACGT"), size=ly).tolist())
            st = int(rng.integers(0, ly - lx + 1))
            y[st : st + lx] = a  # embed a copy so the optimum is a long diagonal
            if lx > 4:
                y[st + lx // 2] = ord("N")
            seqs += [a, bytes(y)]
    b = synth.sw_from_seqs(seqs)
    assert np.array_equal(ctx.sw_score(b), oracle.sw_batch(b))


def test_empty_and_degenerate(ctx, oracle):
    b = synth.sw_from_seqs([b"", b"ACGT", b"ACGT", b"", b"", b"", b"A", b"A", b"\n", b"\n", b"A\n", b"C\n"])
    got = ctx.sw_score(b)
    assert np.array_equal(got, oracle.sw_batch(b))
    assert list(got) == [0, 0, 0, 1, 1, 1]
    assert ctx.sw_score(synth.sw_from_seqs([])).size == 0


def test_all_byte_values_are_symbols(ctx, oracle):
    rng = np.random.default_rng(11)
    seqs = [bytes(rng.integers(1, 256, size=int(rng.integers(1, 300))).astype(np.uint8).tolist()) for _ in range(400)]
    for k in range(0, 400, 4):  # make some pairs related
        seqs[k + 1] = seqs[k][3:] + seqs[k + 1][:5]
    b = synth.sw_from_seqs(seqs)
    assert np.array_equal(ctx.sw_score(b), oracle.sw_batch(b))


def test_reserved_symbol_and_limits_fail_loudly(ctx):
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_score(synth.sw_from_seqs([b"AC\x00GT", b"ACGT"]))
    assert e.value.code == agx.E_SYMBOL
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_score(synth.sw_from_seqs([b"A" * 10241, b"C" * 10241]))
    assert e.value.code == agx.E_LIMIT


def test_batch_object_relaunch_is_idempotent(ctx, oracle):
    b = synth.sw_pairs(3000, 100, 200, seed=9, related_frac=0.3)
    dev = ctx.sw_batch(b)
    dev.launch()
    first = dev.scores()
    for _ in range(3):
        dev.launch()
    assert np.array_equal(dev.scores(), first)
    assert np.array_equal(first, oracle.sw_batch(b))
    info = dev.info()
    assert info.n_pairs == 3000 and info.cells == b.cells() and info.padded_cells >= info.cells
    dev.close()


def test_full_size_config2_properties(ctx, oracle):
    """BASELINE config 2 at full size (65 536 pairs, 150x150): (a) EVERY pair against the oracle (its row-major
    restatement threaded over the host cores, about a second), (b) score(a,b) == score(b,a),
    (c) identical pairs score len+1 (the '\\n' sentinel matches too), (d) the int32 and the
    first packed kernel give the same 65 536 scores."""
    b = synth.sw_pairs(65536, 150, 150, seed=2, related_frac=0.25)
    got = ctx.sw_score(b)
    assert np.array_equal(got, oracle_api.sw_batch_mt(oracle, b))
    for kern in (agx.SW_KERNEL_INT32, agx.SW_KERNEL_PACKED_SIGNED):
        ctx.set_option(agx.OPT_SW_KERNEL, kern)
        try:
            assert np.array_equal(ctx.sw_score(b), got), kern
        finally:
            ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
    swapped = synth.SWBatch(b.bases, b.off.reshape(-1, 2)[:, ::-1].reshape(-1).copy(), b.len.reshape(-1, 2)[:, ::-1].reshape(-1).copy())
    assert np.array_equal(ctx.sw_score(swapped), got)
    same = synth.SWBatch(b.bases, np.repeat(b.off[0::2], 2), np.repeat(b.len[0::2], 2))
    assert np.array_equal(ctx.sw_score(same), b.len[0::2].astype(np.int32))


def test_full_size_config4_mixed_lengths(ctx, oracle):
    """BASELINE config 4 at full size (1 048 576 pairs, both lengths U[32,512]); one GPU takes the
    whole batch here (the 8-GPU run shards it).  (a) a 1/16 sample (65 536 pairs, every 16th) against the
    threaded oracle, (b) scoring two halves separately == scoring the whole, (c) score(a,b) == score(b,a)
    on a 64k slice."""
    b = synth.sw_pairs(1 << 20, 32, 512, seed=4)
    got = ctx.sw_score(b)
    idx = np.arange(0, 1 << 20, 16)
    assert np.array_equal(got[idx], oracle_api.sw_batch_mt(oracle, b.subset(idx)))
    half = 1 << 19
    lo = synth.SWBatch(b.bases, b.off[: 2 * half], b.len[: 2 * half])
    hi = synth.SWBatch(b.bases, b.off[2 * half :], b.len[2 * half :])
    assert np.array_equal(np.concatenate([ctx.sw_score(lo), ctx.sw_score(hi)]), got)
    sl = synth.SWBatch(b.bases, b.off[:131072].reshape(-1, 2)[:, ::-1].reshape(-1).copy(),
                       b.len[:131072].reshape(-1, 2)[:, ::-1].reshape(-1).copy())
    assert np.array_equal(ctx.sw_score(sl), got[:65536])
    assert got.min() >= 0 and got.max() <= 513


def test_external_stream_from_torch(tmp_path):
    """A host that owns a HIP stream (here: PyTorch) installs it with agx_ctx_set_stream; launches then
    order with that stream's other work and torch.cuda.synchronize() covers them.  Runs in its own
    process with torch initialised first, as a torch host would (torch ships its own HIP runtime;
    whichever runtime a process loads first is the one every library in it must share)."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        import torch
        st = torch.cuda.Stream()
        import accelerating_genomics_amd.api as agx, accelerating_genomics_amd.synth as synth
        from tests import oracle_api
        b = synth.sw_pairs(4096, 50, 300, seed=21, related_frac=0.5)
        with agx.Context(0) as c:
            c.set_stream(st.cuda_stream)
            assert c.stream == st.cuda_stream
            dev = c.sw_batch(b)
            with torch.cuda.stream(st):
                dev.launch()
            torch.cuda.synchronize()
            assert np.array_equal(dev.scores(), oracle_api.load().sw_batch(b))
            dev.close()
        print("STREAM_OK")
    """) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"STREAM_OK" in r.stdout, r.stderr.decode()[-1500:]


def test_largest_supported_shapes(ctx, oracle):
    """shorter side 2560 = 64 lanes x 40 columns; longer side up to 65 535 rows streams."""
    rng = np.random.default_rng(31)
    a = bytes(rng.choice(list(b"ACGT"), size=2560).tolist())
    y = bytearray(rng.choice(list(b"ACGT"), size=65535).tolist())
    y[30000:32560] = a  # a full-length hit in the middle
    y[31000] = ord("N")
    b = synth.sw_from_seqs([a, bytes(y), bytes(y[:3000]), a[:2000]])
    got = ctx.sw_score(b)
    assert np.array_equal(got, oracle.sw_batch(b))
    assert got[0] >= 2550


@pytest.mark.parametrize("scoring", [(1, -1, -3, -1), (2, -3, -5, -2), (5, -4, -10, -1), (1, -3, 0, -2), (3, -1, -4, 0),
                                     (12, -100, -50, -7), (2, 0, -1, -1), (3, -1, -10, -3), (4, -6, -2, -5)])
def test_runtime_scoring_vs_parametrised_oracle(ctx, oracle, scoring):
    """8f n3.  Only (1,-1,-3,-1) is the reference's; the rest is pinned against the oracle's own Gotoh."""
    b = synth.sw_pairs(1500, 1, 400, seed=abs(sum(scoring)) + 50, related_frac=0.6)
    dev = ctx.sw_batch(b, scoring)
    dev.launch()
    got = dev.scores()
    dev.close()
    assert np.array_equal(got, oracle.sw_batch_scored(b, scoring))
    if scoring == (1, -1, -3, -1):
        assert np.array_equal(got, ctx.sw_score(b))


def test_scoring_limits(ctx, oracle):
    b = synth.sw_pairs(4, 10, 20, seed=1)
    for bad in [(0, -1, -3, -1), (13, -1, -3, -1), (2, 1, -3, -1), (1, -200, -3, -1), (1, -1, 1, -1), (1, -1, -3, -2000)]:
        with pytest.raises(agx.AgxError) as e:
            ctx.sw_batch(b, bad)
        assert e.value.code == agx.E_LIMIT
    # the largest scores the int16 lanes must hold: match 12 on identical 2560-mers
    long = synth.sw_from_seqs([b"ACGT" * 640, b"ACGT" * 640])
    dev = ctx.sw_batch(long, (12, -1, -3, -1))
    dev.launch()
    assert list(dev.scores()) == [12 * 2560] == list(oracle.sw_batch_scored(long, (12, -1, -3, -1)))
    dev.close()


def test_wide_classes_beyond_the_packed_kernel(ctx, oracle):
    """Shorter sides of 2561..10240 symbols (hipvers.cpp:40 reads lines up to 9999 bytes): one such
    pair moves the batch to the int32 kernel with its 80/120/160-column classes."""
    rng = np.random.default_rng(41)
    seqs = []
    for lx, ly in ((2561, 2561), (4000, 4500), (7680, 7680), (9999, 9999), (10240, 12000), (100, 120)):
        a = bytes(rng.choice(list(b"ACGT"), size=lx).tolist())
        y = bytearray(rng.choice(list(b"ACGT"), size=ly).tolist())
        y[ly - lx : ly - lx + lx // 2] = a[: lx // 2]  # half of a embedded
        seqs += [a, bytes(y)]
    b = synth.sw_from_seqs(seqs)
    assert np.array_equal(ctx.sw_score(b), oracle.sw_batch(b))


def test_substitution_matrix_blosum62_vs_oracle(ctx, oracle):
    """8f n3, "parity unpinned": the reference has no matrix mode; checked against the oracle's Gotoh
    with the same matrix (BLAST's protein defaults: BLOSUM62, existence 11, extension 1)."""
    m = agx.SwMatrix.build(synth.AMINO, synth.BLOSUM62, -11, -1)
    b = synth.protein_pairs(3000, 1, 600, seed=11)
    dev = ctx.sw_batch(b, matrix=m)
    dev.launch()
    dev.launch()
    got = dev.scores()
    dev.close()
    ref = oracle.sw_batch_matrix(b, m)
    assert np.array_equal(got, ref) and ref.max() > 500
    # lower case maps to the same residues; every short length and tiling edge once
    seqs = []
    rng = np.random.default_rng(12)
    aa = np.frombuffer(synth.AMINO, np.uint8)
    for lx in list(range(1, 90)) + [159, 160, 161, 640, 1279, 1280, 1281, 2559, 2560]:
        a = aa[rng.integers(0, 20, size=lx)].tobytes()
        y = aa[rng.integers(0, 20, size=lx + int(rng.integers(0, 40)))].tobytes()
        seqs += [a.lower() if lx % 2 else a, y[: lx // 2] + a[lx // 3 :] + y[lx // 2 :]]
    b = synth.sw_from_seqs(seqs)
    assert np.array_equal(_scores(ctx, b, m), oracle.sw_batch_matrix(b, m))


def _scores(ctx, b, m):
    dev = ctx.sw_batch(b, matrix=m)
    dev.launch()
    out = dev.scores()
    dev.close()
    return out


@pytest.mark.parametrize("scoring", [(1, -1, -3, -1), (2, -3, -5, -2), (5, -4, -10, 0)])
def test_match_mismatch_matrix_equals_runtime_scoring(ctx, oracle, scoring):
    """A matrix holding match on the diagonal and mismatch elsewhere must give the scores of
    agx_sw_batch_create_scored -- at (1,-1,-3,-1) the reference's own."""
    match, mis, go, ge = scoring
    b = synth.sw_pairs(2000, 1, 300, seed=21, related_frac=0.5)
    m = agx.SwMatrix.build(b"ACGT\n", [[match if a == c else mis for c in range(5)] for a in range(5)], go, ge)
    got = _scores(ctx, b, m)
    dev = ctx.sw_batch(b, scoring)
    dev.launch()
    assert np.array_equal(got, dev.scores())
    dev.close()
    assert np.array_equal(got, oracle.sw_batch_scored(b, scoring))


def test_matrix_with_no_negative_entry_and_empty_sides(ctx, oracle):
    m = agx.SwMatrix.build(b"AB", [[2, 0], [0, 3]], 0, -1)
    b = synth.sw_from_seqs([b"", b"AB", b"ABBA", b"", b"ABABAB", b"BBBAAA", b"A", b"B"])
    assert np.array_equal(_scores(ctx, b, m), oracle.sw_batch_matrix(b, m))
    with pytest.raises(agx.AgxError) as e:
        _scores(ctx, synth.sw_from_seqs([b"ABC", b"AB"]), m)
    assert e.value.code == agx.E_SYMBOL


def test_all_four_cells_of_the_biased_fill(ctx, oracle):
    """The default SW kernel picks its cell per batch and per wavefront (agx_sw_pk2_kernel.hip): DNA-coded or general
    (decided on the device: at most four symbols per shorter sequence, sentinels only at the very end) x rising offsets
    or plain (decided on the host: rows up to about 27 000).  One batch per combination, each with sentinel variants
    (both, one, none), a newline inside a sequence, and a fifth symbol, against the oracle."""
    rng = np.random.default_rng(4242)
    acgt, prot = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", np.uint8)

    def seq(n, alpha):
        return alpha[rng.integers(0, alpha.size, size=n)].tobytes()

    def related(a, alpha):
        b = bytearray(a)
        for _ in range(max(1, len(b) // 40)):
            pos = int(rng.integers(0, len(b)))
            b[pos : pos + int(rng.integers(0, 3))] = seq(int(rng.integers(0, 3)), alpha)
        return bytes(b)

    def batch(alpha, long_rows):
        seqs = []
        for k in range(160):
            lx = int(rng.integers(1, 300))
            ly = int(rng.integers(1, 400))
            a = seq(lx, alpha)
            b = related(a, alpha) + seq(ly, alpha) if k % 3 else seq(ly, alpha)
            nl = k % 4  # both, first only, second only, none
            a += b"\n" if nl in (0, 1) else b""
            b += b"\n" if nl in (0, 2) else b""
            if k % 17 == 5:
                b = b[: len(b) // 2] + b"\n" + b[len(b) // 2 :]  # a newline INSIDE: the sentinel may align with it
            if k % 19 == 7:
                a = a[:1] + b"N" + a[1:]  # a fifth symbol in some pairs
            seqs += [a, b]
        if long_rows:  # one pair beyond the rising cell's range moves the whole batch to the plain cell
            a = seq(200, alpha)
            seqs += [a + b"\n", seq(15000, alpha) + a + seq(15000, alpha) + b"\n"]
        return synth.sw_from_seqs(seqs)

    for alpha in (acgt, prot):
        for long_rows in (False, True):
            b = batch(alpha, long_rows)
            assert np.array_equal(ctx.sw_score(b), oracle.sw_batch(b)), (alpha.size, long_rows)


def _planned(ctx, b, planner):
    ctx.set_option(agx.OPT_SW_PLANNER, planner)
    try:
        dev = ctx.sw_batch(b)
    finally:
        ctx.set_option(agx.OPT_SW_PLANNER, agx.SW_PLANNER_AUTO)
    dev.launch()
    s, i = dev.scores(), dev.info()
    dev.close()
    return s, i


@pytest.mark.parametrize("n,lo,hi,seed", [(80000, 32, 512, 21), (150000, 20, 300, 22), (70001, 100, 700, 23)])
def test_device_planner_writes_the_host_planner_s_plan(ctx, oracle, n, lo, hi, seed):
    """the planner's per-pair passes as kernels (agx_sw_plan_kernel.hip: keys, stable radix sort,
    scan, records, wave order).  Same tiling table, same keys, stable sorts: the plan must be the host planner's --
    same wave count, padded cells, image size, one launch -- and the scores bit-exact against the oracle."""
    b = synth.sw_pairs(n, lo, hi, seed=seed, related_frac=0.3)
    b.len[2 * 17] = 0          # a pair with an empty side: sorts behind every bucket, scores 0
    b.len[2 * 4097 + 1] = 0
    s_host, i_host = _planned(ctx, b, agx.SW_PLANNER_HOST)
    s_dev, i_dev = _planned(ctx, b, agx.SW_PLANNER_DEVICE)
    assert i_host.planned_on_device == 0 and i_dev.planned_on_device == 1
    for f in ("n_pairs", "cells", "padded_cells", "input_bytes", "n_launches", "n_waves"):
        assert getattr(i_host, f) == getattr(i_dev, f), f
    assert np.array_equal(s_host, s_dev) and s_dev[17] == 0 and s_dev[4097] == 0
    sub = np.arange(0, n, 7)
    assert np.array_equal(s_dev[sub], oracle_api.sw_batch_mt(oracle, b.subset(sub)))


def test_device_planner_leaves_small_uniform_and_tail_batches_to_the_host(ctx, oracle):
    """The batch-level rules that need another tiling (tail regime, dominant shape) and uniform batches stay with the
    host planner even when the device planner is asked for; AUTO takes the device only from 49 152 pairs on."""
    for b in (synth.sw_pairs(4000, 32, 512, seed=31), synth.sw_pairs(65536, 150, 150, seed=2), synth.sw_pairs(30000, 1, 40, seed=32)):
        s, i = _planned(ctx, b, agx.SW_PLANNER_DEVICE)
        assert i.planned_on_device == 0
        assert np.array_equal(s[::5], oracle_api.sw_batch_mt(oracle, b.subset(np.arange(0, b.n_pairs, 5))))
    b = synth.sw_pairs(40000, 32, 512, seed=33)
    assert _planned(ctx, b, agx.SW_PLANNER_AUTO)[1].planned_on_device == 0
    b = synth.sw_pairs(131072, 32, 512, seed=34)
    s, i = _planned(ctx, b, agx.SW_PLANNER_AUTO)
    assert i.planned_on_device == 1
    assert np.array_equal(s[::16], oracle_api.sw_batch_mt(oracle, b.subset(np.arange(0, b.n_pairs, 16))))


def test_one_shot_score_of_a_large_batch_runs_in_pieces(ctx, oracle):
    """agx_sw_score sends a batch of more than about 128 MB through in contiguous pieces (piece k + 1 uploaded and planned
    beside the fill of piece k): same scores as the one-batch path, errors name pair numbers of the WHOLE batch."""
    b = synth.sw_pairs(300000, 150, 450, seed=41, related_frac=0.2)
    assert b.bases.size > (160 << 20)
    got = ctx.sw_score(b)
    dev = ctx.sw_batch(b)
    dev.launch()
    assert np.array_equal(got, dev.scores())
    dev.close()
    sub = np.arange(0, b.n_pairs, 37)
    assert np.array_equal(got[sub], oracle_api.sw_batch_mt(oracle, b.subset(sub)))
    bad = synth.SWBatch(b.bases.copy(), b.off, b.len)
    bad.bases[int(b.off[2 * 250001]) + 3] = 0      # the padding symbol inside a pair of the second piece
    with pytest.raises(agx.AgxError) as e:
        ctx.sw_score(bad)
    assert e.value.code == agx.E_SYMBOL and "pair 250001 " in str(e.value)


def test_bound_scores_arrive_in_the_callers_page_locked_array(ctx, oracle):
    """agx_sw_batch_bind_scores: a batch planned in file order (uniform lengths) writes its scores into the caller's
    page-locked array from the fill itself (8-byte stores, a wave's groups side by side); odd pair counts (the vacant
    half's spare slot does not exist there), every kernel family, rebinding, and a sorted batch, for which the call is a
    hint and the copy stays."""
    for n in (4097, 20000):
        b = synth.sw_pairs(n, 150, 150, seed=50 + n, related_frac=0.3)
        want = oracle_api.sw_batch_mt(oracle, b)
        for kernel in (agx.SW_KERNEL_AUTO, agx.SW_KERNEL_INT32, agx.SW_KERNEL_PACKED_SIGNED):
            ctx.set_option(agx.OPT_SW_KERNEL, kernel)
            try:
                dev = ctx.sw_batch(b)
            finally:
                ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)
            out = agx.host_array(n + 8, np.int32)
            out[:] = -7
            dev.bind_scores(out[:n])
            for _ in range(2):
                dev.launch()
                got = dev.scores(out[:n])
                assert got is not None and np.array_equal(out[:n], want) and np.all(out[n:] == -7)  # nothing written behind the array
            other = np.empty(n, np.int32)              # fetched elsewhere while bound: a copy of the bound array
            dev.launch()
            assert np.array_equal(dev.scores(other), want)
            dev.bind_scores(None)                      # unbound: the device array and the copy kernel again
            dev.launch()
            assert np.array_equal(dev.scores(), want)
            with pytest.raises(agx.AgxError):
                dev.bind_scores(np.empty(n, np.int32))  # not page-locked
            dev.close()
    mixed = synth.sw_pairs(3000, 20, 300, seed=77)
    dev = ctx.sw_batch(mixed)
    out = agx.host_array(mixed.n_pairs, np.int32)
    dev.bind_scores(out)                               # a hint here
    dev.launch()
    assert np.array_equal(dev.scores(out), oracle.sw_batch(mixed))
    dev.close()


def test_device_planned_batch_with_waves_of_every_kind(ctx, oracle):
    """A large mixed batch whose waves are of every kind the pack kernel knows: plain DNA (coded), a fifth symbol in the
    shorter sequence (bytes, general cell), a newline inside a sequence, a missing final newline, sequences of one and two
    symbols, lengths up to the packed kernel's 2560 columns -- planned on the device, packed by 16-byte chunks, scored
    bit-exactly."""
    rng = np.random.default_rng(91)
    b = synth.sw_pairs(130000, 1, 260, seed=92, related_frac=0.3)
    long_ones = synth.sw_pairs(40, 1800, 2559, seed=93, related_frac=0.5)
    bases = np.concatenate([b.bases, long_ones.bases])
    off = np.concatenate([b.off, long_ones.off + np.uint64(b.bases.size)])
    ln = np.concatenate([b.len, long_ones.len])
    b = synth.SWBatch(bases, off, ln)
    n = b.n_pairs
    for p in rng.choice(n, size=n // 10, replace=False):          # an N somewhere in one sequence of the pair
        k = 2 * int(p) + int(rng.integers(0, 2))
        if b.len[k] > 1:
            b.bases[int(b.off[k]) + int(rng.integers(0, int(b.len[k]) - 1))] = ord("N")
    for p in rng.choice(n, size=300, replace=False):              # a newline inside / no final newline
        k = 2 * int(p) + int(rng.integers(0, 2))
        if b.len[k] > 2:
            if rng.random() < 0.5:
                b.bases[int(b.off[k]) + int(rng.integers(0, int(b.len[k]) - 1))] = 10
            else:
                b.bases[int(b.off[k]) + int(b.len[k]) - 1] = ord("A")
    s_dev, i_dev = _planned(ctx, b, agx.SW_PLANNER_DEVICE)
    assert i_dev.planned_on_device == 1
    sub = np.concatenate([np.arange(0, 130000, 17), np.arange(130000, n)])
    assert np.array_equal(s_dev[sub], oracle_api.sw_batch_mt(oracle, b.subset(sub)))
    s_host, i_host = _planned(ctx, b, agx.SW_PLANNER_HOST)
    assert np.array_equal(s_host, s_dev) and i_host.padded_cells == i_dev.padded_cells and i_host.n_waves == i_dev.n_waves


def test_int32_kernel_with_the_coded_match_across_scorings(ctx, oracle):
    """AGX_SW_KERNEL_INT32 runs the packed plan's DNA-coded image in 32-bit state (agx_sw_i32d_kernel.hip) wherever the
    coded match exists, else agx_sw_kernel.inc's cell: several scorings (one with match - mismatch >= 128: no coded
    match), waves with a fifth symbol (general 32-bit cell), empty sides, odd pair counts, sequences without newline."""
    rng = np.random.default_rng(5)
    b = synth.sw_pairs(6001, 1, 330, seed=61, related_frac=0.5)
    for p in rng.choice(b.n_pairs, size=400, replace=False):
        k = 2 * int(p) + int(rng.integers(0, 2))
        if b.len[k] > 1:
            b.bases[int(b.off[k]) + int(rng.integers(0, int(b.len[k]) - 1))] = ord("N")
    b.len[2 * 33] = 0
    nonl = synth.sw_pairs(500, 20, 200, seed=62, related_frac=0.5, newline=False)
    ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_INT32)
    try:
        for batch in (b, nonl):
            for scoring in ((1, -1, -3, -1), (2, -3, -5, -2), (5, -4, -10, -1), (1, 0, 0, -1), (12, -116, -30, -7), (3, -1, 0, 0)):
                dev = ctx.sw_batch(batch, scoring=scoring)
                dev.launch()
                assert np.array_equal(dev.scores(), oracle.sw_batch_scored(batch, scoring)), scoring
                dev.close()
    finally:
        ctx.set_option(agx.OPT_SW_KERNEL, agx.SW_KERNEL_AUTO)


def test_plan_on_a_device_is_the_plan_only_plan():
    """A host-made plan does not depend on whether a device is there: for the uniform 1024 x 150 x 150 batch, the mixed 300 of
    32..512 and the 500 protein pairs under BLOSUM62 of tests/sw_plan_cases.py, created on device 0 in a child process under
    AGX_TRACE_CREATE, the "plan digest" line (from the host copies of the records that were uploaded) equals the plan-only one
    of tests/golden/sw_plan_digests.json.  Plan-only batches are tiled for 256 CUs and never staged; the child runs under
    AGX_SW_STAGE=0, so that the staged-priority word of the digest is the plan-only one, and a case is compared whenever its
    family, class-period and staged-priority lines equal the recorded ones: the matrix batch on any device (family 0, no such
    choice), all three on a device of 256 CUs."""
    import json

    from tests import sw_plan_cases as pc

    with open(os.path.join(os.path.dirname(__file__), "golden", "sw_plan_digests.json")) as f:
        golden = json.load(f)
    names = ["uniform_1024", "mixed_300", "matrix_500"]
    got, err = pc.run_group("default", names=names, device=True, extra_env={"AGX_SW_STAGE": "0"})
    assert sorted(got) == sorted(names), err[-2000:]
    compared = []
    for name in names:
        want = golden[name]
        if all(got[name].get(k) == want.get(k) for k in ("family", "period", "staged")):
            assert got[name]["digest"] == want["digest"] and got[name]["info"] == want["info"], (name, got[name], want, err[-2000:])
            compared.append(name)
    assert "matrix_500" in compared, (got, err[-2000:])
    if " 2048 resident at once" in err:  # 8 waves on each of 256 CUs
        assert compared == names, (got, err[-2000:])
