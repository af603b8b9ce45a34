"""The seeded sweep over every alignment family on the device: the committed corpus of tests/sw_fuzz_cases.py (SEEDS, CASES per
family), one test per family, every comparison exact.

Against the checker: hits of the batch and of the one-shot entry against the family's by-definition checker, statistics against
the stats checkers, op_off and ops against the CIGAR checkers, every returned CIGAR through the family's path_checks /
host_checks, z-drop stops against sw_band_zdrop_ref.  Composition: each case again as two batches (a random split, each half in
reversed order) and one drawn pair alone -- every pair's record as it was in the whole batch -- and the relaunch of the whole
batch.  Agreement between entries: the header's equivalences (sw_fuzz_cases.twins) between two library entries, on the device.
A planted byte: AGX_E_SYMBOL naming the pair.  A failure carries the line that reproduces it with tools/fuzz_align_gpu.py.

What the sweep does not hold: the limits of length (65 535 a side, the query limits of the unbanded entries), which the family
files keep; tests/test_fuzz_align_cpu.py says what the corpus reaches and which wrong kernels it would tell apart."""
import pytest

import accelerating_genomics_amd.api as agx
from tests import sw_fuzz_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    fc.load_checkers()  # compiled once here for the whole module, not inside whichever family's test happens to run first
    with agx.Context(0) as c:
        yield c


def _sweep(ctx, family):
    done = 0
    for case in fc.corpus(family):
        done += fc.check_case(ctx, case)
    assert done >= 4 * (fc.CASES - 2)  # at most two cases of a corpus carry a planted byte


def test_align(ctx):
    _sweep(ctx, "align")


def test_align_mode(ctx):
    _sweep(ctx, "align_mode")


def test_align_matrix(ctx):
    _sweep(ctx, "align_matrix")


def test_align_stats(ctx):
    _sweep(ctx, "align_stats")


def test_align_cigar(ctx):
    _sweep(ctx, "align_cigar")


def test_band(ctx):
    _sweep(ctx, "band")


def test_band_cigar(ctx):
    _sweep(ctx, "band_cigar")


def test_band_diag(ctx):
    _sweep(ctx, "band_diag")


def test_band_diag_cigar(ctx):
    _sweep(ctx, "band_diag_cigar")


def test_band_diag_matrix(ctx):
    _sweep(ctx, "band_diag_matrix")


def test_band_diag_matrix_cigar(ctx):
    _sweep(ctx, "band_diag_matrix_cigar")


def test_band_zdrop(ctx):
    _sweep(ctx, "band_zdrop")


def test_band_zdrop_cigar(ctx):
    _sweep(ctx, "band_zdrop_cigar")


def test_band_diag_stats(ctx):
    _sweep(ctx, "band_diag_stats")


def test_band_diag_dual(ctx):
    _sweep(ctx, "band_diag_dual")


@pytest.mark.parametrize("name", list(fc.REGRESSIONS))
def test_named_regression_case(ctx, name):
    """the drawn cases that found something (sw_fuzz_cases.REGRESSIONS says what)"""
    family, seed, k, _ = fc.REGRESSIONS[name]
    assert fc.check_case(ctx, fc.draw(family, seed, k)) >= 4


def test_every_family_has_its_test():
    assert all("test_" + f in globals() for f in fc.FAMILIES)
