"""AddressSanitizer + UBSan over the host side of batches banded around a diagonal under a substitution matrix (matrix validation
first, then the band conditions, the limits, lane tiling, sort, waves, records; both kinds of batch) on the CPU build: a
stand-alone program (tests/host/sanitize_band_diag_matrix_driver.c) linked with the library's host sources compiled under the
sanitizers and its device objects unchanged; no device is touched (plan-only batches), nothing is loaded into Python."""
import os

import pytest

from tests import sanitize_build as sb


@pytest.mark.skipif(not os.path.exists(sb.CLANG), reason="ROCm clang not present")
def test_band_diag_matrix_planner_under_asan_ubsan(tmp_path):
    sb.run_driver(tmp_path, "sanitize_band_diag_matrix_driver", b"SANITIZE_BAND_DIAG_MATRIX_DRIVER_OK", "agx_sw_band_diag_mat_kernel.o")
