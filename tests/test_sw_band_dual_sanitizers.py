"""AddressSanitizer + UBSan over the host side of batches banded around a diagonal under two-piece gap costs (validation of all
six scoring numbers, the band conditions, the trimmed rows, lane tiling, sort, waves, records) on the CPU build: a stand-alone
program (tests/host/sanitize_band_dual_driver.c) linked with the library's host sources compiled under the sanitizers and its
device objects unchanged; no device is touched (plan-only batches)."""
import os

import pytest

from tests import sanitize_build as sb


@pytest.mark.skipif(not os.path.exists(sb.CLANG), reason="ROCm clang not present")
def test_band_dual_planner_under_asan_ubsan(tmp_path):
    sb.run_driver(tmp_path, "sanitize_band_dual_driver", b"SANITIZE_BAND_DUAL_DRIVER_OK", "agx_sw_band_dual_kernel.o")
