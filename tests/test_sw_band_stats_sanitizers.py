"""AddressSanitizer + UBSan over the host side of stats batches banded around a diagonal (validation, the band conditions per mode,
lane tiling, sort, waves, records; agx_sw_batch_stats on every kind of banded batch) on the CPU build: a stand-alone program
(tests/host/sanitize_band_stats_driver.c) linked with the library's host sources compiled under the sanitizers and its device
objects unchanged; no device is touched (plan-only batches) and nothing is loaded into Python."""
import os

import pytest

from tests import sanitize_build as sb


@pytest.mark.skipif(not os.path.exists(sb.CLANG), reason="ROCm clang not present")
def test_band_stats_planner_under_asan_ubsan(tmp_path):
    sb.run_driver(tmp_path, "sanitize_band_stats_driver", b"SANITIZE_BAND_STATS_DRIVER_OK", "agx_sw_band_stats_kernel.o")
