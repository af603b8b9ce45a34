"""AddressSanitizer + UBSan over the host side of z-drop batches (validation of zdrop and the mode, the admission rule, lane
tiling, sort, waves, records; agx_sw_batch_zdrop_stops on every kind of batch) on the CPU build: a stand-alone program
(tests/host/sanitize_band_zdrop_driver.c) linked with the library's host sources compiled under the sanitizers and its device
objects unchanged; no device is touched (plan-only batches)."""
import os

import pytest

from tests import sanitize_build as sb


@pytest.mark.skipif(not os.path.exists(sb.CLANG), reason="ROCm clang not present")
def test_band_zdrop_planner_under_asan_ubsan(tmp_path):
    sb.run_driver(tmp_path, "sanitize_band_zdrop_driver", b"SANITIZE_BAND_ZDROP_DRIVER_OK", "agx_sw_band_zdrop_kernel.o")
