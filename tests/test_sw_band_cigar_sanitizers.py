"""AddressSanitizer + UBSan over the host-only side of banded cigar batches (plan-only creates over odd shapes, the chunk bound of
the traced pairs, the band-aware CIGAR check on good and malformed operation lists) on the CPU build: a stand-alone program
(tests/host/sanitize_band_cigar_driver.c) linked with the library's host sources compiled under the sanitizers and its device
objects unchanged; no device is touched.  Upload, traced fill and walk need a device and run under no sanitizer."""
import os

import pytest

from tests import sanitize_build as sb


@pytest.mark.skipif(not os.path.exists(sb.CLANG), reason="ROCm clang not present")
def test_banded_cigar_host_code_under_asan_ubsan(tmp_path):
    sb.run_driver(tmp_path, "sanitize_band_cigar_driver", b"SANITIZE_BAND_CIGAR_DRIVER_OK", "agx_sw_band_trace_kernel.o")
