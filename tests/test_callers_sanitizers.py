"""ThreadSanitizer over the host side of libagx with several CALLERS (tests/host/sanitize_callers_driver.c): four pthreads make
plan-only creates of every batch family at once -- so the process-wide worker pool serves four callers, each of which runs the
others' queued parts while it waits for its own -- and two of them run the text readers at the same time, on files large enough
for the readers' pool to split.  Every result must equal the one made before the callers started.  A stand-alone program on the
CPU build: the device objects are linked unchanged, no device is touched, nothing is loaded into Python under the sanitizer."""
import os

import pytest

from tests import sanitize_build as sb
from tests.sanitize_build import CLANG


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang not present")
def test_four_callers_under_tsan(tmp_path, golden_dir):
    scratch = tmp_path / "files"
    scratch.mkdir()
    sb.run_driver(tmp_path, "sanitize_callers_driver", b"SANITIZE_CALLERS_OK", "agx_phmm_finish_kernel.o", sanitizers="thread",
                  defines=["-DAGX_TUNING"], args=[golden_dir, str(scratch)],
                  env_extra=dict(TSAN_OPTIONS="halt_on_error=1", AGX_HOST_THREADS="4"))  # (a tuning-build knob)
