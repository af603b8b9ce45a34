"""Records tests/golden/sw_band_plan_digests.json: per case of tests/sw_band_plan_cases.py the kind line, the plan digest, the fpad
and trimmed-row counts, the launches' diagonals per lane, the image digest and the agx_sw_info fields that a plan-only create of
a banded batch reports under AGX_TRACE_CREATE (tuning build, no device needed).

Run it after a change that is MEANT to alter banded plans or images, with the library that has the change:
    python tools/record_sw_band_plan_digests.py [path/to/libagx_tuning.so] [out.json]
(default: the tree's own libagx_tuning.so and the fixture in place).  tests/test_sw_band_plan_digest_cpu.py compares against it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sw_band_plan_cases  # noqa: E402

if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "accelerating-genomics_amd", "libagx_tuning.so")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "sw_band_plan_digests.json")
    got = sw_band_plan_cases.record(lib)
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(got), out))
