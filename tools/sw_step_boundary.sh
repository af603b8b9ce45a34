#!/bin/bash
# usage: tools/sw_step_boundary.sh OUT.log [TRACE_DIR]
# tools/sw_step_boundary.py untraced, then once under rocprofv3 --hip-trace --kernel-trace (no counters in the same run), then
# the spans A, B, K, C of the trace.  Every GPU step under its own time limit; the first that fails ends the script.
set -o pipefail
here=$(cd "$(dirname "$0")/.." && pwd)
out=${1:?OUT.log}
dir=${2:-$(mktemp -d)}
cd "$here" || exit 1
timeout -k 10 120 python3 tools/sw_step_boundary.py run > "$out" 2>&1 || exit $?
timeout -k 10 240 rocprofv3 --hip-trace --kernel-trace --output-format csv -d "$dir" -o sb -- python3 tools/sw_step_boundary.py run >> "$out" 2>&1 || exit $?
python3 tools/sw_step_boundary.py parse "$dir" >> "$out" 2>&1
