#!/bin/bash
# Development aid (CPU only, no GPU needed): the frame loop's host-side policy (csrc/loop_policy.h: PipeTuner, GuardRoute) under
# AddressSanitizer + UBSan, in the stand-alone program (tools/host_plan/loop_policy_main.cpp) over its whole scenario list.
# Plain C++: the header includes no HIP header and the program makes no HIP call.  Takes a few seconds.
# The output must still equal the record the host test compares with.  The same flags then build and run the other two plain
# C++ programs of tools/host_plan: the lane bookkeeping, and the host forms' staging path (csrc/host_stage.h).
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
/opt/rocm/bin/hipcc -x c++ -O1 -g -ffp-contract=off -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -fno-omit-frame-pointer "$R/tools/host_plan/loop_policy_main.cpp" -o "$T/loop_policy"
"$T/loop_policy" > "$T/out.txt"
"$T/loop_policy" eviction > /dev/null
cmp "$T/out.txt" "$R/tests/golden/loop_policy_v1.txt"
/opt/rocm/bin/hipcc -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -fno-omit-frame-pointer "$R/tools/host_plan/lane_busy_main.cpp" -o "$T/lane_busy"
"$T/lane_busy" > /dev/null   # (the pipeline's lane bookkeeping: LaneBusy, overlap_allowed)
/opt/rocm/bin/hipcc -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -fno-omit-frame-pointer "$R/tools/host_plan/host_stage_main.cpp" -o "$T/host_stage"
"$T/host_stage" > /dev/null  # (the host forms' staging path: csrc/host_stage.h, temporaries that outlive a wait that gave up)
echo "loop policy: $(wc -l < "$T/out.txt") steps, equal to tests/golden/loop_policy_v1.txt, no sanitizer report"
