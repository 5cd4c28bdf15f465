#!/bin/bash
# Development aid (CPU only, no GPU needed): the image planner (csrc/image_plan.h) under AddressSanitizer + UBSan, in the
# stand-alone dump program (tools/host_plan/plan_dump_main.hip) over its whole case list -- every route, the error cases, the
# seeded sweep.  Host-only build: the planner makes no HIP call and no device code is compiled.  Takes a few seconds.
# The output must still equal the record the host test compares with.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
/opt/rocm/bin/hipcc --cuda-host-only -O1 -g -ffp-contract=off -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -fno-omit-frame-pointer -I"$R/include" "$R/tools/host_plan/plan_dump_main.hip" -o "$T/plan_dump"
"$T/plan_dump" > "$T/out.txt"
"$T/plan_dump" --full wl-C5-ras-fast-sc16-sums > /dev/null
cmp "$T/out.txt" "$R/tests/golden/image_plans_v1.txt"
echo "image planner: $(wc -l < "$T/out.txt") cases, equal to tests/golden/image_plans_v1.txt, no sanitizer report"
