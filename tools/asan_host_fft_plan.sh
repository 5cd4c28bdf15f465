#!/bin/bash
# Development aid (CPU only, no GPU needed): the FFT planner (csrc/fft_plan.h) under AddressSanitizer + UBSan, in the
# stand-alone dump program (tools/host_plan/fft_plan_dump_main.hip) over its whole case list -- every engine, loader, epilogue,
# the fused autocorrelation sequence, the whole-row launches, the error cases.  Host-only build: the planner makes no HIP call
# and no device code is compiled.  Takes a few seconds.  The output must still equal the record the host test compares with.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
/opt/rocm/bin/hipcc --cuda-host-only -O1 -g -ffp-contract=off -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -fno-omit-frame-pointer -I"$R/include" "$R/tools/host_plan/fft_plan_dump_main.hip" -o "$T/fft_plan_dump"
"$T/fft_plan_dump" > "$T/out.txt"
"$T/fft_plan_dump" --full ac-mid-2000000-sc8 > /dev/null
cmp "$T/out.txt" "$R/tests/golden/fft_plans_v1.txt"
echo "FFT planner: $(wc -l < "$T/out.txt") cases, equal to tests/golden/fft_plans_v1.txt, no sanitizer report"
