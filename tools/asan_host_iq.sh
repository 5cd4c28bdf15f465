#!/bin/bash
# Development aid (CPU only, no GPU needed): the argument-checking host code of the integer IQ entry points under
# AddressSanitizer + UBSan, in a stand-alone program (tools/host_asan/iq_args_main.hip).  Only the HOST side of every translation
# unit gets the sanitizers (-Xarch_host); the device code is compiled too, at -O1, only because the host objects refer to their
# code objects -- nothing here launches a kernel.  Takes a few minutes.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
FLAGS="--offload-arch=gfx950 -O1 -g -ffp-contract=off -std=c++17 -w -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -I$R/include"
pids=()
for f in "$R"/tempestsdr.jl_amd/csrc/*.hip "$R"/tools/host_asan/iq_args_main.hip; do
  /opt/rocm/bin/hipcc $FLAGS -c "$f" -o "$T/$(basename "$f" .hip).o" & pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o "$T/iq_args" "$T"/*.o -ldl
ASAN_OPTIONS=detect_leaks=0 "$T/iq_args"
