#!/bin/bash
# Development aid (no GPU needed): show that a host-only change left the device code alone.  Compiles every translation unit
# of a git revision and of the working tree for the device only (build.py's flags) and compares the SHA-256 of the .text and
# .rodata sections of the gfx950 ELFs (the whole object always differs: it carries a per-compilation id).  Where a unit
# differs, the kernels' names, sizes and register / LDS / scratch figures of both sides are diffed instead.
#   tools/device_code_hash.sh [git-ref, default HEAD]        exit status 0: every section equal
set -e
REF=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
# the LLVM tools beside hipcc: ROCm keeps them under llvm/bin or lib/llvm/bin; llvm-readelf is llvm-readobj in its GNU style
LLVM=$LLVM_BIN
for d in /opt/rocm/llvm/bin /opt/rocm/lib/llvm/bin; do [ -n "$LLVM" ] || { [ -x "$d/llvm-objcopy" ] && LLVM=$d; }; done
[ -n "$LLVM" ] || { echo "no llvm-objcopy under /opt/rocm (set LLVM_BIN)" >&2; exit 2; }
readelf() { if [ -x "$LLVM/llvm-readelf" ]; then "$LLVM/llvm-readelf" "$@"; else "$LLVM/llvm-readobj" --elf-output-style=GNU "$@"; fi; }
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS=$(cd "$ROOT" && python3 -c "
import importlib.util as u
s = u.spec_from_file_location('b', 'tempestsdr.jl_amd/build.py'); b = u.module_from_spec(s); s.loader.exec_module(b)
print(' '.join(b.FLAGS))")
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/old" "$TMP/new/tempestsdr.jl_amd" "$TMP/o"
git -C "$ROOT" archive "$REF" tempestsdr.jl_amd/csrc include | tar -x -C "$TMP/old"
cp -r "$ROOT/tempestsdr.jl_amd/csrc" "$TMP/new/tempestsdr.jl_amd/" && cp -r "$ROOT/include" "$TMP/new/"
for side in old new; do
  for f in "$TMP/$side"/tempestsdr.jl_amd/csrc/*.hip; do
    echo "$side $(basename "$f" .hip)"
  done
done | xargs -P "${JOBS:-8}" -L 1 bash -c '
  e='"$TMP"'/o/$0.$1.elf
  '"$HIPCC $FLAGS"' -w --cuda-device-only --no-gpu-bundle-output -c '"$TMP"'/$0/tempestsdr.jl_amd/csrc/$1.hip -o $e
  for s in text rodata; do '"$LLVM"'/llvm-objcopy -O binary --only-section=.$s $e $e.$s; done'
figures() {  # kernel symbols with their sizes, then each kernel's resource figures from the code object's metadata note
  # (both sorted by name: a host-side change may move the order in which kernels are emitted; the per-source id symbol
  # __hip_cuid_* differs whenever the source text does)
  readelf -sW "$1" | awk '($4 == "FUNC" || $4 == "OBJECT") && $8 !~ /^__hip_cuid_/ { print $8, $3 }' | sort
  readelf --notes "$1" | grep -E '^ +\.(name|sgpr_count|vgpr_count|agpr_count|sgpr_spill_count|vgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size|kernarg_segment_size|max_flat_workgroup_size):' | sed 's/^ *//' |
    awk '{ k = $1 } k in seen { print name, rec; delete seen; rec = "" } { seen[k] = 1; if (k == ".name:") name = $2; else rec = rec " " $1 $2 } END { if (rec != "") print name, rec }' | sort
}
bad=0
for f in "$TMP"/new/tempestsdr.jl_amd/csrc/*.hip; do
  n=$(basename "$f" .hip); line="$n"; same=1
  for s in text rodata; do
    a=$(sha256sum < "$TMP/o/old.$n.elf.$s" | cut -c1-16); b=$(sha256sum < "$TMP/o/new.$n.elf.$s" | cut -c1-16)
    [ "$a" = "$b" ] && line="$line  .$s $a ==" || { line="$line  .$s $a != $b"; same=0; }
  done
  echo "$line"
  if [ $same = 0 ]; then
    bad=1
    figures "$TMP/o/old.$n.elf" > "$TMP/o/$n.old.fig"; figures "$TMP/o/new.$n.elf" > "$TMP/o/$n.new.fig"
    if diff "$TMP/o/$n.old.fig" "$TMP/o/$n.new.fig"; then echo "  $n: $(grep -c ' \.sgpr_count:' "$TMP/o/$n.new.fig") kernels, same symbols, sizes and register / LDS / scratch figures"; fi
  fi
done
exit $bad
