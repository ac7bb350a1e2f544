#!/bin/bash
# usage: scripts/isa_diff.sh BASE_REV [JOBS]
# Compiles every csrc/*.hip of BASE_REV and of the working tree device-only to gfx950 assembly (the Makefile's flags) and prints, per
# file, the number of differing lines -- ignoring the lines with __hip_cuid_, a hash of the source text -- and, per kernel, the
# register / spill / scratch figures that changed.  A file that only the working tree has and that defines no kernel is reported as
# "host only".  Exit status 0: identical device code everywhere.  Needs hipcc, no GPU.
set -euo pipefail
BASE=${1:?usage: scripts/isa_diff.sh BASE_REV [JOBS]}
JOBS=${2:-8}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=robocupvision_amd/csrc
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
mkdir -p "$T/base" "$T/asm/base" "$T/asm/head"
git -C "$ROOT" archive "$BASE" -- $CSRC include | tar -x -C "$T/base"
HIPCC=$(make -s -C "$ROOT/$CSRC" --eval 'isa-hipcc: ; @echo $(HIPCC)' isa-hipcc)
FLAGS=$(make -s -C "$ROOT/$CSRC" --eval 'isa-flags: ; @echo $(CXXFLAGS)' isa-flags)

{ for f in "$T/base/$CSRC"/*.hip; do echo "$f $T/asm/base/$(basename "$f" .hip).s"; done
  for f in "$ROOT/$CSRC"/*.hip; do echo "$f $T/asm/head/$(basename "$f" .hip).s"; done; } |
  xargs -P "$JOBS" -L 1 sh -c "$HIPCC $FLAGS -Wno-unused-command-line-argument --cuda-device-only -S \"\$0\" -o \"\$1\""

# kernel name -> "vgpr spill scratch" from the .amdhsa metadata of one assembly file
meta() {
  awk '/\.name:/ { name = $NF }
       /\.private_segment_fixed_size:/ { p = $NF }
       /\.vgpr_count:/ { v = $NF }
       /\.vgpr_spill_count:/ { s = $NF }
       /\.wavefront_size:/ { print name, v, s, p }' "$1" | sort
}

status=0
for name in $(cd "$T/asm" && ls base head | grep '\.s$' | sort -u); do
  b="$T/asm/base/$name"; h="$T/asm/head/$name"
  if [ ! -f "$b" ] && ! grep -q '\.amdhsa_kernel' "$h"; then echo "${name%.s}.hip: host only"; continue; fi      # a new file without kernels
  if [ ! -f "$b" ] || [ ! -f "$h" ]; then echo "${name%.s}.hip: only in $([ -f "$b" ] && echo "$BASE" || echo "the working tree")"; status=1; continue; fi
  n=$(diff <(grep -v __hip_cuid_ "$b") <(grep -v __hip_cuid_ "$h") | grep -c '^[<>]' || true)
  echo "${name%.s}.hip: $n differing lines"
  if [ "$n" != 0 ]; then
    status=1
    join -a 1 -a 2 -e - -o 0,1.2,1.3,1.4,2.2,2.3,2.4 <(meta "$b") <(meta "$h") |
      awk '$2 != $5 || $3 != $6 || $4 != $7 { printf "  %s: vgpr_count %s -> %s, vgpr_spill_count %s -> %s, private_segment_fixed_size %s -> %s\n", $1, $2, $5, $3, $6, $4, $7 }'
  fi
done
exit $status
