#!/bin/bash
# usage: scripts/plan_diff.sh BASE_REV [JOBS]
# Builds librcv.so of BASE_REV in a temporary directory, runs scripts/plan_dump.py (the working tree's) against that build and against
# the working tree's robocupvision_amd/librcv.so (build it first), and prints the number of lines of the dump and of those that differ.
# Exit status 0: every record of the dump is routed alike by both -- return code, error text, workspace, label, filter layout.  Needs
# hipcc, no GPU.
set -euo pipefail
BASE=${1:?usage: scripts/plan_diff.sh BASE_REV [JOBS]}
JOBS=${2:-8}
[ "$JOBS" -le 16 ] || JOBS=16
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=robocupvision_amd/csrc
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
mkdir -p "$T/base"
git -C "$ROOT" archive "$BASE" -- $CSRC include | tar -x -C "$T/base"
make -s -C "$T/base/$CSRC" -j"$JOBS" >/dev/null

RCV_LIBRARY="$T/base/robocupvision_amd/librcv.so" python "$ROOT/scripts/plan_dump.py" > "$T/base.txt"
env -u RCV_LIBRARY python "$ROOT/scripts/plan_dump.py" > "$T/head.txt"
n=$(diff "$T/base.txt" "$T/head.txt" | grep -c '^[<>]' || true)
echo "plan dump: $(wc -l < "$T/head.txt") lines, $n differing lines"
if [ "$n" != 0 ]; then diff "$T/base.txt" "$T/head.txt" | head -40; exit 1; fi
