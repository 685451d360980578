#!/usr/bin/env bash
# Host sanitizers on the record-list layer (csrc/rec_window.hpp, csrc/unfold_window.hpp): builds
# tools/reclist_replay.cpp host-only with AddressSanitizer + UBSan (clang links their runtime statically:
# nothing is preloaded) and runs it, here, on the CPU.
#
#   tools/reclist_replay.sh CASE RESULT   build into a directory of its own (mktemp), replay one case file,
#                                         remove the directory on exit
#   tools/reclist_replay.sh -o DIR        build DIR/reclist_replay only: for a caller that replays many
#                                         cases and owns DIR (tests/test_reclist_replay.py, in pytest's
#                                         temporary directory)
# Nothing is ever built into the tree.
set -euo pipefail
USAGE="usage: $0 -o DIR | CASE RESULT"
[ $# -eq 2 ] || { echo "$USAGE" >&2; exit 2; }
A=$(realpath "$1" 2>/dev/null || echo "$1")   # the arguments may be relative to the caller's directory
B=$(realpath "$2")
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
build() {
  "$HIPCC" -x hip --offload-host-only -O1 -g -std=c++17 -ffp-contract=off -fno-omit-frame-pointer \
      -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all -Wall \
      -I fpga-fmcw-radar-processor_amd/csrc -o "$1/reclist_replay" tools/reclist_replay.cpp
}
if [ "$1" = "-o" ]; then
  [ -d "$B" ] || { echo "$USAGE" >&2; exit 2; }
  build "$B"
  exit 0
fi
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
build "$D"
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$D/reclist_replay" "$A" "$B"
