#!/usr/bin/env bash
# Host sanitizers on the CPU oracle (oracle/fmcw_cpu.c): AddressSanitizer + UBSan, run here.
# The program is built into a directory of its own (mktemp), so another user's or an earlier
# run's file under a fixed name can never be in the way.
set -euo pipefail
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
gcc -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all -fopenmp -std=gnu11 \
    -Wall -Wno-unused-result -o "$D/oracle_asan" tools/oracle_asan.c -lm
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$D/oracle_asan"
