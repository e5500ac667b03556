#!/usr/bin/env bash
# The host side of the FSAI preconditioner (csrc/fsai.cpp) and the host builder under AddressSanitizer +
# UndefinedBehaviorSanitizer, in a stand-alone program (tools/fsai_check.cpp): no GPU, no Python.
#   bash tools/asan_fsai.sh
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
SRC="$ROOT/ehyb_spmv_gpu_amd/csrc"
TMP="$(mktemp -d)"
trap 'rm -rf "$TMP"' EXIT
FLAGS="-O1 -g -fopenmp -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$SRC"
for f in common partition reorder layout er_panel col_triples plan plan_io matrix_io fsai; do
    g++ $FLAGS -c "$SRC/$f.cpp" -o "$TMP/$f.o" &
done
wait
g++ $FLAGS "$ROOT/tools/fsai_check.cpp" "$TMP"/*.o -o "$TMP/fsai_check" -lz -ldl
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$TMP/fsai_check"
