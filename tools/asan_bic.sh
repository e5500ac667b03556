#!/usr/bin/env bash
# The host side of the block incomplete Cholesky preconditioner (csrc/bic.cpp) and the host builder under AddressSanitizer +
# UndefinedBehaviorSanitizer, in a stand-alone program (tools/bic_check.cpp): no GPU, no Python.
#   bash tools/asan_bic.sh
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
SRC="$ROOT/ehyb_spmv_gpu_amd/csrc"
TMP="$(mktemp -d)"
trap 'rm -rf "$TMP"' EXIT
FLAGS="-O1 -g -fopenmp -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$SRC"
for f in common partition reorder layout er_panel col_triples plan plan_io matrix_io fsai bic; do
    g++ $FLAGS -c "$SRC/$f.cpp" -o "$TMP/$f.o" &
done
wait
g++ $FLAGS "$ROOT/tools/bic_check.cpp" "$TMP"/*.o -o "$TMP/bic_check" -lz -ldl
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$TMP/bic_check"
