#!/bin/bash
# AddressSanitizer + UBSan over the host half of bottom samples (rk_bottom_host.cpp: rk_bottom_emit) and the text side of
# --min-copies (rkmh_min_copies.hpp) as a stand-alone program.  Host code only, no GPU needed.
# Usage: bash tools/asan_bottom/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_bottom; mkdir -p $W
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/rkmh_amd/csrc $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_bottom_host.cpp -o $W/bottom_asan
$W/bottom_asan 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
