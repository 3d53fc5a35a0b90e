#!/bin/bash
# AddressSanitizer + UBSan over the host form of multigather (rk_scaled_host.cpp: rk_multigather_scaled_host) as a stand-alone
# program: seeded random batches on 1 and 4 threads, plain and weighted, against the per-query host entries; every refusal.
# Host code only, no GPU needed.
# Usage: bash tools/asan_multigather/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_multigather; mkdir -p $W
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -o $W/multigather_asan
$W/multigather_asan 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
