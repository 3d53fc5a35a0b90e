#!/bin/bash
# AddressSanitizer + UBSan over the host half of scaled sketches (rk_scaled_host.cpp: rk_scaled_max_hash, rk_merge_scaled,
# rk_scaled_distance) as a stand-alone program: the hand-checked vectors of tests/golden/scaled_kat.json and 17-part merges.  Host
# code only, no GPU needed.
# Usage: bash tools/asan_scaled/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_scaled; mkdir -p $W
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -o $W/scaled_asan
python3 - $ROOT/tests/golden/scaled_kat.json > $W/vectors.txt <<'PY'
import json, sys
def side(pieces):
    out = []
    for p in pieces:
        out.extend(range(p[1], p[2], p[3]) if isinstance(p, list) else [p])
    return out
for v in json.load(open(sys.argv[1])):
    a, b = side(v["a"]), side(v["b"])
    print(v["want"], len(a), *a, len(b), *b)
PY
$W/scaled_asan $W/vectors.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
