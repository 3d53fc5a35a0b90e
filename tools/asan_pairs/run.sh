#!/bin/bash
# AddressSanitizer + UBSan over the host half of sketch comparison (rk_pairs_host.cpp: rk_merge_sketches, rk_mash_distance) as a
# stand-alone program: the hand-checked vectors of tests/golden/pairs_kat.json and 17-part merges.  Host code only, no GPU needed.
# Usage: bash tools/asan_pairs/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_pairs; mkdir -p $W
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_pairs_host.cpp -o $W/pairs_asan
python3 - $ROOT/tests/golden/pairs_kat.json > $W/vectors.txt <<'PY'
import json, sys
for v in json.load(open(sys.argv[1])):
    print(v["S"], v["k"], v["want"][2], v["want"][3], repr(v["jaccard"]), repr(v["distance"]), len(v["a"]), *v["a"], len(v["b"]), *v["b"])
PY
$W/pairs_asan $W/vectors.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
