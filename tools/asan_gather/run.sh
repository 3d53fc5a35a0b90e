#!/bin/bash
# AddressSanitizer + UBSan over the host form of gather (rk_scaled_host.cpp: rk_gather_scaled_host) as a stand-alone program: the
# hand-checked vectors of tests/golden/gather_kat.json on 1 and 4 threads, seeded random sets against a plain loop, every refusal.
# Host code only, no GPU needed.
# Usage: bash tools/asan_gather/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_gather; mkdir -p $W
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -o $W/gather_asan
python3 - $ROOT/tests/golden/gather_kat.json > $W/vectors.txt <<'PY'
import json, sys
def side(pieces):
    out = []
    for p in pieces:
        out.extend(range(p[1], p[2], p[3]) if isinstance(p, list) else [p])
    return out
for v in json.load(open(sys.argv[1])):
    q, refs = side(v["q"]), [side(r) for r in v["refs"]]
    row = [v["min_shared"], v["max_rounds"] or len(refs), len(v["want"])] + [x for w in v["want"] for x in w] + [len(q)] + q + [len(refs)]
    for r in refs:
        row += [len(r)] + r
    print(*row)
PY
$W/gather_asan $W/vectors.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
